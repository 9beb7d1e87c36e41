"""k_emit2's fused queue role loads its whole prologue in one round; the died bitmap's copy
into LDS and the slot purge with a folded commit load through clamped indices too.  All three
against the oracle, at the shapes where clamped, fixed-count loads can go wrong.

k_emit2's fused queue blocks read every group row and the rows of the earlier blocks of
their own group with a fixed number of clamped loads (csrc/faasbal_kernels.h:
fused_row_loads): queues of 1 .. 257 blocks at each table width, the last block partial and
full, with a worker dying in the first and in the last block of a group.  The group
geometry comes from plan_tick (tests/plan_probe.cpp), and the launches are observed
(fb_timing_read): a case that left the fused path would test nothing here.

Everything is bit-exact: assignments, orphans, evicted slots, the result record and the next
state (tests/test_gpu_parity.py's helpers).
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import plan_cases as pc
from test_gpu_parity import _cmp_out, _cmp_state, _pair

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
NOW, TTE = 1000.0, 10.0
ALIVE, DEAD = NOW - 1.0, NOW - 100.0
BS = 256       # positions per queue block, slots per slot tile
FTILE = 2048   # log entries per log tile


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """plan_tick's answer for a one-GPU heartbeat context's idle tick: {key: value}."""
    if shutil.which("hipcc") is None:
        pytest.fail("hipcc not found: the plan probe cannot be compiled")
    exe = str(tmp_path_factory.mktemp("plan") / "plan_probe")
    subprocess.run(["hipcc", "-std=c++17", "-O1", "-I" + os.path.join(REPO, "distributed-faas_amd", "csrc"),
                    "-I" + os.path.join(REPO, "include"), os.path.join(HERE, "plan_probe.cpp"), "-o", exe], check=True)

    def ask(W, maxfree, H, Qn, T, **more):
        f = dict(pc.context_inputs("local", W, maxfree, H, {}), Qn=Qn, T=T, **more)
        line = "plan" + "".join(" %s=%d" % kv for kv in f.items()) + "\n"
        out = subprocess.run([exe], input=line, capture_output=True, text=True, check=True).stdout
        ans = dict(w.split("=", 1) for w in out.split())
        assert "error" not in ans, (line, out)
        return ans

    return ask


def _state(W, Q, maxfree, H, seed, dead_pos=(), dead_frac=0.03):
    """W registered workers, the first Q of a random order queued, free counts 1 .. maxfree
    (one live worker holds maxfree: the table width follows the largest), dead_frac of them
    and the workers at queue positions dead_pos expired, H in-flight entries."""
    rng = np.random.default_rng(seed)
    free = rng.integers(1, maxfree + 1, W).astype(np.int32)
    hb = np.where(rng.random(W) < dead_frac, DEAD, ALIVE)
    queue = rng.permutation(W).astype(np.int32)[:Q]
    free[queue[Q // 2]] = maxfree
    hb[queue[Q // 2]] = ALIVE
    for p in dead_pos:
        if p != Q // 2:
            hb[queue[p]] = DEAD
    log = rng.integers(0, W, H).astype(np.int32)
    return dict(reg=np.ones(W, np.uint8), free=free, hb=hb, epoch=np.zeros(W, np.uint32), queue=queue, log=log)


def _tasks(st, levels=2):
    """Tasks for `levels` full rounds and a third of the next (less the orphans that come first)."""
    q = st["queue"]
    alive = int((st["hb"][q] > NOW - TTE).sum())
    return max(alive * levels + alive // 3, 1)


def _idle_tick(g, o, T, t=0, fused=True):
    """One committed idle tick on both, compared; the GPU's launches returned."""
    g.timing_enable(True)
    g.timing_read()
    args = (NOW + 1.5 * t, TTE, [], [], [], [], [], T)
    a, b = g.tick(*args), o.tick(*args)
    kt = {k: int(v[1]) for k, v in g.timing_read().items()}
    g.timing_enable(False)
    _cmp_out(a, b, t)
    # the result record
    ex = o.export()
    assert a["result"]["n_assigned"] == len(b["assign"]) and a["result"]["n_orphans"] == len(b["orphans"])
    assert a["result"]["n_evicted"] == len(b["evicted"])
    assert a["result"]["queue_len"] == len(ex["queue"]) and a["result"]["log_head"] == ex["head"]
    if fused:
        assert set(kt) == {"scan", "emit"}, kt  # two launches: no k_plan / k_logscan / k_slots
    return a, b, kt


NBQ = [1, 2, 4, 5, 16, 17, 64, 65, 128]
ROW_CASES = ([(32, n, full) for n in NBQ + [257] for full in (False, True)] +
             [(64, n, full) for n in NBQ for full in (False, True)] +
             [(128, n, full) for n in NBQ for full in (False, True)])  # (128 rows: the fused limit is 128 blocks)


@pytest.mark.parametrize("maxfree,nbq,full", ROW_CASES,
                         ids=["R%d-nbq%d-%s" % (r, n, "full" if f else "partial") for r, n, f in ROW_CASES])
def test_group_and_block_row_clamps(plan, maxfree, nbq, full):
    """Fused ticks whose queue fills nbq blocks at R = 32 / 64 / 128: every block's prefix from
    the group rows before its group and the block rows before it inside the group (both clamped
    at their last row, the block rows also where a group's first block has none before it)."""
    Q = nbq * BS if full else (nbq - 1) * BS + 77
    W, H = Q + 5, 2 * FTILE + 300
    p = plan(W, maxfree, H, Q, 1)
    assert (p["fused"], p["f_emit"], p["grp_on"]) == ("1", "1", "1"), p
    ngrp = int(p["ngrp"])
    gsz = next(s for s in (1 << k for k in range(12)) if -(-nbq // s) == ngrp)  # blocks per group row
    assert ngrp <= 32 and gsz <= 32  # what the fixed load counts rest on (fused_row_loads)
    # a worker dying in the first and in the last block of a group (the second group, or the only one)
    g0 = min(1, ngrp - 1) * gsz
    g1 = min(g0 + gsz, nbq) - 1
    dead_pos = [min(g0 * BS + 7, Q - 1), min(g1 * BS + 70, Q - 1)]
    st = _state(W, Q, maxfree, H, 1000 * maxfree + 2 * nbq + full, dead_pos)
    g, o = _pair(st, H + 4 * W * 4 + 4096)
    try:
        a, b, _ = _idle_tick(g, o, _tasks(st))
        for pos in dead_pos:
            assert st["queue"][pos] in b["evicted"]
        _cmp_state(g, o, 0)
    finally:
        g.close()


@pytest.mark.parametrize("maxfree,nbq", [(32, 5), (64, 17), (128, 65)])
def test_both_position_sources(maxfree, nbq):
    """The same state as an idle tick (k_emit2 reads the committed per-position arrays itself)
    and as a tick with one heartbeat message (the events instance: k_scan's c_arr / c_hb)."""
    Q = (nbq - 1) * BS + 131
    W, H = Q + 9, FTILE + 50
    st = _state(W, Q, maxfree, H, 77 + nbq, [3, Q - 2])
    T = _tasks(st)
    g, o = _pair(st, H + 4 * W * 4 + 4096)
    try:
        _idle_tick(g, o, T)
        _cmp_state(g, o, 0)
    finally:
        g.close()
    g, o = _pair(st, H + 4 * W * 4 + 4096)
    try:
        s = int(st["queue"][Q // 2])  # a live, queued worker
        args = (NOW, TTE, np.array([pc.EV_HEARTBEAT], np.uint8), np.array([s], np.int32), np.zeros(1, np.int32),
                np.array([NOW], np.float64), np.full(1, -1, np.int64), T)
        a, b = g.tick(*args), o.tick(*args)
        _cmp_out(a, b, 0)
        assert a["result"]["n_evicted"] == len(b["evicted"]) > 0
        _cmp_state(g, o, 0)
    finally:
        g.close()


@pytest.mark.parametrize("knobs", [{}, {"plan": 1, "split_slots": 1}], ids=["emit2_log_tiles", "scan_log_role"])
@pytest.mark.parametrize("W", [1, 63, 65, 4097, 65536, 131072])
def test_bitmap_copy(W, knobs):
    """The died bitmap staged in LDS by whole int4 (1 .. 1024 of them, the last one clamped):
    slots 0 and W - 1 die with in-flight entries in the first and in the last log tile.  By
    k_emit2's log workgroups (fused ticks) and by k_scan's log role (k_slots wrote the bitmap)."""
    H = 2 * FTILE + 333
    st = _state(W, W, 32, H, 5 + W, dead_frac=0.0)
    mine = {3: 0, 5: W - 1, H - 2: 0, H - 4: W - 1}
    for e, s in mine.items():
        st["log"][e] = s
    st["hb"][0] = st["hb"][W - 1] = DEAD
    if W > 1:  # (W = 1: nobody left to serve)
        st["free"][1], st["hb"][1] = 32, ALIVE
    g, o = _pair(st, H + 2 * W + 8192)
    try:
        for k, v in knobs.items():
            g.set_path(k, v)
        a, b, kt = _idle_tick(g, o, min(W, 3000), fused=not knobs)
        if knobs:
            assert "slots" in kt and "scan" in kt, kt  # k_slots wrote the bitmap, k_scan has the log role
        assert set(mine) <= set(int(x) for x in b["orphans"])
        want = np.nonzero(np.isin(st["log"], [0, W - 1]))[0]
        np.testing.assert_array_equal(np.sort(a["orphans"]), want)
        _cmp_state(g, o, 0)
    finally:
        g.close()


def test_folded_commit_in_last_slot_tile():
    """Three committed idle ticks back to back, W no multiple of 256 and the last slot evicted by
    the first tick: its record's deletion rides in the second tick's slot purge (which reads the
    previous status byte and the budget beside the record), in the last, partial tile.  Then a tick
    launched twice without a commit between: identical outputs, the oracle's."""
    from faasbal import synth

    W = 8192 + 77
    st = synth.zipf_state(W=W, seed=11, dead_frac=0.05)
    st["hb"][W - 1] = DEAD  # evicted by the first tick
    st["hb"][W - 3] = NOW + 1.0 - TTE  # alive at the first tick, expired at the second
    st["log"][10] = W - 1
    st["log"][len(st["log"]) - 1] = W - 3
    T = 3 * W
    g, o = _pair(st, len(st["log"]) + 8 * T + 16)
    try:
        carried = 0
        for t in range(3):
            n = carried + T
            a, b, _ = _idle_tick(g, o, n, t)
            if t == 0:
                assert W - 1 in b["evicted"]
            if t == 1:
                assert W - 3 in b["evicted"]
            carried = n + len(b["orphans"]) - len(b["assign"])
        n = carried + T
        outs = []
        for _ in range(2):
            g.launch(NOW + 4.5, TTE, n_pending=n)
            g.wait()
            outs.append(dict(reconnect=g.event_status(), assign=g.assignments(), orphans=g.orphans(),
                             evicted=g.evicted()))
        b = o.tick(NOW + 4.5, TTE, [], [], [], [], [], n)
        _cmp_out(outs[0], b, 3)
        _cmp_out(outs[1], b, 3)
        g.commit()
        _cmp_state(g, o, 3)
    finally:
        g.close()
