"""A shard group's reclaim on the GPU: fb_log_reclaim_shard behind LocalShardGroup.reclaim
(every rank's context on one device) and DistShardGroup.reclaim (two processes over gloo).

The reference of every comparison is tests/reclaim_model.reclaim_model applied to the merged
state read before the call, split per rank again (tests/test_log_reclaim_shard_host.py's
check_group_reclaim, which runs the same checks over model ranks), and -- where ticks run --
a one-GPU twin (GpuBalancer, fb_log_reclaim), itself tested against the oracle in
tests/test_gpu_log_reclaim.py.  Every comparison is exact.
"""
import ctypes as C

import numpy as np
import pytest

from faasbal import FaasbalError, GpuBalancer, _lib, synth
from faasbal._lib import FB_EINVAL, FB_ESTATE
from faasbal.sharded import LocalShardGroup, merge_states, shard_range, split_state
from reclaim_model import reclaim_model, slots_mask
from test_log_reclaim_shard_host import MARKED, _scripted, check_group_reclaim

pytestmark = pytest.mark.gpu

STATE_KEYS = ("reg", "free", "hb", "epoch", "queue", "log", "head")
SEAMS = (0, 1, 63, 64, 65, 2047, 2048, 2049, 4 * 2048 + 1)  # (the last: five tiles, a second workgroup)
CAP = 3 * 4096  # a rank's log


def _rank_states(g):
    return [b.read_state() for b in g.bals]


def _same(a, b, what, keys=STATE_KEYS):
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg="%s: %s" % (what, k))


def _unchanged(g, before, what):
    for r, (x, y) in enumerate(zip(_rank_states(g), before)):
        _same(x, y, "%s, rank %d" % (what, r))
        np.testing.assert_array_equal(x["log_seq"], y["log_seq"], err_msg=what)
        assert x["log_len"] == y["log_len"], what


def _raw(b, below, mask, want_seq, want_slot, cap):
    """fb_log_reclaim_shard through ctypes: (rc, count, seq, slot); the arrays pre-filled with -7."""
    seq = np.full(max(cap, 1), -7, np.int64)
    slot = np.full(max(cap, 1), -7, np.int32)
    n = C.c_int64(-7)
    rc = b.lib.fb_log_reclaim_shard(b.h, int(below), None if mask is None else mask.ctypes.data_as(C.c_void_p),
                                    seq.ctypes.data_as(C.c_void_p) if want_seq else None,
                                    slot.ctypes.data_as(C.c_void_p) if want_slot else None, int(cap), C.byref(n))
    return rc, n.value, seq, slot


def _raises(code, f, *a, needle=None, **k):
    with pytest.raises(FaasbalError) as e:
        f(*a, **k)
    assert e.value.code == code, e.value
    if needle is not None:
        assert needle in str(e.value), e.value


# ------------------------------------------------------------------ 1. the seams
def seam_state(rng, W, world, lengths):
    """A global state whose rank r holds lengths[r] log entries, the ranks' sequences
    interleaved; some slots hold no record and some registrations are younger than entries
    on their slot (fb_load_shard leaves those in the shard, at -1)."""
    parts = []
    for r, n in enumerate(lengths):
        base, cnt = shard_range(W, world, r)
        parts.append(rng.integers(base, base + cnt, n) if cnt else np.zeros(0, np.int64))
    log = np.concatenate(parts).astype(np.int32)
    log = log[rng.permutation(len(log))]
    head = len(log)
    reg = (rng.random(W) < 0.85).astype(np.uint8)
    epoch = np.where(rng.random(W) < 0.7, 0, rng.integers(0, head + 2, W)).astype(np.uint32)
    q = rng.permutation(np.flatnonzero(reg)).astype(np.int32)
    return dict(reg=reg, free=rng.integers(0, 5, W).astype(np.int32), hb=rng.random(W) + 1000.0, epoch=epoch,
                queue=q[: len(q) // 2], log=log)


def bounds_of(seq, head):
    """Bounds placed by a shard's own sequences: below its first, inside a word, at a word
    boundary, at a tile boundary, above its last, at and past the head."""
    idx = [i for i in (0, 1, 37, 64, 100, 2047, 2048, 2049, 4096, len(seq) - 1) if 0 <= i < len(seq)]
    out = {0, head, head + 7} | {int(seq[i]) for i in idx}
    if len(seq):
        out.add(int(seq[-1]) + 1)
    return sorted(out)


def check_ranks(g, world, ranks_pre, below, slots, what):
    """check_group_reclaim's comparisons from one read of the ranks before the call (the last
    call's read after it) and one after: the group's lists and every rank's read-back state
    against reclaim_model of the merged state; returns (the result, the ranks' states after)."""
    W = g.n_workers_global
    pre = merge_states(ranks_pre, W)
    want, seq, slot, _ = reclaim_model(pre, below, None if slots is None else slots_mask(W, slots))
    out = g.reclaim(below, slots)
    assert out["n"] == len(seq), what
    np.testing.assert_array_equal(out["seq"], seq, err_msg=what + ": seq")
    np.testing.assert_array_equal(out["slot"], slot, err_msg=what + ": slot")
    assert out["seq"].dtype == np.int64 and out["slot"].dtype == np.int32, what
    ranks = _rank_states(g)
    for r, (rs, p) in enumerate(zip(ranks, ranks_pre)):
        # log_seq, heads, queue, free, hb and epoch are unchanged; the taken entries are -1 in place
        for k in ("reg", "free", "hb", "epoch", "queue", "log_seq", "head", "log_len"):
            np.testing.assert_array_equal(rs[k], p[k], err_msg="%s: rank %d %s" % (what, r, k))
        mine = np.isin(np.asarray(p["log_seq"], np.int64), seq)
        np.testing.assert_array_equal(rs["log"], np.where(mine, -1, p["log"]), err_msg="%s: rank %d log" % (what, r))
        w = split_state(want, world, r)
        np.testing.assert_array_equal(rs["log"][rs["log"] >= 0], w["log_slot"], err_msg="%s: rank %d live" % (what, r))
    np.testing.assert_array_equal(merge_states(ranks, W)["log"], want["log"], err_msg=what + ": log")
    return out, ranks


@pytest.mark.parametrize("world,W", ((1, 41), (2, 41), (3, 300), (4, 41), (4, 5)))
def test_seams_against_the_model(world, W):
    """Local lengths at every seam of a word, a tile and a workgroup, rotated over the ranks
    (so a rank with an empty shard is among them); W = 5 over four ranks leaves the last
    without a slot.  Per mask the bounds go up over one loaded state, so that later calls find
    the earlier ones' entries at -1 in place."""
    rng = np.random.default_rng(9100 + 10 * world + W)
    g = LocalShardGroup(world, W, CAP, max_events=64)
    if (world, W) == (4, 5):
        assert shard_range(W, world, 3)[1] == 0
    taken = 0
    try:
        for b in g.bals:
            b.timing_enable(True)
        for i in range(len(SEAMS)):
            lengths = [SEAMS[(i + r) % len(SEAMS)] if shard_range(W, world, r)[1] else 0 for r in range(world)]
            st = seam_state(rng, W, world, lengths)
            head = len(st["log"])
            masks = {"none": None, "zero": [], "one": [int(rng.integers(0, W))], "alternate": list(range(0, W, 2))}
            for mname, slots in masks.items():
                g.load(st)
                ranks = _rank_states(g)
                assert [s["log_len"] for s in ranks] == lengths
                for below in bounds_of(ranks[i % world]["log_seq"], head):
                    what = "world %d W %d lengths %s mask %s below %d" % (world, W, lengths, mname, below)
                    out, ranks = check_ranks(g, world, ranks, below, slots, what)
                    taken += out["n"]
        assert taken > 1000
        for b in g.bals:  # the library's own kernels ran, on every rank that owns a slot
            names = b.timing_read(64)
            assert b.n_local == 0 or all(k in names for k in ("lr_flag", "lc_scan", "lr_take")), names
    finally:
        g.close()


def test_raw_call_cap_and_arguments():
    """cap too small: FB_EINVAL, the count comes back, nothing changed; the second call with
    room succeeds.  NULL outputs, one output, below_seq < 0, cap < 0, a one-GPU context."""
    rng = np.random.default_rng(9200)
    W, world = 41, 2
    st = seam_state(rng, W, world, [2049, 700])
    g = LocalShardGroup(world, W, CAP, max_events=64)
    try:
        g.load(st)
        before = _rank_states(g)
        pre = g.read_state()
        want, seq, slot, _ = reclaim_model(pre, None, None)
        for r, b in enumerate(g.bals):
            base, cnt = shard_range(W, world, r)
            mine = (slot >= base) & (slot < base + cnt)
            n = int(mine.sum())
            assert n > 100
            rc, got, sq, sl = _raw(b, 1 << 40, None, True, True, n - 1)
            assert (rc, got) == (FB_EINVAL, n) and (sq == -7).all() and (sl == -7).all()
            rc, got, sq, sl = _raw(b, 1 << 40, None, False, True, 0)  # (the group's count step)
            assert (rc, got) == (FB_EINVAL, n) and (sl == -7).all()
            assert b.reclaim_part(count_only=True) == {"n": n, "seq": None, "slot": None}
            assert _raw(b, -1, None, False, False, 0)[0] == FB_EINVAL
            assert _raw(b, 0, None, True, True, -1)[0] == FB_EINVAL
            now = b.read_state()
            _same(now, before[r], "refused arguments, rank %d" % r)
            np.testing.assert_array_equal(now["log_seq"], before[r]["log_seq"])
            if r == 0:  # with room: both lists
                rc, got, sq, sl = _raw(b, 1 << 40, np.full(cnt, 255, np.uint8), True, True, n)
                assert (rc, got) == (0, n)
                np.testing.assert_array_equal(sq[:n], seq[mine])
                np.testing.assert_array_equal(sl[:n], slot[mine])
            else:  # no outputs: cap is not looked at
                rc, got, sq, sl = _raw(b, pre["head"], None, False, False, 0)
                assert (rc, got) == (0, n) and (sq == -7).all() and (sl == -7).all()
        _same(g.read_state(), dict(want, head=pre["head"]), "after the raw calls")
        # a one-GPU context is sent to fb_log_reclaim, unchanged
        o = GpuBalancer(W, CAP, max_events=64)
        o.load(st)
        so = o.read_state()
        rc, got, _, _ = _raw(o, 10, None, True, True, 64)
        assert rc == FB_ESTATE and got == -7 and "use fb_log_reclaim" in o.lib.fb_last_error(o.h).decode()
        _same(o.read_state(), so, "one-GPU context", keys=STATE_KEYS[:-1])
        o.close()
    finally:
        g.close()


# ------------------------------------------------------------------ 2. world 1 is fb_log_reclaim
def test_world_1_is_fb_log_reclaim():
    rng = np.random.default_rng(9300)
    W = 48
    st = seam_state(rng, W, 1, [2049 + 700])
    g = LocalShardGroup(1, W, CAP, max_events=64)
    o = GpuBalancer(W, CAP, max_events=64)
    try:
        for below, slots in ((1000, None), (2048, [3, 7, 40]), (None, list(range(0, W, 2))), (None, None)):
            g.load(st)
            o.load(st)
            x, y = g.reclaim(below, slots), o.reclaim(below, slots)
            assert x["n"] == y["n"] > 0
            np.testing.assert_array_equal(x["seq"], y["seq"])
            np.testing.assert_array_equal(x["slot"], y["slot"])
            _same(g.read_state(), o.read_state(), "world 1, below %s" % below, keys=("reg", "queue", "log"))
    finally:
        g.close()
        o.close()


# ------------------------------------------------------------------ 3. ticked states against the twin
def _scenario(seed, W):
    scen = synth.random_scenario(seed, W=W, n_ticks=5, max_events=40, max_new=80)
    st = dict(reg=scen["init_reg"], free=scen["init_free"], hb=scen["init_hb"], epoch=scen["init_epoch"],
              queue=scen["init_queue"], log=scen["init_log"])
    return scen, st


def _resolve(tk, log):
    seq = np.full(len(tk["ev_kind"]), -1, np.int64)
    for i in np.nonzero(tk["ev_kind"] == synth.EV_RESULT)[0]:
        mine = np.nonzero(log == tk["ev_slot"][i])[0]
        if len(mine) and tk["ev_pick"][i] % 5 != 4:
            seq[i] = mine[tk["ev_pick"][i] % len(mine)]
    return seq


def _tick_both(g, o, args, t):
    a, b = g.tick(*args), o.tick(*args)
    for k in ("reconnect", "assign", "orphans", "evicted"):
        np.testing.assert_array_equal(a[k], b[k], err_msg="tick %s: %s" % (t, k))
    for k in ("n_assigned", "log_head", "queue_len"):
        assert a["result"][k] == b["result"][k], (t, k)
    sg, so = g.read_state(), o.read_state()
    _same(sg, so, "after tick %s" % t, keys=("reg", "queue", "log"))
    reg = so["reg"].astype(bool)
    for k in ("free", "hb", "epoch"):
        np.testing.assert_array_equal(sg[k][reg], so[k][reg], err_msg="after tick %s: %s" % (t, k))
    return a, b


TTE = 10.0


def ticked_state(rng, W=300, n_log=500):
    """Every slot registered at clock 1000 and queued, n_log live entries in flight."""
    return dict(reg=np.ones(W, np.uint8), free=rng.integers(1, 5, W).astype(np.int32), hb=np.full(W, 1000.0),
                epoch=np.zeros(W, np.uint32), queue=rng.permutation(W).astype(np.int32),
                log=rng.integers(0, W, n_log).astype(np.int32))


def ticked_events(rng, log, reg, now, silent, n_results, leaver=None):
    """A tick's messages: a heartbeat from every registered worker but the silent ones, a
    result for n_results live entries of workers that are not silent, a goodbye."""
    if leaver is not None:  # (its goodbye is its only message: a later one would meet an unknown identity)
        silent = np.append(silent, leaver)
    alive = np.flatnonzero(reg)
    beats = alive[~np.isin(alive, silent)]
    live = np.flatnonzero((log >= 0) & ~np.isin(log, silent))
    named = np.sort(rng.choice(live, min(n_results, len(live)), replace=False))
    kind = np.concatenate([np.full(len(beats), synth.EV_HEARTBEAT), np.full(len(named), synth.EV_RESULT)])
    slot = np.concatenate([beats, log[named]])
    seq = np.concatenate([np.full(len(beats), -1), named])
    if leaver is not None:
        kind, slot, seq = np.append(kind, _lib.FB_EV_LEAVE), np.append(slot, leaver), np.append(seq, -1)
    order = rng.permutation(len(kind))
    return (kind[order].astype(np.uint8), slot[order].astype(np.int32), np.zeros(len(kind), np.int32),
            np.full(len(kind), float(now)), seq[order].astype(np.int64))


def run_ticked(tick_both, reclaim_both, read, seed):
    """The scenario of test_ticked_states_against_the_one_gpu_twin over two callables:
    tick_both(args, t) -> the tick's outputs, reclaim_both(below, slots) -> dict(seq, slot),
    read() -> the state.  Four ticks (results in each; ten silent workers expire in the third,
    which also carries a goodbye), two reclaims, a late result, a reclaimed-from worker's death."""
    rng = np.random.default_rng(seed)
    st = read()
    doomed = np.unique(st["log"])[:10]
    carried, n_orph, n_res = 0, 0, 0
    for t, (now, n_new, n_results) in enumerate(((1001.0, 200, 40), (1007.0, 100, 30), (1013.0, 50, 30), (1019.0, 50, 30))):
        st = read()
        leaver = None
        if t == 2:  # a goodbye from a worker with entries in flight that is not about to expire
            owners = np.unique(st["log"][st["log"] >= 0])
            leaver = int(owners[~np.isin(owners, doomed)][7])
        k, s, v, ts, q = ticked_events(rng, st["log"], st["reg"], now, doomed, n_results, leaver)
        n = carried + n_new
        out = tick_both((now, TTE, k, s, v, ts, q, n), t)
        carried = n + len(out["orphans"]) - len(out["assign"])
        n_orph += len(out["orphans"])
        n_res += int((q >= 0).sum())
        if t == 2:
            assert set(doomed.tolist()) | {leaver} <= set(out["evicted"].tolist())
    assert n_orph > 10 and n_res == 130
    # the reclaims: a prefix, then three workers' entries
    pre = read()
    live = np.flatnonzero(pre["log"] >= 0)
    assert len(live) > 200
    below = int(live[len(live) // 3])
    x = reclaim_both(below, None)
    want, seq_m, slot_m, _ = reclaim_model(pre, below, None)
    np.testing.assert_array_equal(x["seq"], seq_m)
    np.testing.assert_array_equal(x["slot"], slot_m)
    left = np.flatnonzero(want["log"] >= 0)
    owners = [int(w) for w in np.unique(want["log"][left])[:3]]
    x2 = reclaim_both(None, owners)
    assert len(x["seq"]) > 60 and len(x2["seq"]) >= 3
    assert not np.isin(read()["log"], owners).any()
    # a late result names a reclaimed sequence: an ordinary result that completes nothing
    late, late_slot = int(x2["seq"][0]), int(x2["slot"][0])
    victim = next(w for w in owners if w != late_slot)
    st = read()
    free0 = int(st["free"][late_slot])
    k, s, v, ts, q = ticked_events(rng, st["log"], st["reg"], 1025.0, [victim], 0)
    k, s, v, ts, q = (np.append(k, synth.EV_RESULT).astype(np.uint8), np.append(s, late_slot).astype(np.int32),
                      np.append(v, 0).astype(np.int32), np.append(ts, 1025.0), np.append(q, late))
    out = tick_both((1025.0, TTE, k, s, v, ts, q, 0), "late result")
    st = read()
    assert st["log"][late] == -1 and len(out["assign"]) == 0 and int(st["free"][late_slot]) == free0 + 1
    # the victim, silent since 1019, expires: nothing of what was taken from it is an orphan
    taken = set(x["seq"].tolist()) | set(x2["seq"].tolist())
    died = []
    for step, now in enumerate((1028.0, 1031.0)):
        st = read()
        k, s, v, ts, q = ticked_events(rng, st["log"], st["reg"], now, [victim], 10)
        out = tick_both((now, TTE, k, s, v, ts, q, 20), "death %d" % step)
        died += out["evicted"].tolist()
        assert not taken & set(out["orphans"].tolist())
    assert died == [victim]


@pytest.mark.parametrize("xplan", (0, 1))
@pytest.mark.parametrize("world", (2, 3))
def test_ticked_states_against_the_one_gpu_twin(world, xplan):
    """Ticks with results, deaths and a leave, the group against a one-GPU twin after every
    step; a reclaim on both; then a result that names a reclaimed sequence completes nothing,
    a reclaimed-from worker that dies does not list the reclaimed entries among its orphans,
    and the ticks after the reclaim are the twin's (the pipeline's launches and reruns:
    test_reclaim_leaves_the_tick_pipeline_alone)."""
    W = 300
    st = ticked_state(np.random.default_rng(9400), W)
    g = LocalShardGroup(world, W, 8192, max_events=1024)
    o = GpuBalancer(W, 8192, max_events=1024)
    try:
        g.load(st)
        o.load(st)
        for b in g.bals:
            b.set_path("xplan", xplan)

        def reclaim_both(below, slots):
            x, y = g.reclaim(below, slots), o.reclaim(below, slots)
            assert x["n"] == y["n"] == len(x["seq"])
            np.testing.assert_array_equal(x["seq"], y["seq"])
            np.testing.assert_array_equal(x["slot"], y["slot"])
            _same(g.read_state(), o.read_state(), "after a reclaim", keys=("reg", "queue", "log"))
            return x

        run_ticked(lambda args, t: _tick_both(g, o, args, t)[0], reclaim_both, g.read_state, 9401)
    finally:
        g.close()
        o.close()


def _launches(grp):
    return [{k: v[1] for k, v in b.timing_read(64).items()} for b in grp.bals]


def test_reclaim_leaves_the_tick_pipeline_alone():
    """Two groups tick alike; one reclaims between the ticks.  No worker dies afterwards, so
    the log's content decides nothing: the ticks' outputs, result records (reruns, fill level,
    max_free: the round hint at work) and kernel launches are the same on every rank, and the
    reclaiming group launched lr_flag / lc_scan / lr_take besides."""
    W, world = 300, 3
    scen, st = _scenario(9500, W)
    tte = 1.0e6  # nobody expires
    A, B = (LocalShardGroup(world, W, len(st["log"]) + 8192, max_events=256) for _ in range(2))
    try:
        for g in (A, B):
            g.load(st)
            for b in g.bals:
                b.timing_enable(True)
        carried, n_taken = 0, 0
        for t, tk in enumerate(scen["ticks"]):
            seq = _resolve(tk, B.read_state()["log"])  # (B's log: entries A reclaimed are named too)
            if t >= 1:
                live = np.flatnonzero(A.read_state()["log"] >= 0)
                n_taken += A.reclaim(int(live[len(live) // 2]) if len(live) else 0, None if t % 2 else list(range(0, W, 3)))["n"]
            n = carried + tk["n_new"]
            args = (tk["now"], tte, tk["ev_kind"], tk["ev_slot"], tk["ev_val"], tk["ev_ts"], seq, n)
            a, b = A.tick(*args), B.tick(*args)
            for k in ("reconnect", "assign", "orphans", "evicted"):
                np.testing.assert_array_equal(a[k], b[k], err_msg="tick %d: %s" % (t, k))
            assert a["result"] == b["result"], (t, a["result"], b["result"])
            carried = n + len(b["orphans"]) - len(b["assign"])
        assert n_taken > 20
        sa, sb = A.read_state(), B.read_state()
        _same(sa, sb, "final", keys=("reg", "free", "hb", "epoch", "queue", "head"))
        assert ((sa["log"] == sb["log"]) | (sa["log"] == -1)).all() and (sa["log"] != sb["log"]).any()
        for r, (x, y) in enumerate(zip(_launches(A), _launches(B))):
            assert x.get("lr_flag", 0) > 0 and "lr_flag" not in y, (r, x, y)
            assert {k for k in x if k not in y} <= {"lr_flag", "lc_scan", "lr_take"}, (r, sorted(x), sorted(y))
            assert {k: v for k, v in x.items() if k not in ("lr_flag", "lc_scan", "lr_take")} == \
                {k: v for k, v in y.items() if k != "lc_scan"}, (r, x, y)
    finally:
        A.close()
        B.close()


# ------------------------------------------------------------------ 4. refusals change nothing
def _sum_exchange(bals):
    import torch
    torch.cuda.synchronize()
    total = bals[0].exchange().clone()
    for b in bals[1:]:
        total += b.exchange()
    for b in bals:
        b.exchange().copy_(total)
    torch.cuda.synchronize()


def test_refusals_change_nothing():
    W, world = 37, 2
    scen, st = _scenario(9600, W)
    tte = scen["tte"]
    g, twin = (LocalShardGroup(world, W, len(st["log"]) + 4096, max_events=256) for _ in range(2))
    try:
        g.load(st)
        twin.load(st)
        tk = scen["ticks"][0]
        args = (tk["now"], tte, tk["ev_kind"], tk["ev_slot"], tk["ev_val"], tk["ev_ts"], _resolve(tk, g.read_state()["log"]), 30)
        b0, b1 = g.bals
        before = _rank_states(g)
        # below_seq < 0, through the group
        _raises(FB_EINVAL, g.reclaim, -1, needle="below_seq")
        _unchanged(g, before, "below_seq < 0")
        # staged events
        for b in g.bals:
            b.stage(tk["now"])
        _raises(FB_ESTATE, b0.reclaim_part, needle="fb_log_reclaim_shard with staged events")
        _raises(FB_ESTATE, g.reclaim, 50, needle="staged events")
        _unchanged(g, before, "staged events")
        # phase 1 enqueued; phase 2 enqueued and not waited for
        for b in g.bals:
            b.launch(*args)
        for b in g.bals:
            _raises(FB_ESTATE, b.reclaim_part, needle="fb_log_reclaim_shard with a tick launched")
        _raises(FB_ESTATE, g.reclaim, needle="tick launched")
        for b in g.bals:
            n = C.c_int64()
            b._chk(b.lib.fb_exchange_bytes(b.h, b._E, C.byref(n)))
            b._xbytes = n.value
        _sum_exchange(g.bals)
        for b in g.bals:
            b.cont()
        _raises(FB_ESTATE, b1.reclaim_part, 50, needle="tick launched")
        _raises(FB_ESTATE, g.reclaim, 50, needle="tick launched")
        # waited, and committed on rank 0 only: the group raises FB_ESTATE and no rank took anything
        for b in g.bals:
            b.wait()
        _raises(FB_ESTATE, b0.reclaim_part, needle="wait and its commit")
        b0.commit()
        r0 = b0.read_state()
        assert b0.reclaim_part(count_only=True)["n"] > 0  # (rank 0 alone could)
        _raises(FB_ESTATE, g.reclaim, needle="wait and its commit")
        _same(b0.read_state(), r0, "rank 0, the other rank not committed")
        b1.commit()
        twin.tick(*args)
        before = _rank_states(g)
        for r, (x, y) in enumerate(zip(before, _rank_states(twin))):
            _same(x, y, "rank %d against the twin that was never asked" % r)
            np.testing.assert_array_equal(x["log_seq"], y["log_seq"])
        # between a compaction's mark and its cancel
        for b in g.bals:
            b.compact_mark()
        _raises(FB_ESTATE, b0.reclaim_part, needle=MARKED)
        _raises(FB_ESTATE, g.reclaim, needle=MARKED)
        for b in g.bals:
            b.compact_cancel()
        _unchanged(g, before, "marked, cancelled")
        # slots outside the table
        with pytest.raises(ValueError):
            g.reclaim(slots=[W])
        _unchanged(g, before, "slots outside the table")
        # ... and the group reclaims
        assert check_group_reclaim(g, lambda: _rank_states(g), world, None, None, "after the refusals")["n"] > 0
    finally:
        g.close()
        twin.close()


def test_reclaim_takes_back_a_dropped_launchs_clears():
    """A sharded tick's results clear their log entries at launch.  Its wait fails the length
    check on every rank (fault_qlen): the launch is dropped, and the reclaim owes the undo
    before it counts -- the entries the dropped launch's results named are reclaimed as live."""
    W, world = 41, 2
    rng = np.random.default_rng(9700)
    st = seam_state(rng, W, world, [2049, 900])
    st["reg"][:] = 1
    st["epoch"][:] = 0
    st["hb"][:] = 1000.0
    g = LocalShardGroup(world, W, CAP, max_events=1024)
    try:
        g.load(st)
        pre = g.read_state()
        before = _rank_states(g)
        live = np.flatnonzero(pre["log"] >= 0)
        assert len(live) == 2949
        named = np.sort(rng.choice(live, 300, replace=False))
        k = np.full(len(named), synth.EV_RESULT, np.uint8)
        args = (1000.5, 100.0, k, pre["log"][named], np.zeros(len(k), np.int32), np.full(len(k), 1000.5), named, 20)
        for b in g.bals:
            b.timing_enable(True)
            b.set_path("fault_qlen", 1 << 30)
            b.launch(*args)
        for b in g.bals:
            n = C.c_int64()
            b._chk(b.lib.fb_exchange_bytes(b.h, b._E, C.byref(n)))
            b._xbytes = n.value
        _sum_exchange(g.bals)
        for b in g.bals:
            b.cont()
        for b in g.bals:
            with pytest.raises(FaasbalError, match="queue length"):
                b.wait()
        for b in g.bals:
            assert "log_undo" not in b.timing_read(64)
        want, seq, slot, _ = reclaim_model(pre, None, None)
        out = g.reclaim()
        for b in g.bals:
            assert b.timing_read(64)["log_undo"][1] == 1  # (owed once: the count step paid it)
        assert out["n"] == len(live)
        np.testing.assert_array_equal(out["seq"], seq)
        np.testing.assert_array_equal(out["slot"], slot)
        assert np.isin(named, out["seq"]).all()
        post = g.read_state()
        assert (post["log"] == -1).all() and post["head"] == pre["head"]
        for x, y in zip(_rank_states(g), before):
            _same(x, y, "records", keys=("reg", "free", "hb", "epoch", "queue", "head"))
    finally:
        g.close()


# ------------------------------------------------------------------ 5. the drop-in on a group
@pytest.mark.parametrize("world", (2, 3))
def test_dispatcher_deadlines_over_a_local_shard_group(world):
    """GpuPushDispatcher over a LocalShardGroup with task_timeout and max_attempts: the scripted
    deadline and restart scenarios send what the one-GPU dispatcher sends."""
    from faasbal.dispatcher import GpuPushDispatcher
    groups = []

    def over_group(*a, **kw):
        grp = LocalShardGroup(world, kw["max_workers"], kw["max_inflight"], max_events=kw["max_events"])
        groups.append(grp)
        return GpuPushDispatcher(*a, balancer=grp, **kw)
    one, d1 = _scripted(GpuPushDispatcher)
    grp, dn = _scripted(over_group)
    try:
        assert grp == one and len(one) > 12
        assert [d.reclaimed for d in dn] == [d.reclaimed for d in d1] == [1, 2, 2]
        for a, b in zip(d1, dn):
            la, lb = a.balancer.read_state()["log"], b.balancer.read_state()["log"]
            np.testing.assert_array_equal(la, lb)
            assert b.head == len(lb) and all(lb[q] == s for q, (_, s) in b.inflight.items())
    finally:
        for d in d1:
            d.balancer.close()
        for grp in groups:
            grp.close()


# ------------------------------------------------------------------ 6. across processes
def _dist_main(rank, port, errq):
    """Two processes on one GPU over gloo, library contexts on both: the call and the slots
    travel as tensors, the ranks' headers through all_gather, the lists in one gather."""
    from test_gpu_shard_dist import _setup
    dist = _setup(rank, port)
    from faasbal.sharded import DistShardGroup, ShardedBalancer, serve_shard
    try:
        W = 300
        rng = np.random.default_rng(9800)
        st = seam_state(rng, W, 2, [2049, 4 * 2048 + 1])
        bal = ShardedBalancer(rank, 2, W, CAP, max_events=256, device=0)
        if rank != 0:
            # before this rank's third count step it stages events: that reclaim is refused here
            part, counts = bal.reclaim_part, [0]

            def counted(below_seq=None, slots=None, count_only=False):
                if count_only:
                    counts[0] += 1
                    if counts[0] == 3:
                        bal.stage(2000.0)
                return part(below_seq, slots, count_only)
            bal.reclaim_part = counted
            serve_shard(bal)  # (it keeps serving after the refused reclaim)
            assert counts[0] == 5
            bal.read_state()
            return
        g = DistShardGroup(bal, W)
        assert callable(g.reclaim)
        g.load(st)
        shards = lambda: g._each("read", with_log=True)  # noqa: E731 -- every rank's shard, through the group
        head = len(st["log"])
        assert check_group_reclaim(g, shards, 2, head // 3, None, "gloo, a bound")["n"] > 100
        assert check_group_reclaim(g, shards, 2, None, list(range(0, W, 2)), "gloo, a mask")["n"] > 100
        # rank 1 refuses in the count step: rank 0 raises its code, every shard is as it was
        before = g.read_state()
        with pytest.raises(FaasbalError) as e:
            g.reclaim(head - 100)
        assert e.value.code == FB_ESTATE and "staged events" in str(e.value), e.value
        _same(g.read_state(), before, "a rank refused")
        # the group goes on: a tick takes the staged batch, then the reclaim works
        g.tick(2000.0, 1.0e6, n_pending=7)
        assert check_group_reclaim(g, shards, 2, head - 100, None, "gloo, after a refusal")["n"] > 100
        assert check_group_reclaim(g, shards, 2, head - 100, None, "gloo, nothing left below")["n"] == 0
        g.close()
    except Exception as e:  # report to the parent, keep the peer from hanging
        errq.put("rank %d: %r" % (rank, e))
        raise
    finally:
        dist.destroy_process_group()


def test_dist_group_reclaims_over_gloo_on_one_gpu():
    from test_gpu_shard_dist import _spawn
    _spawn(_dist_main, ())
