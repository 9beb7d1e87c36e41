"""fb_log_reclaim on the GPU: live log entries taken back from workers that stay registered.

Against the numpy model of the rule (tests/reclaim_model.py) over read_state()'s arrays, and
-- ticking on after reclaims -- against the oracle, in which a reclaim is export / edit / load
(the statement of include/faasbal.h: the state afterwards is the one fb_load_state installs
from fb_read_state's arrays with the reclaimed entries set to -1).  Nothing here compares the
library with itself.
"""
import ctypes as C

import numpy as np
import pytest

from faasbal import FaasbalError, GpuBalancer, _lib, synth
from fill_cases import water_fill
from lc_model import compact_model
from oracle import Oracle
from reclaim_model import inflight_model, live_entries, reclaim_model, slots_mask
from test_gpu_log_compact import _pattern, _resolve_own, _shape_state, _state_of

pytestmark = pytest.mark.gpu

STATE_KEYS = ("reg", "free", "hb", "epoch", "queue", "log")


def _same_state(a, b, what, keys=STATE_KEYS):
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg="%s: %s" % (what, k))
    assert a["head"] == len(b["log"]), what


def _raw(g, below, mask, want_seq, want_slot, cap):
    """fb_log_reclaim through ctypes: (rc, count, seq, slot); the arrays pre-filled with -7."""
    seq = np.full(max(cap, 1), -7, np.int64)
    slot = np.full(max(cap, 1), -7, np.int32)
    n = C.c_int64(-7)
    rc = g.lib.fb_log_reclaim(g.h, int(below), None if mask is None else mask.ctypes.data_as(C.c_void_p),
                              seq.ctypes.data_as(C.c_void_p) if want_seq else None,
                              slot.ctypes.data_as(C.c_void_p) if want_slot else None, int(cap), C.byref(n))
    return rc, n.value, seq, slot


# ------------------------------------------------------------------ 1. shapes vs the model
HEADS = (0, 1, 63, 64, 65, 2047, 2048, 2049, 3 * 2048 + 5)
BELOWS = (0, 1, 63, 64, 65, 2047, 2048, 2049)
PATTERNS = ("all", "none", "alternating", "random30", "first", "last")
W_SHAPES = 300


@pytest.mark.parametrize("head", HEADS)
def test_shapes_against_the_model(head):
    rng = np.random.default_rng(1000 + head)
    g = GpuBalancer(W_SHAPES, 3 * 2048 + 64, max_events=64)
    belows = sorted({b for b in BELOWS + (head, head + 7) if b <= head + 7})
    taken = 0
    for name in PATTERNS:
        st = _shape_state(head, _pattern(name, head, rng), rng)
        g.load(st)
        before, infl = g.read_state(), g.inflight()
        np.testing.assert_array_equal(infl, inflight_model(before), err_msg="loaded counts")
        owners = np.unique(before["log"][live_entries(before)])
        masks = {"none": None, "zero": [], "one": [int(owners[len(owners) // 2])] if len(owners) else [0],
                 "half": np.flatnonzero(rng.random(W_SHAPES) < 0.5).tolist()}
        first = True
        for below in belows:
            for mname, slots in masks.items():
                what = "head %d %s below %d mask %s" % (head, name, below, mname)
                if not first:
                    g.load(st)
                first = False
                mask = None if slots is None else slots_mask(W_SHAPES, slots)
                want, seq, slot, drop = reclaim_model(before, below, mask)
                out = g.reclaim(below, slots)
                assert out["n"] == len(seq), what
                np.testing.assert_array_equal(out["seq"], seq, err_msg=what + ": seq")
                np.testing.assert_array_equal(out["slot"], slot, err_msg=what + ": slot")
                _same_state(g.read_state(), want, what)
                np.testing.assert_array_equal(g.inflight(), infl - drop, err_msg=what + ": inflight")
                taken += len(seq)
        # the raw call: below_seq far past the head, no outputs, one output, and too little room
        want, seq, slot, drop = reclaim_model(before, None, None)
        n = len(seq)
        what = "head %d %s raw" % (head, name)
        if n:
            g.load(st)
            rc, cnt, sq, sl = _raw(g, 1 << 40, None, True, True, n - 1)
            assert (rc, cnt) == (_lib.FB_EINVAL, n), what  # the count to come back with
            assert (sq == -7).all() and (sl == -7).all(), what
            _same_state(g.read_state(), before, what + ": cap n - 1 changes nothing")
            np.testing.assert_array_equal(g.inflight(), infl, err_msg=what)
            rc, cnt, sq, sl = _raw(g, 1 << 40, None, False, True, n - 1)
            assert (rc, cnt) == (_lib.FB_EINVAL, n) and (sl == -7).all(), what
            _same_state(g.read_state(), before, what + ": cap n - 1, one output")
        g.load(st)
        rc, cnt, sq, sl = _raw(g, head, None, False, False, 0)  # no outputs: cap is not looked at
        assert (rc, cnt) == (0, n) and (sq == -7).all() and (sl == -7).all(), what
        _same_state(g.read_state(), want, what + ": NULL outputs")
        np.testing.assert_array_equal(g.inflight(), infl - drop, err_msg=what + ": NULL outputs")
        g.load(st)
        rc, cnt, sq, sl = _raw(g, head + 7, np.full(W_SHAPES, 255, np.uint8), True, False, n)
        assert (rc, cnt) == (0, n) and (sl == -7).all(), what
        np.testing.assert_array_equal(sq[:n], seq, err_msg=what + ": seq alone")
        _same_state(g.read_state(), want, what + ": seq alone")
        assert _raw(g, -1, None, False, False, 0)[0] == _lib.FB_EINVAL
        assert _raw(g, 0, None, True, True, -1)[0] == _lib.FB_EINVAL
        _same_state(g.read_state(), want, what + ": refused arguments")
    assert taken > 0 or head == 0
    g.close()


# ------------------------------------------------------------------ 2. budget extremes
@pytest.mark.parametrize("shape", ["one_slot", "all_different"])
def test_budget_extremes(shape):
    """Every entry of a tile (and one more) on one slot; every entry on a slot of its own: the
    per-slot counts afterwards are the model's."""
    if shape == "one_slot":
        W, log = 8, np.zeros(2049, np.int32)
    else:
        W = 2048
        log = np.random.default_rng(2).permutation(W).astype(np.int32)
    st = dict(reg=np.ones(W, np.uint8), free=np.full(W, 3, np.int32), hb=np.full(W, 1000.0),
              epoch=np.zeros(W, np.uint32), queue=np.arange(W, dtype=np.int32), log=log)
    g = GpuBalancer(W, 4096, max_events=16)
    for below, slots in ((None, None), (1000, None), (2048, None), (None, [0, 5])):
        g.load(st)
        before = g.read_state()
        infl = g.inflight()
        np.testing.assert_array_equal(infl, inflight_model(before))
        want, seq, slot, drop = reclaim_model(before, below, None if slots is None else slots_mask(W, slots))
        out = g.reclaim(below, slots)
        what = "%s below %s slots %s" % (shape, below, slots)
        np.testing.assert_array_equal(out["seq"], seq, err_msg=what)
        np.testing.assert_array_equal(out["slot"], slot, err_msg=what)
        np.testing.assert_array_equal(g.inflight(), inflight_model(want), err_msg=what + ": counts")
        np.testing.assert_array_equal(g.inflight(), infl - drop, err_msg=what + ": counts")
        _same_state(g.read_state(), want, what)
        assert len(seq) > 0, what
    g.close()


# ------------------------------------------------------------------ helpers: ticks vs the oracle
def _load_pair(st, W, cap, max_events=64, setup=None, purge_mode=1):
    g = GpuBalancer(W, cap, max_events=max_events)
    if setup is not None:
        setup(g)
    g.load(st)
    o = Oracle(W, cap, purge_mode=purge_mode)
    o.load(st["reg"], st["free"], st["hb"], st["epoch"], st["queue"], st["log"])
    return g, o


def _oracle_level(so, tk, tte, seq, n):
    """The fill level the reference loop reaches on this tick: a second oracle applies the
    messages and the purge without dispatching, and the ten-line water fill
    (tests/fill_cases.py) runs over the queue it leaves."""
    o2 = Oracle(len(so["reg"]), len(so["log"]) + 8)
    o2.load(so["reg"], so["free"], so["hb"], so["epoch"], so["queue"], so["log"])
    b = o2.tick(tk["now"], tte, tk["ev_kind"], tk["ev_slot"], tk["ev_val"], tk["ev_ts"], seq, n, dispatch_limit=0)
    s2 = o2.export()
    return water_fill(np.maximum(s2["free"][s2["queue"]], 1), n + len(b["orphans"]))[0]


def _tick_pair(g, o, tk, tte, n, t, seq=None):
    so = o.export()
    if seq is None:
        seq = _resolve_own(so["log"], tk)
    level = _oracle_level(so, tk, tte, seq, n)
    a = g.tick(tk["now"], tte, tk["ev_kind"], tk["ev_slot"], tk["ev_val"], tk["ev_ts"], seq, n)
    b = o.tick(tk["now"], tte, tk["ev_kind"], tk["ev_slot"], tk["ev_val"], tk["ev_ts"], seq, n)
    for k in ("reconnect", "assign", "orphans", "evicted"):
        np.testing.assert_array_equal(a[k], b[k], err_msg="tick %d: %s" % (t, k))
    r, s1 = a["result"], o.export()
    got = (r["n_assigned"], r["n_orphans"], r["n_evicted"], r["log_head"], r["queue_len"], r["fill_level"])
    want = (len(b["assign"]), len(b["orphans"]), len(b["evicted"]), s1["head"], len(s1["queue"]), level)
    assert got == want, "tick %d: result record %s, the oracle's %s" % (t, got, want)
    return b


def _reclaim_pair(g, o, below, slots, what):
    """A reclaim on the GPU (no state read before it) and, in the oracle, export / edit / load."""
    so = o.export()
    mask = None if slots is None else slots_mask(len(so["reg"]), slots)
    new, seq, slot, _ = reclaim_model(so, below, mask)
    out = g.reclaim(below, slots)
    np.testing.assert_array_equal(out["seq"], seq, err_msg=what + ": seq")
    np.testing.assert_array_equal(out["slot"], slot, err_msg=what + ": slot")
    assert out["n"] == len(seq), what
    o.load(new["reg"], new["free"], new["hb"], new["epoch"], new["queue"], new["log"])
    return out


def _final(g, o, counts=True):
    sg, so = g.read_state(), o.export()
    np.testing.assert_array_equal(sg["reg"], so["reg"], err_msg="final reg")
    reg = so["reg"].astype(bool)
    np.testing.assert_array_equal(sg["free"][reg], so["free"][reg], err_msg="final free")
    np.testing.assert_array_equal(sg["hb"][reg], so["hb"][reg], err_msg="final hb")
    np.testing.assert_array_equal(sg["epoch"][reg], so["epoch"][reg], err_msg="final epoch")
    np.testing.assert_array_equal(sg["queue"], so["queue"], err_msg="final queue")
    np.testing.assert_array_equal(sg["log"], so["log"], err_msg="final log")
    if counts:
        np.testing.assert_array_equal(g.inflight(), inflight_model(so), err_msg="final in-flight counts")


def _ev(kind, slot, val, ts, seq=None):
    return dict(ev_kind=np.asarray(kind, np.uint8), ev_slot=np.asarray(slot, np.int32),
                ev_val=np.asarray(val, np.int32), ev_ts=np.asarray(ts, np.float64),
                ev_seq=np.full(len(kind), -1, np.int64) if seq is None else np.asarray(seq, np.int64))


# ------------------------------------------------------------------ 3. ticks on, vs the oracle
@pytest.mark.parametrize("lazy", [1, 0])
@pytest.mark.parametrize("plan", [0, 1, 2])
def test_scripted_ticks_against_the_oracle(plan, lazy):
    """Six ticks, four reclaims between them, each right after a committed tick with no state
    read in between (the deferred commit is the gate's to flush):
      A  slots {3, 5} below 4: slot 3 keeps one older entry and the task tick 0 gave it, and
         dies in tick 1 -- its orphans are exactly those two, the fill level the oracle's (the
         budget seam); slot 5's result in tick 1 names its reclaimed sequence: an ordinary result;
      B  below = head right after tick 1, which evicted slot 3 with tasks in flight: the
         entries that tick redistributed are still in the log (lazy commits) and are not live;
      C  a prefix, before slot 1 falls silent; it dies in tick 4 with reclaimed and kept entries;
      D  a result in tick 3 names one of C's sequences."""
    W = 8
    st = dict(reg=np.ones(W, np.uint8), free=np.asarray([2, 6, 2, 2, 2, 2, 2, 2], np.int32), hb=np.full(W, 1000.0),
              epoch=np.zeros(W, np.uint32), queue=np.arange(W, dtype=np.int32),
              log=np.asarray([3, -1, 3, 5, -1, 3, 1, -1], np.int32))

    def setup(g):
        g.set_path("plan", plan)
        g.set_path("lazy", lazy)
    g, o = _load_pair(st, W, 512, setup=setup)

    def beat(now, who, extra=None):
        tk = _ev([synth.EV_HEARTBEAT] * len(who), who, [0] * len(who), [now] * len(who))
        if extra is not None:
            tk = {k: np.concatenate([tk[k], extra[k]]) for k in tk}
        return dict(tk, now=now)

    not3 = [s for s in range(W) if s != 3]
    not1 = [s for s in range(W) if s != 1]
    carried = 0

    def tick(t, tk, n_new):
        nonlocal carried
        n = carried + n_new
        b = _tick_pair(g, o, tk, 10.0, n, t, seq=tk["ev_seq"])
        carried = n + len(b["orphans"]) - len(b["assign"])
        return b

    b0 = tick(0, beat(1005.0, not3), 4)
    assert 3 in b0["assign"]  # slot 3 got a task of this tick
    a = _reclaim_pair(g, o, 4, [3, 5], "A")
    np.testing.assert_array_equal(a["seq"], [0, 2, 3])
    b1 = tick(1, beat(1011.0, not3, _ev([synth.EV_RESULT], [5], [0], [1011.0], [3])), 0)
    np.testing.assert_array_equal(b1["evicted"], [3])
    np.testing.assert_array_equal(b1["orphans"], [5, 8 + int(np.flatnonzero(b0["assign"] == 3)[0])])
    head = o.export()["head"]
    bb = _reclaim_pair(g, o, head, None, "B")
    assert bb["n"] > 0 and 3 not in bb["slot"] and not set(bb["seq"]) & {0, 2, 3, 5}
    tick(2, beat(1012.0, not3, _ev([synth.EV_REGISTER], [3], [3], [1012.0])), 14)
    head = o.export()["head"]
    c = _reclaim_pair(g, o, head - 4, None, "C")
    on1 = c["seq"][c["slot"] == 1]
    kept1 = np.flatnonzero(o.export()["log"] == 1)
    assert len(on1) and len(kept1), "slot 1 needs reclaimed and kept entries: %s / %s" % (on1, kept1)
    other = int(np.flatnonzero((c["slot"] != 1) & (c["slot"] != 3))[0])
    late = _ev([synth.EV_RESULT], [int(c["slot"][other])], [0], [1018.0], [int(c["seq"][other])])
    tick(3, beat(1018.0, not1, late), 0)
    b4 = tick(4, beat(1023.0, not1), 2)
    np.testing.assert_array_equal(b4["evicted"], [1])
    np.testing.assert_array_equal(b4["orphans"], kept1)
    tick(5, beat(1024.0, not1), 3)
    _final(g, o)
    g.close()


@pytest.mark.parametrize("seed", range(4))
def test_random_streams_against_the_oracle(seed):
    """synth streams with results and deaths; between ticks a reclaim of a random prefix and
    mask (every other one right after the commit, the rest after a state read)."""
    W = [48, 300][seed % 2]
    scen = synth.random_scenario(9100 + seed, W=W, n_ticks=6, max_events=[40, 200][seed % 2], max_new=[70, 300][seed % 2])
    st = _state_of(scen)
    g, o = _load_pair(st, W, len(st["log"]) + 8000, max_events=256, setup=lambda g: g.set_path("plan", seed % 3))
    rng = np.random.default_rng(seed)
    carried, taken = 0, 0
    for t, tk in enumerate(scen["ticks"]):
        n = carried + tk["n_new"]
        b = _tick_pair(g, o, tk, scen["tte"], n, t)
        carried = n + len(b["orphans"]) - len(b["assign"])
        if t % 2:
            g.read_state(with_log=bool(t % 4 == 1))
        head = o.export()["head"]
        below = [None, head, int(rng.integers(0, head + 1)), head + 3][int(rng.integers(0, 4))]
        slots = None if rng.random() < 0.4 else np.flatnonzero(rng.random(W) < 0.5).tolist()
        taken += _reclaim_pair(g, o, below, slots, "after tick %d" % t)["n"]
    assert taken > 0
    _final(g, o)
    g.close()


# ------------------------------------------------------------------ 4. the window survives
def test_window_pipeline_survives_a_reclaim():
    st = synth.zipf_state(W=300, seed=3, dead_frac=0.0)
    ticks = synth.stream_ticks(st, n_ticks=6, seed=11, tasks_per_tick=16, results_per_tick=16, dt=0.3,
                               hb_frac=0.01, join_frac=0.0)
    E = max(len(t["ev_kind"]) for t in ticks)
    g, o = _load_pair(st, 300, 3 * len(st["log"]) + 1024, max_events=max(E, 1), setup=lambda g: g.set_window(1),
                      purge_mode=2)
    carried = 0
    for t, tk in enumerate(ticks):
        n = carried + tk["n_new"]
        b = _tick_pair(g, o, tk, 10.0, n, t, seq=tk["ev_seq"])
        assert g.last["fill_level"] == 0, "tick %d" % t
        carried = n + len(b["orphans"]) - len(b["assign"])
        if t == 3:
            wt, fb = g.window_stats()
            assert wt >= 2, "window ticks before the reclaim: %d (fallbacks %d)" % (wt, fb)
            head = o.export()["head"]
            out = _reclaim_pair(g, o, head // 2, list(range(0, 300, 2)), "between window ticks")
            assert out["n"] > 0
            assert g.window_stats() == (wt, fb)
        if t == 4:
            assert g.window_stats() == (wt + 1, fb), "the tick after the reclaim left the window path"
    _final(g, o)
    g.close()


# ------------------------------------------------------------------ 5. the large kind
def test_large_context_in_place_clears_no_counts():
    W = (1 << 17) + 5
    rng = np.random.default_rng(5)
    workers = np.asarray([0, 1, 77, 4095, 65536, 1 << 17, W - 1], np.int32)
    reg = np.zeros(W, np.uint8)
    reg[workers] = 1
    free = np.zeros(W, np.int32)
    free[workers] = 4
    hb = np.zeros(W)
    hb[workers] = 1000.0
    log = workers[rng.integers(0, len(workers), 5000)].astype(np.int32)
    log[rng.random(5000) < 0.2] = -1
    st = dict(reg=reg, free=free, hb=hb, epoch=np.zeros(W, np.uint32), queue=workers.copy(), log=log)
    g, o = _load_pair(st, W, 8192, max_events=64)
    with pytest.raises(FaasbalError) as e:
        g.inflight()  # (this kind keeps no counts)
    assert e.value.code == _lib.FB_ESTATE
    g.timing_enable(True)
    g.timing_read()
    out = _reclaim_pair(g, o, 4100, [1, 4095, W - 1], "large")
    assert out["n"] > 100
    names = g.timing_read()
    assert {"lr_flag", "lc_scan", "lr_take"} <= set(names), names
    assert sum(cnt for _, cnt in names.values()) <= 5, names
    g.timing_enable(False)
    alive = [int(s) for s in workers if s != 77]
    for t, (now, n) in enumerate(((1005.0, 6), (1011.0, 3))):  # slot 77 expires in the second
        tk = dict(_ev([synth.EV_HEARTBEAT] * len(alive), alive, [0] * len(alive), [now] * len(alive)), now=now)
        b = _tick_pair(g, o, tk, 10.0, n, t, seq=tk["ev_seq"])
    np.testing.assert_array_equal(b["evicted"], [77])
    _final(g, o, counts=False)
    g.close()


# ------------------------------------------------------------------ 6. order on the device
def test_refused_out_of_order_and_on_other_kinds():
    scen = synth.random_scenario(8805, W=48, n_ticks=2, max_events=30, max_new=40)
    st = _state_of(scen)
    g, o = _load_pair(st, 48, len(st["log"]) + 4000)
    tk = scen["ticks"][0]
    seq = _resolve_own(o.export()["log"], tk)
    before, infl = g.read_state(), g.inflight()

    def refused(what):
        rc, cnt, sq, sl = _raw(g, 1 << 40, None, True, True, 1 << 16)
        assert rc == _lib.FB_ESTATE and cnt == -7 and (sq == -7).all() and (sl == -7).all(), what
        assert b"fb_log_reclaim" in g.lib.fb_last_error(g.h), what

    g.stage(tk["now"], tk["ev_kind"], tk["ev_slot"], tk["ev_val"], tk["ev_ts"], seq)
    refused("staged")
    _same_state(g.read_state(), before, "staged")
    g.launch_staged(scen["tte"], 30)
    refused("launched")
    g.wait()
    refused("waited")
    a = dict(reconnect=g.event_status(), assign=g.assignments(), orphans=g.orphans(), evicted=g.evicted())
    g.commit()
    b = o.tick(tk["now"], scen["tte"], tk["ev_kind"], tk["ev_slot"], tk["ev_val"], tk["ev_ts"], seq, 30)
    for k in ("reconnect", "assign", "orphans", "evicted"):  # the refusals left the tick alone
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    _reclaim_pair(g, o, None, None, "after the commit")
    _final(g, o)
    g.close()
    # a deque context has no liveness; a sharded context's sequences are global
    d = GpuBalancer(16, 64, max_events=16, mode="deque")
    d.load(dict(reg=np.ones(16, np.uint8), free=np.ones(16, np.int32), hb=np.zeros(16), epoch=None,
                queue=np.arange(16, dtype=np.int32), log=np.asarray([1, 2, 3], np.int32)))
    n = C.c_int64(-7)
    assert d.lib.fb_log_reclaim(d.h, 3, None, None, None, 0, C.byref(n)) == _lib.FB_ESTATE and n.value == -7
    assert b"deque" in d.lib.fb_last_error(d.h)
    np.testing.assert_array_equal(d.read_state()["log"], [1, 2, 3])
    d.close()
    from faasbal.sharded import ShardedBalancer
    assert ShardedBalancer.reclaim is None
    sb = ShardedBalancer(0, 1, 16, 64, max_events=16)
    assert sb.lib.fb_log_reclaim(sb.h, 3, None, None, None, 0, C.byref(n)) == _lib.FB_ESTATE and n.value == -7
    assert b"fb_log_compact_shard_mark" in sb.lib.fb_last_error(sb.h)
    sb.close()


# ------------------------------------------------------------------ 7. neighbours
def test_compaction_and_pool_summary_after_a_reclaim():
    rng = np.random.default_rng(7)
    head = 3 * 2048 + 5
    st = _shape_state(head, _pattern("random30", head, rng), rng)
    g = GpuBalancer(W_SHAPES, head + 64, max_events=64)
    g.load(st)
    before = g.read_state()
    live = int(live_entries(before).sum())
    s0 = g.pool_stats(1000.0, 1e9)
    assert s0["inflight"] == live and s0["inflight_max"] == int(inflight_model(before).max())
    slots = np.flatnonzero(rng.random(W_SHAPES) < 0.5).tolist()
    want, seq, slot, drop = reclaim_model(before, 5000, slots_mask(W_SHAPES, slots))
    out = g.reclaim(5000, slots)
    n = out["n"]
    assert n == len(seq) and 0 < n < live
    s1 = g.pool_stats(1000.0, 1e9)
    assert s1["inflight"] == live - n and s1["inflight_max"] == int(inflight_model(want).max())
    assert s1["log_head"] == head and s1["free_total"] == s0["free_total"] and s1["n_queued"] == s0["n_queued"]
    want2, kept = compact_model(want)
    got = g.compact_log(expect=live - n)
    np.testing.assert_array_equal(got["kept"], kept)
    after = g.read_state()
    for k in STATE_KEYS:
        np.testing.assert_array_equal(after[k], want2[k], err_msg=k)
    np.testing.assert_array_equal(g.inflight(), inflight_model(want2))
    g.close()
