"""fb_pool_stats on the GPU: the committed pool summarised on the device.

Against the numpy model of the rule (faasbal/poolstats.py) on the read_state() of a twin
balancer, against the tick itself (what it evicts, redistributes and places at the same
clock), and -- called before every tick of a scenario -- against a twin that never calls it:
the ticks' outputs, the final state, the window statistics and the launches stay the same.
"""
import ctypes as C
import glob
import os

import numpy as np
import pytest

from faasbal import FaasbalError, GpuBalancer, _lib, synth
from faasbal.poolstats import MAX_EDGES, diff_summary, pool_stats_model
from oracle import fixture_ticks

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
I32MAX = (1 << 31) - 1


def _check(got, st, now, tte, edges, what, **kw):
    want = pool_stats_model(st, now, tte, edges, **kw)
    d = diff_summary(got, want)
    assert not d, "%s: device vs model %r" % (what, d)
    return want


# ------------------------------------------------------------------ 1. shapes vs the model
WS = (0, 1, 255, 256, 257, 1023, 1025, 4100)
HEADS = (0, 1, 2047, 2048, 2049, 3 * 2048 + 5)
QS = (0, 1, 256, 257)
EDGES = ((), (10.0,), tuple(float(i) for i in range(1, 16)))
NOW, TTE = 1000.0, 10.0


def _shape_state(W, head, Q, rng):
    """As _shape_state of tests/test_gpu_log_compact.py for any W: the first two thirds of the
    slots registered -- half of those with epoch 0 (they own the live entries), a quarter with
    epochs anywhere in [0, head] (inside dead runs, on live entries), the rest with epoch ==
    head -- the last third without a record, epochs up to past the head.  Free counts -3 .. 39
    plus the edge values, heartbeats on quarter seconds up to 15.75 s old (on the age edges,
    on tte itself), one registered slot with a NaN heartbeat; Q queued slots, expired ones and
    ones without free processes among them."""
    nreg = min(W, max(1, 2 * W // 3))
    a = max(1, nreg // 2)
    b = max(a, 3 * nreg // 4)
    reg = (np.arange(W) < nreg).astype(np.uint8)
    epoch = np.zeros(W, np.uint32)
    epoch[a:b] = rng.integers(0, head + 1, b - a)
    epoch[b:nreg] = head
    epoch[nreg:] = rng.integers(0, head + 6, W - nreg)
    log = np.full(head, -1, np.int32)
    if W:
        live = rng.random(head) < 0.5
        live[head // 3: head // 2] = False  # a dead run
        idx = np.flatnonzero(live)
        s = rng.integers(0, b, len(idx))
        log[idx] = np.where(idx >= epoch[s].astype(np.int64), s, idx % a)
    free = np.where(reg, rng.integers(-3, 40, W), 0).astype(np.int32)
    edge = np.asarray([-3, 0, 31, 32, 33, I32MAX, I32MAX, I32MAX], np.int32)[:nreg]
    free[:len(edge)] = edge
    hb = np.where(reg, NOW - 0.25 * rng.integers(0, 64, W), 0.0)
    hb[:len(edge)] = NOW - 0.25 * np.arange(len(edge))  # (the edge values count: alive)
    if nreg > 4:
        hb[nreg - 1] = np.nan
    queue = rng.permutation(nreg).astype(np.int32)[:min(Q, nreg)]
    return dict(reg=reg, free=free, hb=hb, epoch=epoch, queue=queue, log=log)


@pytest.fixture(scope="module")
def pair():
    g, twin = (GpuBalancer(4100, 3 * 2048 + 64, max_events=64) for _ in range(2))
    yield g, twin
    g.close()
    twin.close()


@pytest.mark.parametrize("W", WS)
def test_shapes_against_the_model(W, pair):
    g, twin = pair
    rng = np.random.default_rng(W)
    for j, head in enumerate(HEADS):
        Q = QS[(j + WS.index(W)) % len(QS)]
        st = _shape_state(W, head, Q, rng)
        g.load(st)
        twin.load(st)
        ref = twin.read_state()
        for edges in EDGES:
            what = "W %d head %d Q %d edges %d" % (W, head, Q, len(edges))
            want = _check(g.pool_stats(NOW, TTE, edges), ref, NOW, TTE, edges, what)
            assert want["n_slots"] == W and want["log_head"] == head, what
            assert want["n_queued"] + want["n_queued_expired"] == min(Q, len(st["queue"])), what
        if W >= 255:  # the state has what the test is about
            assert 0 < want["n_expired"] < want["n_registered"] and want["free_total"] > 3 * I32MAX, what
            assert want["free_hist"][[0, 31, 32]].all() and (want["age_hist"] > 0).sum() == MAX_EDGES + 1, what
            if head > 64:
                assert want["inflight"] > 0 and want["inflight_expired"] > 0, what
        # a moved clock: everything expired, then nothing (tte huge)
        _check(g.pool_stats(NOW + 100.0, TTE, (1.0, 2.0)), ref, NOW + 100.0, TTE, (1.0, 2.0), "W %d late" % W)
        _check(g.pool_stats(NOW, 1e300), ref, NOW, 1e300, (), "W %d patient" % W)


# ------------------------------------------------------------------ 2. against the tick itself
SMALL = sorted(glob.glob(os.path.join(GOLDEN, "small_*.npz")))


@pytest.mark.parametrize("path", SMALL[:: max(1, len(SMALL) // 6)][:6], ids=lambda p: os.path.basename(p)[:-4])
def test_the_tick_does_what_the_summary_says(path):
    z = np.load(path)
    st = dict(reg=z["init_reg"], free=z["init_free"], hb=z["init_hb"], epoch=z["init_epoch"],
              queue=z["init_queue"], log=z["init_log"])
    now, tte = float(z["now"][0]), float(z["tte"])
    room = int(np.maximum(st["free"].astype(np.int64), 1).sum()) + len(st["log"]) + 64
    g = GpuBalancer(int(z["W"]), len(st["log"]) + room, max_events=16)
    g.load(st)
    s = g.pool_stats(now, tte)
    assert int(g.inflight().sum()) == s["inflight"] + s["inflight_expired"]
    g.launch(now, tte, n_pending=s["dispatchable"] + 7)
    r = g.wait()
    g.commit()
    assert r["n_evicted"] == s["n_expired"]
    assert r["n_orphans"] == s["inflight_expired"]
    assert r["n_assigned"] == s["dispatchable"]
    # ... and afterwards nobody is expired at that clock, the orphans are in flight again
    t = _check(g.pool_stats(now, tte), g.read_state(), now, tte, (), "after the tick")
    assert t["n_expired"] == t["inflight_expired"] == 0 and t["n_registered"] == s["n_registered"] - s["n_expired"]
    assert t["inflight"] == s["inflight"] + r["n_assigned"]
    g.close()


# ------------------------------------------------------------------ 3. the pipeline is untouched
def _twins(W, cap, E, setup):
    out = []
    for _ in range(3):
        g = GpuBalancer(W, cap, max_events=E)
        setup(g)
        out.append(g)
    return out


def _run_twins(st, ticks, tte, W, cap, E, setup=lambda g: None):
    """A summarises the pool before every tick and never reads the state; B does neither; C
    gives the state the summaries are held against.  Returns (A, B, A's summaries)."""
    A, B, Cc = _twins(W, cap, E, setup)
    A.timing_enable(True)
    for g in (A, B, Cc):
        g.load(st)
    edges = (tte / 4, tte / 2, tte)
    carried, seen = 0, []
    for t, tk in enumerate(ticks):
        s = A.pool_stats(tk["now"], tte, edges)
        _check(s, Cc.read_state(), tk["now"], tte, edges, "before tick %d" % t)
        seen.append(s)
        n = carried + tk["n_new"]
        outs = [g.tick(tk["now"], tte, tk["ev_kind"], tk["ev_slot"], tk["ev_val"], tk["ev_ts"], tk["ev_seq"], n)
                for g in (A, B, Cc)]
        for k in ("reconnect", "assign", "orphans", "evicted"):
            np.testing.assert_array_equal(outs[0][k], outs[1][k], err_msg="tick %d: %s" % (t, k))
        assert outs[0]["result"] == outs[1]["result"], "tick %d" % t
        carried = n + len(outs[1]["orphans"]) - len(outs[1]["assign"])
    s = A.pool_stats(ticks[-1]["now"], tte, edges)  # right behind the last commit
    _check(s, Cc.read_state(), ticks[-1]["now"], tte, edges, "after the last tick")
    seen.append(s)
    timing = A.timing_read(64)
    assert "settle" not in timing, sorted(timing)
    assert timing["ps_fold"][1] == len(seen) and "ps_slots" in timing and "ps_log" in timing, sorted(timing)
    assert A.window_stats() == B.window_stats()
    a, b = A.read_state(), B.read_state()
    for k in ("reg", "free", "hb", "epoch", "queue", "log"):
        np.testing.assert_array_equal(a[k], b[k], err_msg="final %s" % k)
    np.testing.assert_array_equal(A.inflight(), B.inflight())
    Cc.close()
    return A, B, seen


def test_summaries_between_ticks_leave_the_pipeline_alone():
    """Messages, expiries, orphans kept lazily in the log, deferred commits."""
    z = np.load(os.path.join(GOLDEN, "cfg5_w512_churn.npz"))
    st = dict(reg=z["init_reg"], free=z["init_free"], hb=z["init_hb"], epoch=z["init_epoch"],
              queue=z["init_queue"], log=z["init_log"])
    ticks = list(fixture_ticks(z))[:12]
    assert len(ticks) == 12
    W, E = int(z["W"]), max(len(t["ev_kind"]) for t in ticks)
    cap = len(st["log"]) + len(z["exp_assign"]) + 4096
    A, B, seen = _run_twins(st, ticks, float(z["tte"]), W, cap, max(E, 1))
    # the scenario has what the test is about: expired workers holding tasks before some tick,
    # and live entries counted while dead registrations' entries were still in the log
    assert sum(s["n_expired"] > 0 and s["inflight_expired"] > 0 for s in seen) >= 2
    assert any(s["log_head"] - s["inflight"] - s["inflight_expired"] > 0 for s in seen[1:])
    A.close()
    B.close()


def test_summaries_between_window_ticks_leave_the_window_alone():
    """Level-0 ticks under set_window(1): the window (offset, tombstones) is read in place."""
    st = synth.zipf_state(W=300, seed=3, dead_frac=0.0)
    ticks = synth.stream_ticks(st, n_ticks=12, seed=11, tasks_per_tick=16, results_per_tick=16, dt=0.3,
                               hb_frac=0.01, join_frac=0.0)
    E = max(len(t["ev_kind"]) for t in ticks)
    A, B, seen = _run_twins(st, ticks, 10.0, 300, 3 * len(st["log"]) + 4096, max(E, 1), setup=lambda g: g.set_window(1))
    wt, fb = A.window_stats()
    assert wt >= 6, "window ticks: %d (fallbacks %d)" % (wt, fb)
    A.close()
    B.close()


# ------------------------------------------------------------------ 4. deque contexts
def test_deque_context():
    scen = synth.random_deque_scenario(611, W=40, n_ticks=4, max_events=40, max_new=50, dup_frac=1.0)
    st = dict(reg=scen["init_reg"], free=scen["init_free"], hb=scen["init_hb"], epoch=scen["init_epoch"],
              queue=scen["init_queue"], log=scen["init_log"])
    g = GpuBalancer(40, len(st["log"]) + 4000, max_events=64, mode="deque")
    g.load(st)
    carried, repeats = 0, False
    for t, tk in enumerate(scen["ticks"] + [None]):
        ref = g.read_state()
        repeats = repeats or len(ref["queue"]) > len(set(ref["queue"].tolist()))
        # now, tte and the edges are ignored: NaN and a descending pair are as good as any
        s = g.pool_stats(float("nan"), -1.0, (3.0, 2.0))
        _check(s, ref, 0.0, 0.0, (), "deque tick %d" % t, deque=True)
        assert s["n_queued"] == len(ref["queue"]) and s["n_queued_expired"] == s["n_expired"] == s["inflight_expired"] == 0
        assert s["dispatchable"] == s["inflight_max"] == -1 and np.isnan(s["oldest_hb"]) and np.isnan(s["newest_hb"])
        assert not s["age_hist"].any() and s["free_hist"].sum() == s["n_registered"] == int(ref["reg"].sum())
        assert s["inflight"] == int((ref["log"] >= 0).sum())
        if tk is None:
            break
        n = carried + tk["n_new"]
        out = g.tick(tk["now"], 0.0, tk["ev_kind"], tk["ev_slot"], tk["ev_val"], tk["ev_ts"],
                     np.full(len(tk["ev_kind"]), -1, np.int64), n)
        carried = n - len(out["assign"])
    assert repeats, "the deque never repeated an id"
    g.close()


# ------------------------------------------------------------------ 5. refusals change nothing
def _state_of(scen):
    return dict(reg=scen["init_reg"], free=scen["init_free"], hb=scen["init_hb"], epoch=scen["init_epoch"],
                queue=scen["init_queue"], log=scen["init_log"])


def _refused(g, code, *a):
    with pytest.raises(FaasbalError) as e:
        g.pool_stats(*a)
    assert e.value.code == code, e.value


def test_refusals():
    scen = synth.random_scenario(8805, W=48, n_ticks=2, max_events=30, max_new=40)
    st, tte = _state_of(scen), scen["tte"]
    g, twin = (GpuBalancer(48, len(st["log"]) + 4000, max_events=64) for _ in range(2))
    g.load(st)
    twin.load(st)
    tk = scen["ticks"][0]
    seq = np.full(len(tk["ev_kind"]), -1, np.int64)
    args = (tk["now"], tte, tk["ev_kind"], tk["ev_slot"], tk["ev_val"], tk["ev_ts"], seq, 30)
    now = tk["now"]
    # arguments
    for bad in (tuple(float(i) for i in range(16)), (2.0, 1.0), (1.0, 1.0), (1.0, float("inf"))):
        _refused(g, _lib.FB_EINVAL, now, tte, bad)
    _refused(g, _lib.FB_EINVAL, float("nan"), tte)
    _refused(g, _lib.FB_EINVAL, now, float("inf"))
    assert g.lib.fb_pool_stats(g.h, now, tte, None, 0, None) == _lib.FB_EINVAL
    _check(g.pool_stats(now, tte, (1.0,)), twin.read_state(), now, tte, (1.0,), "after bad arguments")
    # between launch and wait, between wait and commit
    g.launch(*args)
    _refused(g, _lib.FB_ESTATE, now, tte)
    g.wait()
    _refused(g, _lib.FB_ESTATE, now, tte)
    a = dict(reconnect=g.event_status(), assign=g.assignments(), orphans=g.orphans(), evicted=g.evicted())
    g.commit()
    b = twin.tick(*args)
    for k in ("reconnect", "assign", "orphans", "evicted"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    _check(g.pool_stats(now + 1.0, tte), twin.read_state(), now + 1.0, tte, (), "after the commit")
    # staged events pending
    g.stage(now + 1.0)
    _refused(g, _lib.FB_ESTATE, now + 1.0, tte)
    g.launch_staged(tte, 0)
    g.wait()
    g.commit()
    twin.tick(now + 1.0, tte)
    _check(g.pool_stats(now + 2.0, tte), twin.read_state(), now + 2.0, tte, (), "after the staged tick")
    np.testing.assert_array_equal(g.read_state()["log"], twin.read_state()["log"])
    g.close()
    twin.close()


def test_sharded_context_is_refused():
    from faasbal.sharded import ShardedBalancer
    assert ShardedBalancer.pool_stats is None
    sb = ShardedBalancer(0, 1, 16, 64, max_events=16)
    out = _lib.PoolSummary()
    out.n_slots = -7
    assert sb.lib.fb_pool_stats(sb.h, 1.0, 1.0, None, 0, C.byref(out)) == _lib.FB_ESTATE
    assert out.n_slots == -7
    sb.close()
