"""The goodbye message (FB_EV_LEAVE) on the GPU vs the leave model (tests/leave_model.py,
pinned to the C oracle by tests/test_leave_model.py).

Every apply path: the linked-list grouping (one message, runs of up to 16 through both
register sorts), the radix-sorted path and its rerun, the plan / logscan / split-slots
launch sequences, in-place and lazy log clears, window ticks and the tombstones they leave,
pinned and device-resident batches, fb_apply_events, sharded groups, a deque context (which
refuses it) and the drop-in dispatcher over the real balancer.
"""
import ctypes as C

import numpy as np
import pytest

from faasbal import FaasbalError, GpuBalancer, synth
from faasbal._lib import FB_EINVAL, TickResult
from faasbal.balancer import TEST_PATHS
from leave_cases import SCRIPTED, SEEDS, LOG_ROOM, check_scripted, cmp_out, cmp_state, events, pool, random_run, state
from leave_model import EV_LEAVE, LeaveModel
from oracle import DequeOracle

pytestmark = pytest.mark.gpu

L, REG, HB, RES = EV_LEAVE, 0, 2, 3
NONE = tuple(np.zeros(0, d) for d in (np.uint8, np.int32, np.int32, np.float64, np.int64))


def _gpu(st, cap, max_events=256, window=None):
    g = GpuBalancer(len(st["reg"]), cap, max_events=max_events)
    if window is not None:
        g.set_window(window)
    g.load(st)
    return g


def _model(st, cap):
    m = LeaveModel(len(st["reg"]), cap)
    m.load(st["reg"], st["free"], st["hb"], st["epoch"], st["queue"], st["log"])
    return m


def _replay(seed, W, read_between="full", window=None, few_pending=False):
    """One random scenario with leaves on a one-GPU context: outputs against the model's
    every tick, the state with the log at the end; between ticks the whole state, the state
    without the log (stale entries stay in the log under lazy clears), or nothing."""
    scen, args, outs, states = random_run(seed, W, few_pending=few_pending)
    g = _gpu(state(scen), len(scen["init_log"]) + LOG_ROOM, window=window)
    for t, (a, exp, st) in enumerate(zip(args, outs, states)):
        out = g.tick(*a)
        cmp_out(out, exp, "seed %d tick %d" % (seed, t))
        if read_between == "full":
            cmp_state(g.read_state(), st, "seed %d tick %d" % (seed, t))
        elif read_between == "nolog":
            cmp_state(g.read_state(with_log=False), st, "seed %d tick %d" % (seed, t), with_log=False)
    cmp_state(g.read_state(), states[-1], "seed %d end" % seed)
    live = states[-1]["log"][states[-1]["log"] >= 0]
    np.testing.assert_array_equal(g.inflight(), np.bincount(live, minlength=W).astype(np.uint32))
    return g


@pytest.mark.parametrize("seed,W", SEEDS)
@pytest.mark.parametrize("read_between", ["full", "nolog"])
def test_random_multitick_vs_model(seed, W, read_between):
    _replay(seed, W, read_between).close()


PATHS = {"default": {}, "radix": {"ev_ll": 0}, "plan": {"plan": 1}, "logscan": {"logscan": 1},
         "split_slots": {"logscan": 0, "split_slots": 1}, "eager_clears": {"lazy": 0}}


@pytest.mark.parametrize("seed,W", SEEDS)
@pytest.mark.parametrize("path", sorted(PATHS))
def test_random_multitick_across_paths(monkeypatch, path, seed, W):
    for k, v in PATHS[path].items():
        monkeypatch.setitem(TEST_PATHS, k, v)
    _replay(seed, W, "none").close()


@pytest.mark.parametrize("seed,W", SEEDS)
def test_random_multitick_window_mode(seed, W):
    """Window mode 1 with a handful of pending tasks per tick: ticks stay at fill level 0."""
    _replay(seed, W, "nolog", window=1, few_pending=True).close()


def test_random_window_mode_commits_window_ticks():
    """... and some of those ticks do commit as window ticks.  One scenario may have none -- a
    tick with an unserved front insertion, or one behind a tick above level 0, falls back to
    the general path -- so the count is taken over all eight."""
    n = 0
    for seed, W in SEEDS:
        g = _replay(seed, W, "none", window=1, few_pending=True)
        n += g.window_stats()[0]
        g.close()
    assert n >= 1


@pytest.mark.parametrize("name", sorted(SCRIPTED))
@pytest.mark.parametrize("radix", [0, 1])
def test_scripted(monkeypatch, name, radix):
    if radix:
        monkeypatch.setitem(TEST_PATHS, "ev_ll", 0)
    st, now, tte, ev, n, _ = SCRIPTED[name]
    g, m = _gpu(st, 64), _model(st, 64)
    out = g.tick(now, tte, *ev, n)
    check_scripted(name, out, g.read_state())
    cmp_out(out, m.tick(now, tte, *ev, n), name)
    g.close()


# ------------------------------------------------------------------ window ticks
def _window_pool():
    # 40 workers with one free process each, 0..38 queued in slot order, two in-flight tasks on
    # each of workers 3, 20 and 39; worker 39 is registered and busy (free 0), not queued.  The
    # first tick serves workers 0, 1, 2: worker 3 is then the window's head
    W = 40
    st = pool(W=W, free=1, queue=np.arange(W - 1), log=(3, 20, 39, 3, 20, 39))
    st["free"][W - 1] = 0
    return st


@pytest.mark.parametrize("where,s", [("head", 3), ("deep", 20), ("not_queued", 39)])
def test_leave_in_window_ticks_and_over_the_tombstone(where, s):
    """A leave in a window tick -- the worker at the window's head, deep in the queue behind
    the served prefix, or not queued -- then two more ticks that walk over the tombstone."""
    st = _window_pool()
    g, m = _gpu(st, 256, window=1), _model(st, 256)
    ticks = [(1000.0, NONE, 3),                                       # a level-0 tick opens the window
             (1000.25, events((L, s, 0, 1000.25, -1)), 4),           # the leave: two orphans + 4 tasks
             (1000.5, events((HB, 5, 0, 1000.5, -1)), 12),
             (1000.75, NONE, 30)]
    for t, (now, ev, n) in enumerate(ticks):
        a, b = g.tick(now, 10.0, *ev, n), m.tick(now, 10.0, *ev, n)
        cmp_out(a, b, "%s tick %d" % (where, t))
        if t == 1:
            assert list(a["evicted"]) == [s] and len(a["orphans"]) == 2
        cmp_state(g.read_state(with_log=(t % 2 == 1)), m.export(), "%s tick %d" % (where, t), with_log=(t % 2 == 1))
    cmp_state(g.read_state(), m.export(), where)
    assert g.window_stats()[0] >= 1, g.window_stats()
    g.close()


# ------------------------------------------------------------------ many messages on one slot
def _one_slot_batch(counts, W=64, seed=0):
    """{slot: n} messages per slot, a leave in the middle of each run, kinds mixed around it;
    every other slot quiet.  Clocks ascending."""
    rng = np.random.default_rng(seed)
    ev = []
    for s, n in counts.items():
        kinds = [int(k) for k in rng.choice([REG, 1, HB, RES], size=n, p=[0.2, 0.2, 0.3, 0.3])]
        kinds[n // 2] = L
        ev += [(k, s) for k in kinds]
    order = rng.permutation(len(ev))
    ts = 1000.0 + 0.25 * np.arange(len(ev))
    return events(*[(ev[j][0], ev[j][1], int(rng.integers(0, 4)), float(ts[i]), -1) for i, j in enumerate(order)])


@pytest.mark.parametrize("counts,reruns", [({7: 20}, True), ({3: 3, 9: 9}, False)], ids=["resort_20", "sorts_3_and_9"])
def test_runs_of_messages_with_a_leave_in_the_middle(counts, reruns):
    """20 messages on one slot take the tick through the resort rerun (more than the 16 the
    linked-list path sorts in registers); 3 and 9 exercise its two bitonic networks."""
    st = pool(W=64, free=2, log=tuple(np.repeat(np.arange(64), 2)))
    k, s, v, t, q = _one_slot_batch(counts)
    res = np.nonzero(k == RES)[0]
    q[res] = 2 * s[res] + (np.arange(len(res)) % 2)  # the sender's own entries, some twice
    g, m = _gpu(st, 1024), _model(st, 1024)
    a, b = g.tick(float(t[-1]), 10.0, k, s, v, t, q, 10), m.tick(float(t[-1]), 10.0, k, s, v, t, q, 10)
    cmp_out(a, b, str(counts))
    cmp_state(g.read_state(), m.export(), str(counts))
    if TEST_PATHS.get("ev_ll", 1) != 0:
        assert (a["result"]["reruns"] > 0) == reruns, a["result"]
    g.close()


# ------------------------------------------------------------------ lazy clears
def test_second_leave_does_not_orphan_the_first_registrations_entries():
    """s leaves with live entries, re-registers and gets tasks, leaves again -- no log read in
    between, so under lazy clears the first registration's entries may still sit in the log
    naming s: they are not orphaned a second time."""
    st = pool(W=6, free=2, log=(2, 2, 1, 2))
    g, m = _gpu(st, 256), _model(st, 256)
    ticks = [(1000.25, events((L, 2, 0, 1000.25, -1)), 0),
             (1000.5, events((REG, 2, 3, 1000.5, -1)), 2),
             (1000.75, events((L, 2, 0, 1000.75, -1)), 0),
             (1001.0, NONE, 1)]
    outs = []
    for t, (now, ev, n) in enumerate(ticks):
        a, b = g.tick(now, 10.0, *ev, n), m.tick(now, 10.0, *ev, n)
        cmp_out(a, b, "tick %d" % t)
        outs.append(a)
    assert list(outs[0]["orphans"]) == [0, 1, 3]
    first = list(outs[0]["orphans"])
    assert len(outs[2]["orphans"]) > 0 and not set(outs[2]["orphans"]) & set(first)
    assert all(q >= 4 for q in outs[2]["orphans"])
    cmp_state(g.read_state(), m.export(), "end")
    g.close()


# ------------------------------------------------------------------ pinned and device-resident batches
def _tick_pinned(g, now, tte, k, s, v, t, q, n):
    return g.tick(now, tte, *g.pin_events(k, s, v, t, q), n)


def _tick_device(g, now, tte, k, s, v, t, q, n):
    import torch
    d = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (k, s, v, t, q)]
    g.stage_device(now, *d)
    g.launch_staged(tte, n)
    r = g.wait()
    out = dict(result=r, reconnect=g.event_status(), assign=g.assignments(), orphans=g.orphans(),
               evicted=g.evicted())
    g.commit()
    del d
    return out


@pytest.mark.parametrize("tick", [_tick_pinned, _tick_device], ids=["pinned", "resident"])
def test_batches_the_device_checks(tick):
    """k_ev_link's check of batches the host does not read: kind 5 is applied, kind 6 fails
    the wait naming its index and commits nothing, and the next tick runs."""
    st = pool(W=16, free=2, log=(3, 4, 3, 5))
    g, m = _gpu(st, 256), _model(st, 256)
    ev = events((HB, 1, 0, 999.0, -1), (L, 3, 0, 999.25, -1), (RES, 4, 0, 999.5, 1), (L, 9, 0, 999.5, -1))
    a, b = tick(g, 1000.0, 10.0, *ev, 3), m.tick(1000.0, 10.0, *ev, 3)
    cmp_out(a, b, "kind 5")
    assert list(a["evicted"]) == [3, 9] and list(a["orphans"]) == [0, 2]
    cmp_state(g.read_state(), m.export(), "kind 5")
    bad = events((HB, 1, 0, 1000.0, -1), (L, 4, 0, 1000.0, -1), (6, 5, 0, 1000.0, -1), (HB, 2, 0, 1000.0, -1))
    with pytest.raises(FaasbalError, match="event 2") as e:
        tick(g, 1001.0, 10.0, *bad, 3)
    assert e.value.code == FB_EINVAL
    cmp_state(g.read_state(), m.export(), "after the refused batch")
    ev = events((L, 4, 0, 1001.0, -1))
    a, b = tick(g, 1001.0, 10.0, *ev, 2), m.tick(1001.0, 10.0, *ev, 2)
    cmp_out(a, b, "next tick")
    cmp_state(g.read_state(), m.export(), "next tick")
    g.close()


def test_host_checked_batch_refuses_kind_6():
    g = _gpu(pool(W=8), 64)
    ev = events((L, 1, 0, 999.0, -1), (6, 2, 0, 999.0, -1))
    with pytest.raises(FaasbalError, match="event 1: unknown kind 6"):
        g.tick(1000.0, 10.0, *ev, 1)
    g.close()


# ------------------------------------------------------------------ fb_apply_events
def test_apply_events_through_ctypes():
    """Leaves through fb_apply_events: they evict and report orphans, nothing is dispatched."""
    def p(a):
        return a.ctypes.data_as(C.c_void_p)

    st = pool(W=8, free=2, log=(1, 2, 1, 3, 5))
    g, m = _gpu(st, 64), _model(st, 64)
    k, s, v, t, q = events((L, 1, 0, 999.0, -1), (RES, 3, 0, 999.25, 3), (L, 3, 0, 999.5, -1), (L, 7, 0, 999.5, -1),
                           (HB, 7, 0, 999.75, -1))
    r = TickResult()
    evs, orph, evic = np.zeros(8, np.uint8), np.zeros(64, np.int64), np.zeros(8, np.int32)
    assert g.lib.fb_apply_events(g.h, 10.0, len(k), p(k), p(s), p(v), p(t), p(q), C.byref(r), p(evs), p(orph),
                                 p(evic)) == 0, g.lib.fb_last_error(g.h)
    x = m.tick(float(t[-1]), 10.0, k, s, v, t, q, 0, dispatch_limit=0)
    np.testing.assert_array_equal(evs[:len(k)], x["reconnect"])
    np.testing.assert_array_equal(orph[:r.n_orphans], x["orphans"])
    np.testing.assert_array_equal(evic[:r.n_evicted], x["evicted"])
    assert r.n_assigned == 0 and list(x["orphans"]) == [0, 2] and list(x["evicted"]) == [1, 3]
    assert list(evs[:len(k)]) == [0, 0, 0, 0, 1]  # the heartbeat behind slot 7's leave: reconnect
    cmp_state(g.read_state(), m.export(), "apply_events")
    g.close()


# ------------------------------------------------------------------ deque contexts
def test_deque_context_refuses_a_leave():
    scen = synth.random_deque_scenario(3, W=24, n_ticks=2, max_events=30, max_new=40)
    st = state(scen)
    g = GpuBalancer(24, len(st["log"]) + 512, max_events=64, mode="deque")
    g.load(st)
    o = DequeOracle(24, len(st["log"]) + 512)
    o.load(st["reg"], st["free"], st["hb"], st["epoch"], st["queue"], st["log"])
    before = g.read_state()
    ev = events((REG, 1, 2, 999.0, -1), (REG, 2, 2, 999.0, -1), (L, 1, 0, 999.5, -1))
    with pytest.raises(FaasbalError, match="event 2: leave on a deque context") as e:
        g.tick(1000.0, 0.0, *ev, 4)
    assert e.value.code == FB_EINVAL
    after = g.read_state()
    for key in ("reg", "free", "hb", "queue", "log"):
        np.testing.assert_array_equal(after[key], before[key], err_msg=key)
    tk = scen["ticks"][0]
    args = (tk["now"], 0.0, tk["ev_kind"], tk["ev_slot"], tk["ev_val"], tk["ev_ts"], tk["ev_seq"], tk["n_new"])
    a, b = g.tick(*args), o.tick(*args)
    for key in ("reconnect", "assign"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    sg, so = g.read_state(), o.export()
    for key in ("reg", "queue", "log"):
        np.testing.assert_array_equal(sg[key], so[key], err_msg=key)
    g.close()


# ------------------------------------------------------------------ sharded groups
def _group(st, world, cap):
    import torch  # noqa: F401  (loads the HIP runtime before libfaasbal)
    from faasbal.sharded import LocalShardGroup
    grp = LocalShardGroup(world, len(st["reg"]), cap, max_events=256)
    grp.load(st)
    return grp


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("seed,W", [SEEDS[1], SEEDS[2]])
def test_sharded_random_multitick_vs_model(world, seed, W):
    scen, args, outs, states = random_run(seed, W)
    grp = _group(state(scen), world, len(scen["init_log"]) + LOG_ROOM)
    for t, (a, exp, st) in enumerate(zip(args, outs, states)):
        cmp_out(grp.tick(*a), exp, "world %d seed %d tick %d" % (world, seed, t))
        cmp_state(grp.read_state(), st, "world %d seed %d tick %d" % (world, seed, t))
    grp.close()


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_scripted_queued_worker(world):
    st, now, tte, ev, n, _ = SCRIPTED["queued_three_inflight"]
    grp = _group(st, world, 64)
    out = grp.tick(now, tte, *ev, n)
    check_scripted("queued_three_inflight", out, grp.read_state())
    grp.close()


# ------------------------------------------------------------------ the drop-in dispatcher
@pytest.mark.parametrize("how", ["message", "evict"])
def test_dispatcher_leave_over_the_real_balancer(how):
    from faasbal.dispatcher import GpuPushDispatcher
    from test_leave_dispatcher import leave_scenario
    leave_scenario(GpuPushDispatcher, how).balancer.close()


def test_dispatcher_unknown_leave_and_deque_over_the_real_balancer():
    from faasbal.dispatcher import GpuPushDispatcher
    from test_leave_dispatcher import deque_scenario, unknown_leave_scenario
    unknown_leave_scenario(GpuPushDispatcher).balancer.close()
    deque_scenario(GpuPushDispatcher).balancer.close()
