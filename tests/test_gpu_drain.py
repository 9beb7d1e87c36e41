"""The planned shutdown (FB_EV_DRAIN: drain / resume) on the GPU vs the drain model
(tests/drain_model.py, pinned to the C oracle by tests/test_drain_model.py).

Every apply path, as tests/test_gpu_leave.py runs the goodbye: the linked-list grouping
(one message, runs at the register sort's seam of 16), the radix-sorted path and its rerun,
the plan / logscan / split-slots launch sequences, in-place and lazy log clears, window
ticks, pinned and device-resident batches, fb_apply_events, sharded groups and a deque
context (which refuses it).  What is new against a leave is the combination "record alive,
queued at tick start, out of the queue after its messages, not dead": every reader of the
post-message queue status meets it here (DESIGN.md §2.1 names them and the test of each).
"""
import ctypes as C

import numpy as np
import pytest

from faasbal import FaasbalError, GpuBalancer, synth
from faasbal._lib import FB_DRAIN_BELOW, FB_DRAIN_BIAS, FB_EINVAL, TickResult
from faasbal.balancer import TEST_PATHS
from drain_cases import LOG_CAP, SCRIPTED, check_scripted, draining_dict, random_run
from drain_model import EV_DRAIN, DrainModel
from leave_cases import LOG_ROOM, SEEDS, cmp_out, cmp_state, events, pool, state
from oracle import DequeOracle
from test_gpu_leave import _tick_device, _tick_pinned, _window_pool

pytestmark = pytest.mark.gpu

DR, REG, REC, HB, RES = EV_DRAIN, 0, 1, 2, 3
NONE = tuple(np.zeros(0, d) for d in (np.uint8, np.int32, np.int32, np.float64, np.int64))


def _gpu(st, cap, max_events=256, window=None):
    g = GpuBalancer(len(st["reg"]), cap, max_events=max_events)
    if window is not None:
        g.set_window(window)
    g.load(st)
    return g


def _model(st, cap):
    m = DrainModel(len(st["reg"]), cap)
    m.load(st["reg"], st["free"], st["hb"], st["epoch"], st["queue"], st["log"])
    return m


def _check_counts(g, st):
    """draining() and fb_read_inflight against the expected state st (with its log)"""
    d = g.draining()
    assert {int(s): int(f) for s, f in zip(d["slot"], d["free"])} == draining_dict(st)
    live = st["log"][st["log"] >= 0]
    np.testing.assert_array_equal(g.inflight(), np.bincount(live, minlength=len(st["reg"])).astype(np.uint32))


def _replay(seed, W, read_between="full", window=None, few_pending=False):
    """One random scenario with leaves, drains and resumes on a one-GPU context: outputs
    against the model's every tick, the state with the log, the draining set and the in-flight
    counts at the end; between ticks the whole state, the state without the log, or nothing."""
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
    _check_counts(g, states[-1])
    return g


@pytest.mark.parametrize("seed,W", SEEDS)
@pytest.mark.parametrize("read_between", ["full", "nolog", "none"])
def test_random_multitick_vs_model(seed, W, read_between):
    _replay(seed, W, read_between).close()


PATHS = {"radix": {"ev_ll": 0}, "plan": {"plan": 1}, "logscan": {"logscan": 1},
         "split_slots": {"logscan": 0, "split_slots": 1}, "eager_clears": {"lazy": 0}}


@pytest.mark.parametrize("seed,W", SEEDS)
@pytest.mark.parametrize("path", sorted(PATHS))
def test_random_multitick_across_paths(monkeypatch, path, seed, W):
    for k, v in PATHS[path].items():
        monkeypatch.setitem(TEST_PATHS, k, v)
    _replay(seed, W, "none").close()


@pytest.mark.parametrize("seed,W", SEEDS)
def test_random_multitick_window_mode(seed, W):
    _replay(seed, W, "nolog", window=1, few_pending=True).close()


@pytest.mark.parametrize("name", sorted(SCRIPTED))
@pytest.mark.parametrize("ev_ll", [1, 0])
def test_scripted(monkeypatch, name, ev_ll):
    if not ev_ll:
        monkeypatch.setitem(TEST_PATHS, "ev_ll", 0)
    st, now, tte, ev, n, _ = SCRIPTED[name]
    g, m = _gpu(st, LOG_CAP), _model(st, LOG_CAP)
    out = g.tick(now, tte, *ev, n)
    post = g.read_state()
    check_scripted(name, out, post)
    cmp_out(out, m.tick(now, tte, *ev, n), name)
    _check_counts(g, m.export())
    # the tick after: the committed state is a state like any other
    a, b = g.tick(now + 0.25, tte, *NONE, 5), m.tick(now + 0.25, tte, *NONE, 5)
    cmp_out(a, b, name + " next")
    cmp_state(g.read_state(), m.export(), name + " next")
    g.close()


# ------------------------------------------------------------------ window ticks
@pytest.mark.parametrize("where,s", [("head", 3), ("inside", 20), ("beyond", 39)])
def test_drain_in_window_ticks(where, s):
    """A drain in a window tick -- the worker at the window's head, inside the window behind
    the served prefix, or beyond it (not queued) -- then ticks that walk over the position it
    left, a result of the drained worker, and its resume (a front insertion).  All four
    commit as window ticks."""
    st = _window_pool()
    g, m = _gpu(st, 256, window=1), _model(st, 256)
    q0 = {3: 0, 20: 1, 39: 2}[s]
    ticks = [(1000.0, NONE, 3),                                       # a level-0 tick opens the window
             (1000.25, events((DR, s, 1, 1000.25, -1)), 4),           # the drain: no orphans, 4 tasks
             (1000.5, events((HB, 5, 0, 1000.5, -1), (RES, s, 0, 1000.5, q0)), 12),
             (1000.75, events((HB, 6, 0, 1000.75, -1)), 10),         # (only message ticks are window ticks)
             (1001.0, events((DR, s, 0, 1001.0, -1)), 2)]             # the resume: first in line
    wins = []
    for t, (now, ev, n) in enumerate(ticks):
        a, b = g.tick(now, 10.0, *ev, n), m.tick(now, 10.0, *ev, n)
        cmp_out(a, b, "%s tick %d" % (where, t))
        if t == 1:
            assert len(a["evicted"]) == 0 and len(a["orphans"]) == 0 and s not in a["assign"]
        if t == 4:
            assert a["assign"][0] == s
        wins.append(g.window_stats()[0])
        cmp_state(g.read_state(with_log=(t % 2 == 1)), m.export(), "%s tick %d" % (where, t), with_log=(t % 2 == 1))
    cmp_state(g.read_state(), m.export(), where)
    _check_counts(g, m.export())
    # every tick behind the first has messages and follows a level-0 tick (fewer tasks than
    # queued workers), which is what the plan asks of a window tick (plan_window): the drain,
    # the result, the walk over the position the drain left and the resume all commit as one
    assert [b - a for a, b in zip(wins, wins[1:])] == [1, 1, 1, 1], (wins, g.window_stats())
    g.close()


# ------------------------------------------------------------------ many messages on one slot
def _one_slot_batch(counts, seed=0):
    """{slot: n} messages per slot, a drain in the middle of each run, kinds mixed around it
    (resumes and further drains among them); every other slot quiet.  Clocks ascending."""
    rng = np.random.default_rng(seed)
    ev = []
    for s, n in counts.items():
        kinds = [int(k) for k in rng.choice([REG, REC, HB, RES, DR], size=n, p=[0.1, 0.1, 0.2, 0.3, 0.3])]
        kinds[n // 2] = DR
        ev += [(k, s, (1 if j == n // 2 else int(rng.integers(0, 3)))) for j, k in enumerate(kinds)]
    order = rng.permutation(len(ev))
    ts = 1000.0 + 0.25 * np.arange(len(ev))
    return events(*[(ev[j][0], ev[j][1], ev[j][2], float(ts[i]), -1) for i, j in enumerate(order)])


@pytest.mark.parametrize("counts,reruns", [({7: 16}, False), ({7: 17}, True), ({3: 3, 9: 9}, False)],
                         ids=["run_16", "run_17_resorts", "sorts_3_and_9"])
@pytest.mark.parametrize("seed", [0, 1])
def test_runs_of_messages_with_a_drain_in_the_middle(counts, reruns, seed):
    """16 messages on one slot are the most the linked-list path sorts in registers, 17 take
    the tick through the resort rerun; 3 and 9 exercise its two bitonic networks."""
    st = pool(W=64, free=2, log=tuple(np.repeat(np.arange(64), 2)))
    k, s, v, t, q = _one_slot_batch(counts, seed)
    res = np.nonzero(k == RES)[0]
    q[res] = 2 * s[res] + (np.arange(len(res)) % 2)  # the sender's own entries, some twice
    g, m = _gpu(st, 1024), _model(st, 1024)
    a, b = g.tick(float(t[-1]), 10.0, k, s, v, t, q, 10), m.tick(float(t[-1]), 10.0, k, s, v, t, q, 10)
    cmp_out(a, b, str(counts))
    cmp_state(g.read_state(), m.export(), str(counts))
    _check_counts(g, m.export())
    if TEST_PATHS.get("ev_ll", 1) != 0:
        assert (a["result"]["reruns"] > 0) == reruns, a["result"]
    g.close()


# ------------------------------------------------------------------ pinned and device-resident batches
@pytest.mark.parametrize("tick", [_tick_pinned, _tick_device], ids=["pinned", "resident"])
def test_batches_the_device_checks(tick):
    """k_ev_link's check of batches the host does not read: kind 7 is applied, kinds 6 and 8
    fail the wait naming their index and commit nothing, and the next tick runs."""
    st = pool(W=16, free=2, log=(3, 4, 3, 5))
    g, m = _gpu(st, 256), _model(st, 256)
    ev = events((HB, 1, 0, 999.0, -1), (DR, 3, 1, 999.25, -1), (RES, 4, 0, 999.5, 1), (DR, 9, 1, 999.5, -1),
                (RES, 3, 0, 999.75, 0))
    a, b = tick(g, 1000.0, 10.0, *ev, 3), m.tick(1000.0, 10.0, *ev, 3)
    cmp_out(a, b, "kind 7")
    assert len(a["evicted"]) == 0 and len(a["orphans"]) == 0 and 3 not in a["assign"] and 9 not in a["assign"]
    cmp_state(g.read_state(), m.export(), "kind 7")
    _check_counts(g, m.export())
    for bad_kind, idx in ((6, 2), (8, 1), (255, 3)):
        bad = [(HB, 1, 0, 1000.0, -1), (DR, 4, 1, 1000.0, -1), (HB, 5, 0, 1000.0, -1), (HB, 2, 0, 1000.0, -1)]
        bad[idx] = (bad_kind, 5, 0, 1000.0, -1)
        # by name: fb_tick_wait reads a pinned batch back and names the kind; of a resident
        # batch it has the index from the device and the list of what the check refuses
        named = "event %d: unknown kind %d" % (idx, bad_kind) if tick is _tick_pinned else \
            "event %d: invalid message .*unknown kind" % idx
        with pytest.raises(FaasbalError, match=named) as e:
            tick(g, 1001.0, 10.0, *events(*bad), 3)
        assert e.value.code == FB_EINVAL
        cmp_state(g.read_state(), m.export(), "after the refused batch")
    ev = events((DR, 3, 0, 1001.0, -1), (DR, 4, 1, 1001.0, -1))
    a, b = tick(g, 1001.0, 10.0, *ev, 2), m.tick(1001.0, 10.0, *ev, 2)
    cmp_out(a, b, "next tick")
    cmp_state(g.read_state(), m.export(), "next tick")
    g.close()


def test_host_checked_batch_refuses_kinds_6_and_8_by_name():
    g = _gpu(pool(W=8), 64)
    for k in (6, 8):
        ev = events((DR, 1, 1, 999.0, -1), (k, 2, 0, 999.0, -1))
        with pytest.raises(FaasbalError, match="event 1: unknown kind %d" % k):
            g.tick(1000.0, 10.0, *ev, 1)
    assert len(g.draining()["slot"]) == 0
    g.close()


# ------------------------------------------------------------------ fb_apply_events
def test_apply_events_through_ctypes():
    """Drains through fb_apply_events: the marks are set, nothing is orphaned or dispatched."""
    def p(a):
        return a.ctypes.data_as(C.c_void_p)

    st = pool(W=8, free=2, log=(1, 2, 1, 3, 5))
    g, m = _gpu(st, 64), _model(st, 64)
    k, s, v, t, q = events((DR, 1, 1, 999.0, -1), (RES, 3, 0, 999.25, 3), (DR, 3, 1, 999.5, -1), (DR, 7, 1, 999.5, -1),
                           (DR, 7, 0, 999.75, -1), (RES, 1, 0, 999.75, 0))
    r = TickResult()
    evs, orph, evic = np.zeros(8, np.uint8), np.zeros(64, np.int64), np.zeros(8, np.int32)
    assert g.lib.fb_apply_events(g.h, 10.0, len(k), p(k), p(s), p(v), p(t), p(q), C.byref(r), p(evs), p(orph),
                                 p(evic)) == 0, g.lib.fb_last_error(g.h)
    x = m.tick(float(t[-1]), 10.0, k, s, v, t, q, 0, dispatch_limit=0)
    np.testing.assert_array_equal(evs[:len(k)], x["reconnect"])
    assert r.n_assigned == 0 and r.n_orphans == 0 and r.n_evicted == 0 and not evs.any()
    cmp_state(g.read_state(), m.export(), "apply_events")
    assert draining_dict(g.read_state()) == {1: 3, 3: 3}
    _check_counts(g, m.export())
    g.close()


# ------------------------------------------------------------------ deque contexts
def test_deque_context_refuses_a_drain():
    scen = synth.random_deque_scenario(3, W=24, n_ticks=2, max_events=30, max_new=40)
    st = state(scen)
    g = GpuBalancer(24, len(st["log"]) + 512, max_events=64, mode="deque")
    g.load(st)
    o = DequeOracle(24, len(st["log"]) + 512)
    o.load(st["reg"], st["free"], st["hb"], st["epoch"], st["queue"], st["log"])
    before = g.read_state()
    for val in (1, 0):
        ev = events((REG, 1, 2, 999.0, -1), (REG, 2, 2, 999.0, -1), (DR, 1, val, 999.5, -1))
        with pytest.raises(FaasbalError, match="event 2: drain on a deque context") as e:
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
    g.close()


# ------------------------------------------------------------------ sharded groups
def _group(st, world, cap):
    import torch  # noqa: F401  (loads the HIP runtime before libfaasbal)
    from faasbal.sharded import LocalShardGroup
    grp = LocalShardGroup(world, len(st["reg"]), cap, max_events=256)
    grp.load(st)
    return grp


@pytest.mark.parametrize("s", [1, 5], ids=["rank0", "rank1"])
def test_sharded_drain_on_each_rank_in_turn(s):
    """World 2 over eight workers: the drained slot on rank 0, then on rank 1 -- drain, a
    result of the drained worker, the resume."""
    st = pool(W=8, free=2, log=(s, 0, s, 2, s))
    grp, m = _group(st, 2, 256), _model(st, 256)
    ticks = [(1000.25, events((DR, s, 1, 1000.25, -1)), 3),
             (1000.5, events((RES, s, 0, 1000.5, 2), (HB, 0, 0, 1000.5, -1)), 9),
             (1000.75, events((DR, s, 0, 1000.75, -1)), 2),
             (1001.0, NONE, 4)]
    for t, (now, ev, n) in enumerate(ticks):
        a, b = grp.tick(now, 10.0, *ev, n), m.tick(now, 10.0, *ev, n)
        cmp_out(a, b, "tick %d" % t)
        exp = m.export()
        cmp_state(grp.read_state(), exp, "tick %d" % t)
        d = grp.draining()
        assert {int(x): int(f) for x, f in zip(d["slot"], d["free"])} == draining_dict(exp), t
        if t < 2:
            assert s not in a["assign"] and list(d["slot"]) == [s]
        if t == 2:
            assert a["assign"][0] == s
    grp.close()


@pytest.mark.parametrize("seed,W", [SEEDS[1], SEEDS[2]])
def test_sharded_random_multitick_vs_model(seed, W):
    scen, args, outs, states = random_run(seed, W)
    grp = _group(state(scen), 2, len(scen["init_log"]) + LOG_ROOM)
    for t, (a, exp, st) in enumerate(zip(args, outs, states)):
        cmp_out(grp.tick(*a), exp, "seed %d tick %d" % (seed, t))
        cmp_state(grp.read_state(), st, "seed %d tick %d" % (seed, t))
    grp.close()


# ------------------------------------------------------------------ the encoding is the state
@pytest.mark.parametrize("seed,W", [SEEDS[0], SEEDS[1], SEEDS[2]])
def test_state_after_drain_ticks_round_trips_through_a_load(seed, W):
    """After every tick: read_state -> load into a second context -> the next tick's outputs
    and states are equal.  The mark travels in the free counts and nowhere else."""
    scen, args, outs, states = random_run(seed, W)
    cap = len(scen["init_log"]) + LOG_ROOM
    g = _gpu(state(scen), cap)
    g2 = GpuBalancer(W, cap, max_events=256)
    for t in range(len(args) - 1):
        cmp_out(g.tick(*args[t]), outs[t], "seed %d tick %d" % (seed, t))
        g2.load(g.read_state())
        out2 = g2.tick(*args[t + 1])
        cmp_out(out2, outs[t + 1], "seed %d loaded before tick %d" % (seed, t + 1))
        cmp_state(g2.read_state(), states[t + 1], "seed %d loaded before tick %d" % (seed, t + 1))
        _check_counts(g2, states[t + 1])
    g.close()
    g2.close()


# ------------------------------------------------------------------ a drained worker dies
@pytest.mark.parametrize("plan", [0, 1, 2])
def test_drained_worker_dies_next_tick_orphans_are_its_live_entries(monkeypatch, plan):
    """Worker 1 drains holding entries 0, 2 and 4, completes entry 2, and its heartbeat expires
    in the next tick while the others' are fresh: the orphans are exactly entries 0 and 4
    (the in-flight budget moved with the free count: DESIGN.md §5g)."""
    monkeypatch.setitem(TEST_PATHS, "plan", plan)
    st = SCRIPTED["drain_queued"][0]
    g, m = _gpu(st, LOG_CAP), _model(st, LOG_CAP)
    ev = events((DR, 1, 1, 1000.25, -1), (RES, 1, 0, 1000.25, 2), *[(HB, w, 0, 1005.0, -1) for w in (0, 2, 3, 4, 5, 6, 7)])
    a, b = g.tick(1005.0, 10.0, *ev, 3), m.tick(1005.0, 10.0, *ev, 3)
    cmp_out(a, b, "drain")
    _check_counts(g, m.export())
    assert int(g.inflight()[1]) == 2
    a, b = g.tick(1011.0, 10.0, *NONE, 1), m.tick(1011.0, 10.0, *NONE, 1)
    cmp_out(a, b, "death")
    assert list(a["orphans"]) == [0, 4] and list(a["evicted"]) == [1] and len(a["assign"]) == 3
    cmp_state(g.read_state(), m.export(), "death")
    _check_counts(g, m.export())
    g.close()


@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("ev_ll", [1, 0])
def test_resume_of_a_count_wider_than_the_round_table(monkeypatch, world, ev_ll):
    """A resume puts a worker with 100 free processes first in line while every count the
    launch can size its round table from is 2 (the batch's register / reconnect values: none;
    the last tick's queue: 2 each): 112 tasks fill the pool to level 99, past the first table,
    and the tick comes out right through its wider rerun.  Then the same from a loaded state."""
    if not ev_ll:
        monkeypatch.setitem(TEST_PATHS, "ev_ll", 0)
    st = pool(W=8, free=2)
    st["free"][1] = 100
    g = _gpu(st, 1024) if world == 1 else _group(st, world, 1024)
    m = _model(st, 1024)
    ticks = [(1000.25, events((DR, 1, 1, 1000.25, -1)), 2),
             (1000.5, events((DR, 1, 0, 1000.5, -1), (HB, 2, 0, 1000.5, -1)), 150)]
    for t, (now, ev, n) in enumerate(ticks):
        a, b = g.tick(now, 10.0, *ev, n), m.tick(now, 10.0, *ev, n)
        cmp_out(a, b, "tick %d" % t)
        cmp_state(g.read_state(), m.export(), "tick %d" % t)
    assert len(a["assign"]) == 112 and int((a["assign"] == 1).sum()) == 100 and a["result"]["fill_level"] >= 99
    g.close()


def test_draining_lists_true_free_counts():
    st = pool(W=8, free=2)
    st["free"][2], st["free"][6] = 5 - FB_DRAIN_BIAS, -FB_DRAIN_BIAS
    st["reg"][6] = 0                                     # no record: not listed whatever its count
    st["queue"] = np.asarray([0, 1, 3, 4, 5, 7], np.int32)
    g = _gpu(st, 64)
    d = g.draining()
    assert list(d["slot"]) == [2] and list(d["free"]) == [5] and st["free"][2] < FB_DRAIN_BELOW
    s = g.pool_stats(1000.0, 10.0)
    assert s["free_total"] == 2 * 6 and s["free_hist"][0] == 1 and s["free_hist"][2] == 6
    g.close()
