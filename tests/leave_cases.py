"""Scenarios with goodbye messages, shared by the leave tests -- TEST ONLY.

synth.random_scenario knows no leave: the tests turn a seeded sixth of its non-register
messages into leaves themselves, resolve the results against the model's log as
test_random_multitick_vs_oracle does against the oracle's, and run the model
(tests/leave_model.py) once per scenario -- every test that needs the expected outputs
and states of a scenario shares that one run.
"""
import functools

import numpy as np

from faasbal import synth
from leave_model import EV_LEAVE, EV_REGISTER, LeaveModel

SEEDS = [(seed, [5, 37, 300][seed % 3]) for seed in range(8)]  # 8 seeds over W in {5, 37, 300}
LOG_ROOM = 8000


def state(scen):
    return dict(reg=scen["init_reg"], free=scen["init_free"], hb=scen["init_hb"], epoch=scen["init_epoch"],
                queue=scen["init_queue"], log=scen["init_log"])


def resolve_seq(tk, log):
    """result messages -> in-flight sequence numbers of the sender (or -1)"""
    seq = np.full(len(tk["ev_kind"]), -1, np.int64)
    for i in np.nonzero(tk["ev_kind"] == synth.EV_RESULT)[0]:
        mine = np.nonzero(log == tk["ev_slot"][i])[0]
        if len(mine) and tk["ev_pick"][i] % 5 != 4:
            seq[i] = mine[tk["ev_pick"][i] % len(mine)]
    return seq


def with_leaves(scen, seed, frac=1.0 / 6.0):
    """The scenario with a seeded `frac` of its non-register messages turned into leaves."""
    rng = np.random.default_rng(90000 + seed)
    for tk in scen["ticks"]:
        kind = tk["ev_kind"].copy()
        cand = np.nonzero(kind != EV_REGISTER)[0]
        kind[cand[rng.random(len(cand)) < frac]] = EV_LEAVE
        tk["ev_kind"] = kind
    return scen


@functools.lru_cache(maxsize=None)
def random_run(seed, W, max_events=200, max_new=400, few_pending=False):
    """(scenario, per-tick args, per-tick model outputs, per-tick model states) of one random
    scenario with leaves; few_pending: at most a handful of tasks per tick (window ticks
    that stay at fill level 0)."""
    scen = with_leaves(synth.random_scenario(3000 + seed, W=W, n_ticks=6, max_events=max_events,
                                             max_new=3 if few_pending else max_new), seed)
    m = LeaveModel(W, len(scen["init_log"]) + LOG_ROOM)
    st = state(scen)
    m.load(st["reg"], st["free"], st["hb"], st["epoch"], st["queue"], st["log"])
    args, outs, states = [], [], []
    carried = 0
    for tk in scen["ticks"]:
        seq = resolve_seq(tk, m.export()["log"])
        n = carried + tk["n_new"]
        a = (tk["now"], scen["tte"], tk["ev_kind"], tk["ev_slot"], tk["ev_val"], tk["ev_ts"], seq, n)
        out = m.tick(*a)
        args.append(a)
        outs.append(out)
        states.append(m.export())
        carried = n + len(out["orphans"]) - len(out["assign"])
    assert sum(int((a[2] == EV_LEAVE).sum()) for a in args) > 0, "scenario without a leave"
    return scen, args, outs, states


def cmp_out(a, b, where):
    for k in ("reconnect", "assign", "orphans", "evicted"):
        np.testing.assert_array_equal(a[k], b[k], err_msg="%s: %s" % (where, k))


def cmp_state(sa, sb, where, with_log=True):
    """sa against the expected sb: records of registered slots, the queue, the log."""
    np.testing.assert_array_equal(sa["reg"], sb["reg"], err_msg="%s reg" % where)
    reg = np.asarray(sb["reg"]).astype(bool)
    for k in ("free", "hb", "epoch"):
        np.testing.assert_array_equal(np.asarray(sa[k])[reg], np.asarray(sb[k])[reg], err_msg="%s %s" % (where, k))
    np.testing.assert_array_equal(sa["queue"], sb["queue"], err_msg="%s queue" % where)
    if with_log:
        np.testing.assert_array_equal(sa["log"], sb["log"], err_msg="%s log" % where)


# ------------------------------------------------------------------ scripted cases
def pool(W=8, free=2, now=1000.0, queue=None, log=()):
    """W registered workers, heartbeats at now, all queued in slot order."""
    return dict(reg=np.ones(W, np.uint8), free=np.full(W, free, np.int32), hb=np.full(W, float(now)),
                epoch=np.zeros(W, np.uint32), queue=np.arange(W, dtype=np.int32) if queue is None else
                np.asarray(queue, np.int32), log=np.asarray(log, np.int32))


def events(*ev):
    """(kind, slot, val, ts, seq) tuples -> the five arrays"""
    k = np.asarray([e[0] for e in ev], np.uint8)
    s = np.asarray([e[1] for e in ev], np.int32)
    v = np.asarray([e[2] for e in ev], np.int32)
    t = np.asarray([e[3] for e in ev], np.float64)
    q = np.asarray([e[4] for e in ev], np.int64)
    return k, s, v, t, q


_LOG5 = (1, 0, 1, 2, 1)  # worker 1 holds entries 0, 2 and 4


def _four(**kw):
    return pool(W=4, free=2, log=_LOG5, **kw)


def _never_seen():
    st = _four()
    st["reg"][3] = 0
    st["queue"] = np.asarray([0, 1, 2], np.int32)
    return st


def _expired():
    st = _four()
    st["hb"][1] = 985.0
    return st


L, REG, RES, HB = EV_LEAVE, EV_REGISTER, 3, 2
# name -> (state, now, tte, events, n_pending, expected outputs and post-tick facts, written by hand)
SCRIPTED = {
    # a queued worker with three in-flight tasks says goodbye: evicted, its three tasks are the
    # orphans and are dispatched first (3 orphans + 2 pending over the queue 0, 2, 3 with two free
    # processes each), and it is out of the next queue
    "queued_three_inflight": (_four(), 1000.5, 10.0, events((L, 1, 0, 1000.25, -1)), 2, dict(
        reconnect=[0], orphans=[0, 2, 4], evicted=[1], assign=[0, 2, 3, 0, 2], queue=[3], reg=[1, 0, 1, 1],
        log=[-1, 0, -1, 2, -1, 0, 2, 3, 0, 2])),
    # result then leave: the completed entry is not orphaned
    "result_then_leave": (_four(), 1000.5, 10.0, events((RES, 1, 0, 1000.25, 2), (L, 1, 0, 1000.25, -1)), 0, dict(
        reconnect=[0, 0], orphans=[0, 4], evicted=[1], assign=[0, 2], queue=[3, 0, 2], reg=[1, 0, 1, 1],
        log=[-1, 0, -1, 2, -1, 0, 2])),
    # leave then result: the result meets an unknown identity -- reconnect, its entry is orphaned
    # with the others, and the free = 0 record of :356-358 is left behind (so: not evicted)
    "leave_then_result": (_four(), 1000.5, 10.0, events((L, 1, 0, 1000.25, -1), (RES, 1, 0, 1000.25, 2)), 0, dict(
        reconnect=[0, 1], orphans=[0, 2, 4], evicted=[], assign=[0, 2, 3], queue=[0, 2, 3], reg=[1, 1, 1, 1],
        log=[-1, 0, -1, 2, -1, 0, 2, 3], free1=0, epoch1=5, hb1=1000.25)),
    # leave then register in one tick: not evicted, a new epoch, the old entries orphaned and
    # dispatched first -- the new registration, moved to the front, takes the first
    "leave_then_register": (_four(), 1000.5, 10.0, events((L, 1, 0, 1000.25, -1), (REG, 1, 3, 1000.25, -1)), 0, dict(
        reconnect=[0, 0], orphans=[0, 2, 4], evicted=[], assign=[1, 0, 2], queue=[3, 1, 0, 2], reg=[1, 1, 1, 1],
        log=[-1, 0, -1, 2, -1, 1, 0, 2], free1=2, epoch1=5, hb1=1000.25)),
    "leave_twice": (_four(), 1000.5, 10.0, events((L, 1, 0, 1000.25, -1), (L, 1, 0, 1000.5, -1)), 2, dict(
        reconnect=[0, 0], orphans=[0, 2, 4], evicted=[1], assign=[0, 2, 3, 0, 2], queue=[3], reg=[1, 0, 1, 1],
        log=[-1, 0, -1, 2, -1, 0, 2, 3, 0, 2])),
    # a slot that never had a record: nothing happens, no record, no reconnect -- and the evicted
    # list names it (it got a message and holds no record after the tick)
    "never_seen": (_never_seen(), 1000.5, 10.0, events((L, 3, 0, 1000.25, -1)), 1, dict(
        reconnect=[0], orphans=[], evicted=[3], assign=[0], queue=[1, 2, 0], reg=[1, 1, 1, 0],
        log=[1, 0, 1, 2, 1, 0])),
    # the purge at the leave's clock had deleted the record anyway
    "expired_anyway": (_expired(), 1000.5, 10.0, events((L, 1, 0, 1000.0, -1)), 0, dict(
        reconnect=[0], orphans=[0, 2, 4], evicted=[1], assign=[0, 2, 3], queue=[0, 2, 3], reg=[1, 0, 1, 1],
        log=[-1, 0, -1, 2, -1, 0, 2, 3])),
    # nobody ever expires: the leave is the only way out
    "tte_inf": (_expired(), 1000.5, float("inf"), events((L, 2, 0, 1000.25, -1)), 1, dict(
        reconnect=[0], orphans=[3], evicted=[2], assign=[0, 1], queue=[3, 0, 1], reg=[1, 1, 0, 1],
        log=[1, 0, 1, -1, 1, 0, 1])),
}


def check_scripted(name, out, st):
    """the hand-written expectations of SCRIPTED[name] against a tick's outputs and post-tick state"""
    exp = SCRIPTED[name][5]
    for k in ("reconnect", "orphans", "evicted", "assign"):
        np.testing.assert_array_equal(np.asarray(out[k]).astype(np.int64), np.asarray(exp[k], np.int64),
                                      err_msg="%s: %s" % (name, k))
    for k in ("queue", "reg", "log"):
        np.testing.assert_array_equal(np.asarray(st[k]).astype(np.int64), np.asarray(exp[k], np.int64),
                                      err_msg="%s: %s" % (name, k))
    if "free1" in exp:
        assert (int(st["free"][1]), int(st["epoch"][1]), float(st["hb"][1])) == (exp["free1"], exp["epoch1"], exp["hb1"])
