"""Scenarios with drain and resume messages, shared by the drain tests -- TEST ONLY.

The shape of tests/leave_cases.py, whose helpers these build on: scripted single ticks
with expectations written by hand, and leave_cases' random scenarios (same seeds, same
sizes) with a seeded part of the messages turned into leaves, drains and resumes, run
once through the model (tests/drain_model.py) and shared by every test that needs them.
"""
import functools

import numpy as np

from faasbal import synth
from drain_model import EV_DRAIN, DrainModel, is_draining
from faasbal._lib import FB_DRAIN_BIAS
from leave_cases import LOG_ROOM, events, pool, resolve_seq, state, with_leaves
from leave_model import EV_LEAVE, EV_REGISTER

D = FB_DRAIN_BIAS


def with_drains(scen, seed, frac=0.2):
    """The scenario with a seeded `frac` of its messages that are neither registers nor leaves
    turned into drains (val 1, three in five) and resumes (val 0)."""
    rng = np.random.default_rng(70000 + seed)
    for tk in scen["ticks"]:
        kind, val = tk["ev_kind"].copy(), tk["ev_val"].copy()
        cand = np.nonzero((kind != EV_REGISTER) & (kind != EV_LEAVE))[0]
        pick = cand[rng.random(len(cand)) < frac]
        kind[pick] = EV_DRAIN
        val[pick] = (rng.random(len(pick)) < 0.6).astype(val.dtype)
        tk["ev_kind"], tk["ev_val"] = kind, val
    return scen


@functools.lru_cache(maxsize=None)
def random_run(seed, W, max_events=200, max_new=400, few_pending=False):
    """(scenario, per-tick args, per-tick model outputs, per-tick model states) of one random
    scenario with leaves, drains and resumes; few_pending as in leave_cases.random_run."""
    scen = synth.random_scenario(3000 + seed, W=W, n_ticks=6, max_events=max_events,
                                 max_new=3 if few_pending else max_new)
    scen = with_drains(with_leaves(scen, seed, frac=1.0 / 12.0), seed)
    m = DrainModel(W, len(scen["init_log"]) + LOG_ROOM)
    st = state(scen)
    m.load(st["reg"], st["free"], st["hb"], st["epoch"], st["queue"], st["log"])
    args, outs, states = [], [], []
    carried = 0
    n_live_drains = 0
    for tk in scen["ticks"]:
        seq = resolve_seq(tk, m.export()["log"])
        n = carried + tk["n_new"]
        a = (tk["now"], scen["tte"], tk["ev_kind"], tk["ev_slot"], tk["ev_val"], tk["ev_ts"], seq, n)
        out = m.tick(*a)
        args.append(a)
        outs.append(out)
        states.append(m.export())
        n_live_drains += int((states[-1]["reg"].astype(bool) & (states[-1]["free"] < -(1 << 29))).sum())
        carried = n + len(out["orphans"]) - len(out["assign"])
    assert sum(int((a[2] == EV_DRAIN).sum()) for a in args) > 0, "scenario without a drain"
    assert n_live_drains > 0, "scenario in which no record is ever draining after a tick"
    return scen, args, outs, states


# ------------------------------------------------------------------ scripted cases
_LOG5 = (1, 0, 1, 2, 1)  # worker 1 holds entries 0, 2 and 4
DR, L, REG, RES = EV_DRAIN, EV_LEAVE, EV_REGISTER, 3


def _eight(free1=None, queued1=True, reg7=True, hb1=None):
    """8 workers with two free processes each, all queued in slot order; worker 1 holds three
    in-flight tasks."""
    st = pool(W=8, free=2, log=_LOG5)
    q = list(range(8))
    if free1 is not None:
        st["free"][1] = free1
    if not queued1:
        q.remove(1)
    if not reg7:
        st["reg"][7] = 0
        q.remove(7)
    if hb1 is not None:
        st["hb"][1] = hb1
    st["queue"] = np.asarray(q, np.int32)
    return st


_NOT1 = [0, 2, 3, 4, 5, 6, 7]
_ALL1 = [1] * 8
_GONE = dict(orphans=[0, 2, 4], evicted=[1], assign=[0, 2, 3], queue=[4, 5, 6, 7, 0, 2, 3],
             reg=[1, 0, 1, 1, 1, 1, 1, 1], log=[-1, 0, -1, 2, -1, 0, 2, 3], draining={})
# name -> (state, now, tte, events, n_pending, expected outputs and post-tick facts, written by hand;
#          free1 / hb1: worker 1's record after the tick, draining: slot -> true free count)
SCRIPTED = {
    # a queued worker drains: out of the queue, its record and its three in-flight tasks stay
    # (no orphans, not evicted), the three pending tasks go to 0, 2, 3
    "drain_queued": (_eight(), 1000.5, 10.0, events((DR, 1, 1, 1000.25, -1)), 3, dict(
        reconnect=[0], orphans=[], evicted=[], assign=[0, 2, 3], queue=[4, 5, 6, 7, 0, 2, 3], reg=_ALL1,
        log=[1, 0, 1, 2, 1, 0, 2, 3], free1=2 - D, hb1=1000.0, draining={1: 2})),
    # a busy worker (free 0, not queued) drains: only the mark changes
    "drain_busy": (_eight(free1=0, queued1=False), 1000.5, 10.0, events((DR, 1, 1, 1000.25, -1)), 2, dict(
        reconnect=[0], orphans=[], evicted=[], assign=[0, 2], queue=[3, 4, 5, 6, 7, 0, 2], reg=_ALL1,
        log=[1, 0, 1, 2, 1, 0, 2], free1=-D, hb1=1000.0, draining={1: 0})),
    # drain then result: the entry is completed, free goes up by one, the heartbeat moves, and
    # the worker stays out of the queue
    "drain_then_result": (_eight(), 1000.5, 10.0, events((DR, 1, 1, 1000.25, -1), (RES, 1, 0, 1000.25, 2)), 1, dict(
        reconnect=[0, 0], orphans=[], evicted=[], assign=[0], queue=[2, 3, 4, 5, 6, 7, 0], reg=_ALL1,
        log=[1, 0, -1, 2, 1, 0], free1=3 - D, hb1=1000.25, draining={1: 3})),
    # result then drain on a busy worker: the result brings free to 1 and appends the worker to
    # the queue, the drain takes it out again
    "result_then_drain": (_eight(free1=0, queued1=False), 1000.5, 10.0,
                          events((RES, 1, 0, 1000.25, 2), (DR, 1, 1, 1000.25, -1)), 1, dict(
        reconnect=[0, 0], orphans=[], evicted=[], assign=[0], queue=[2, 3, 4, 5, 6, 7, 0], reg=_ALL1,
        log=[1, 0, -1, 2, 1, 0], free1=1 - D, hb1=1000.25, draining={1: 1})),
    "drain_twice": (_eight(), 1000.5, 10.0, events((DR, 1, 1, 1000.25, -1), (DR, 1, 1, 1000.5, -1)), 0, dict(
        reconnect=[0, 0], orphans=[], evicted=[], assign=[], queue=_NOT1, reg=_ALL1,
        log=list(_LOG5), free1=2 - D, hb1=1000.0, draining={1: 2})),
    "drain_resume_drain": (_eight(), 1000.5, 10.0,
                           events((DR, 1, 1, 1000.25, -1), (DR, 1, 0, 1000.25, -1), (DR, 1, 7, 1000.5, -1)), 0, dict(
        reconnect=[0, 0, 0], orphans=[], evicted=[], assign=[], queue=_NOT1, reg=_ALL1,
        log=list(_LOG5), free1=2 - D, hb1=1000.0, draining={1: 2})),
    # drain then resume: back first in line, as after a reconnect(2); the heartbeat is not touched
    "drain_resume": (_eight(), 1000.5, 10.0, events((DR, 1, 1, 1000.25, -1), (DR, 1, 0, 1000.5, -1)), 1, dict(
        reconnect=[0, 0], orphans=[], evicted=[], assign=[1], queue=[0, 2, 3, 4, 5, 6, 7, 1], reg=_ALL1,
        log=[1, 0, 1, 2, 1, 1], free1=1, hb1=1000.0, draining={})),
    # a resume of a worker that is not draining: nothing (it keeps its place, it is not moved
    # to the front)
    "resume_without_drain": (_eight(), 1000.5, 10.0, events((DR, 1, 0, 1000.25, -1)), 1, dict(
        reconnect=[0], orphans=[], evicted=[], assign=[0], queue=[1, 2, 3, 4, 5, 6, 7, 0], reg=_ALL1,
        log=[1, 0, 1, 2, 1, 0], free1=2, hb1=1000.0, draining={})),
    # a slot without a record: nothing happens, no record, no reconnect; listed as evicted (it
    # got a message and holds no record after the tick)
    "drain_empty_slot": (_eight(reg7=False), 1000.5, 10.0, events((DR, 7, 1, 1000.25, -1)), 1, dict(
        reconnect=[0], orphans=[], evicted=[7], assign=[0], queue=[1, 2, 3, 4, 5, 6, 0],
        reg=[1, 1, 1, 1, 1, 1, 1, 0], log=[1, 0, 1, 2, 1, 0], free1=2, hb1=1000.0, draining={})),
    # drain then leave: the leave deletes the record as ever, its live entries are orphans
    "drain_then_leave": (_eight(), 1000.5, 10.0, events((DR, 1, 1, 1000.25, -1), (L, 1, 0, 1000.25, -1)), 0,
                         dict(_GONE, reconnect=[0, 0])),
    # leave then drain: the drain meets no record and creates none
    "leave_then_drain": (_eight(), 1000.5, 10.0, events((L, 1, 0, 1000.25, -1), (DR, 1, 1, 1000.25, -1)), 0,
                         dict(_GONE, reconnect=[0, 0])),
    # drain then register(2): a restarted worker is a fresh worker -- free 2, front of the
    # queue, the same registration (a register over a live record keeps its epoch)
    "drain_then_register": (_eight(), 1000.5, 10.0, events((DR, 1, 1, 1000.25, -1), (REG, 1, 2, 1000.5, -1)), 1, dict(
        reconnect=[0, 0], orphans=[], evicted=[], assign=[1], queue=[0, 2, 3, 4, 5, 6, 7, 1], reg=_ALL1,
        log=[1, 0, 1, 2, 1, 1], free1=1, hb1=1000.5, draining={})),
    # the purge at the drain's clock deletes the record first: the drain does nothing
    "drain_expired_at_ts": (_eight(hb1=985.0), 1000.5, 10.0, events((DR, 1, 1, 1000.0, -1)), 0,
                            dict(_GONE, reconnect=[0])),
    # an absurd count is clamped into the draining range, and comes back clamped
    "clamp": (_eight(free1=1 << 29), 1000.5, 10.0, events((DR, 1, 1, 1000.25, -1)), 1, dict(
        reconnect=[0], orphans=[], evicted=[], assign=[0], queue=[2, 3, 4, 5, 6, 7, 0], reg=_ALL1,
        log=[1, 0, 1, 2, 1, 0], free1=(1 << 29) - 1 - D, hb1=1000.0, draining={1: (1 << 29) - 1})),
    "clamp_resume": (_eight(free1=1 << 29), 1000.5, 10.0,
                     events((DR, 1, 1, 1000.25, -1), (DR, 1, 0, 1000.25, -1)), 2, dict(
        reconnect=[0, 0], orphans=[], evicted=[], assign=[1, 0], queue=[2, 3, 4, 5, 6, 7, 1, 0], reg=_ALL1,
        log=[1, 0, 1, 2, 1, 1, 0], free1=(1 << 29) - 2, hb1=1000.0, draining={})),
    # a negative count (reconnect(-3) is legal in the reference) keeps its value under the mark
    "negative_free": (_eight(free1=-3), 1000.5, 10.0, events((DR, 1, 1, 1000.25, -1)), 1, dict(
        reconnect=[0], orphans=[], evicted=[], assign=[0], queue=[2, 3, 4, 5, 6, 7, 0], reg=_ALL1,
        log=[1, 0, 1, 2, 1, 0], free1=-3 - D, hb1=1000.0, draining={1: -3})),
    # ... and a resume gives it back without queueing the worker (only a count > 0 does)
    "negative_resume": (_eight(free1=-3), 1000.5, 10.0,
                        events((DR, 1, 1, 1000.25, -1), (DR, 1, 0, 1000.25, -1)), 1, dict(
        reconnect=[0, 0], orphans=[], evicted=[], assign=[0], queue=[2, 3, 4, 5, 6, 7, 0], reg=_ALL1,
        log=[1, 0, 1, 2, 1, 0], free1=-3, hb1=1000.0, draining={})),
}
LOG_CAP = 64


def draining_dict(st):
    """slot -> true free count of the draining records of a state dict"""
    return {int(s): int(st["free"][s]) + D for s in range(len(st["reg"])) if st["reg"][s] and is_draining(int(st["free"][s]))}


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
        assert (int(st["free"][1]), float(st["hb"][1])) == (exp["free1"], exp["hb1"]), name
    assert draining_dict(st) == exp["draining"], name
