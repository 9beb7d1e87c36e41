"""The drain model (tests/drain_model.py) pinned to the C oracle -- CPU.

The model is what the GPU tests of FB_EV_DRAIN compare against, and it is trusted only as
far as these tests tie it to oracle/push_oracle.c: (a) without kind 7 it is the oracle,
output for output and state for state, on leave_cases' scenarios with the leaves stripped;
(b) the split form: a batch whose only drains (resumes) are its last messages, all at
ts = now, equals the oracle run in two halves around an edit of the exported state -- the
one honest statement of the encoding: a draining record is a record out of the queue whose
free count carries the bias; (c) scripted cases with expectations written by hand.
"""
import numpy as np
import pytest

from faasbal import synth
from faasbal._lib import FB_DRAIN_BELOW, FB_DRAIN_BIAS
from drain_cases import LOG_CAP, SCRIPTED, check_scripted, random_run as drain_run
from drain_model import CLAMP, EV_DRAIN, DrainModel
from leave_cases import SEEDS, cmp_out, cmp_state, resolve_seq, state, with_leaves
from leave_model import EV_LEAVE
from oracle import Oracle

ROOM = 8000
NONE = tuple(np.zeros(0, d) for d in (np.uint8, np.int32, np.int32, np.float64, np.int64))


def _pair(st, cap):
    W = len(st["reg"])
    m, o = DrainModel(W, cap), Oracle(W, cap)
    for x in (m, o):
        x.load(st["reg"], st["free"], st["hb"], st["epoch"], st["queue"], st["log"])
    return m, o


@pytest.mark.parametrize("seed,W", SEEDS)
def test_batches_without_kind_7_equal_the_oracle(seed, W):
    """leave_cases' scenarios with the leaves stripped from the batches."""
    scen = with_leaves(synth.random_scenario(3000 + seed, W=W, n_ticks=6, max_events=200, max_new=400), seed)
    m, o = _pair(state(scen), len(scen["init_log"]) + ROOM)
    carried = 0
    for t, tk in enumerate(scen["ticks"]):
        keep = tk["ev_kind"] != EV_LEAVE
        tk = {k: (v[keep] if isinstance(v, np.ndarray) and len(v) == len(keep) else v) for k, v in tk.items()}
        seq = resolve_seq(tk, o.export()["log"])
        n = carried + tk["n_new"]
        args = (tk["now"], scen["tte"], tk["ev_kind"], tk["ev_slot"], tk["ev_val"], tk["ev_ts"], seq, n)
        a, b = m.tick(*args), o.tick(*args)
        cmp_out(a, b, "tick %d" % t)
        sm, so = m.export(), o.export()
        cmp_state(sm, so, "tick %d" % t)
        for k in ("free", "hb", "epoch"):
            np.testing.assert_array_equal(sm[k], so[k], err_msg="tick %d %s (all slots)" % (t, k))
        carried = n + len(b["orphans"]) - len(b["assign"])


def _split(o, st, now, tte, head_msgs, tail_slots, drain, T):
    """The oracle's side of the split form, from state st: the messages before the trailing
    drains / resumes with nothing dispatched, the exported state edited as the rule says,
    loaded, and the dispatch of T + the first half's orphans.  Returns (outputs, evicted)."""
    o.load(st["reg"], st["free"], st["hb"], st["epoch"], st["queue"], st["log"])
    first = o.tick(now, tte, *head_msgs, 0, dispatch_limit=0)
    x = o.export()
    free, queue = x["free"].copy(), [int(s) for s in x["queue"]]
    for s in tail_slots:  # in message order
        if not x["reg"][s]:
            continue
        if drain and free[s] >= FB_DRAIN_BELOW:
            free[s] = min(int(free[s]), CLAMP) - FB_DRAIN_BIAS
            if s in queue:
                queue.remove(s)
        elif not drain and free[s] < FB_DRAIN_BELOW:
            free[s] += FB_DRAIN_BIAS
            if free[s] > 0:
                if s in queue:
                    queue.remove(s)
                queue.insert(0, s)
    o.load(x["reg"], free, x["hb"], x["epoch"], np.asarray(queue, np.int32), x["log"])
    second = o.tick(now, tte, *NONE, T + len(first["orphans"]))
    assert len(second["orphans"]) == 0
    return dict(reconnect=first["reconnect"], assign=second["assign"], orphans=first["orphans"]), \
        np.union1d(first["evicted"], second["evicted"])


@pytest.mark.parametrize("drain", [True, False], ids=["drain", "resume"])
@pytest.mark.parametrize("seed,W", SEEDS)
def test_split_form_equals_the_oracle(seed, W, drain):
    """Every tick from the model's state (the drain scenarios' own: draining records exist):
    the batch without its kinds 5 and 7, then a seeded handful of drains (resumes) at
    ts = now as its last messages."""
    scen, args, _, states = drain_run(seed, W)
    rng = np.random.default_rng(500 + seed)
    cap = len(scen["init_log"]) + ROOM
    m, o = DrainModel(W, cap), Oracle(W, cap)
    n_applied = 0
    for t, a in enumerate(args):
        st = state(scen) if t == 0 else states[t - 1]
        now, tte, kind, slot, val, ts, seq, n = a
        keep = (kind != EV_DRAIN) & (kind != EV_LEAVE)
        head = tuple(x[keep] for x in (kind, slot, val, ts, seq))
        # two slots at random (with or without a record), up to three records that are
        # draining (resumes need them) and up to three that are not
        reg = st["reg"].astype(bool)
        drn, oth = np.nonzero(reg & (st["free"] < FB_DRAIN_BELOW))[0], np.nonzero(reg & (st["free"] >= FB_DRAIN_BELOW))[0]
        tail = [int(s) for s in rng.integers(0, W, size=2)] + [int(s) for s in rng.permutation(drn)[:3]] + \
            [int(s) for s in rng.permutation(oth)[:3]]
        tail = [tail[i] for i in rng.permutation(len(tail))]
        E = len(tail)
        full = (np.concatenate([head[0], np.full(E, EV_DRAIN, np.uint8)]),
                np.concatenate([head[1], np.asarray(tail, np.int32)]),
                np.concatenate([head[2], np.full(E, 1 if drain else 0, np.int32)]),
                np.concatenate([head[3], np.full(E, now)]),
                np.concatenate([head[4], np.full(E, -1, np.int64)]))
        T = min(int(n), 50)
        m.load(st["reg"], st["free"], st["hb"], st["epoch"], st["queue"], st["log"])
        got = m.tick(now, tte, *full, T)
        exp, evicted = _split(o, st, now, tte, head, tail, drain, T)
        where = "seed %d tick %d" % (seed, t)
        np.testing.assert_array_equal(got["assign"], exp["assign"], err_msg=where)
        np.testing.assert_array_equal(got["orphans"], exp["orphans"], err_msg=where)
        np.testing.assert_array_equal(got["reconnect"][:len(head[0])], exp["reconnect"], err_msg=where)
        assert not got["reconnect"][len(head[0]):].any(), where
        # the evicted rule: a slot whose only messages were drains and that holds no record is
        # listed by the model (it got a message); the oracle never saw it
        post = m.export()
        others = set(int(s) for s in head[1])
        extra = [s for s in tail if not st["reg"][s] and not post["reg"][s] and s not in others]
        np.testing.assert_array_equal(got["evicted"], np.union1d(evicted, extra).astype(np.int32), err_msg=where)
        cmp_state(post, o.export(), where)
        was = st["free"] < FB_DRAIN_BELOW
        n_applied += sum(1 for s in set(tail) if post["reg"][s] and st["reg"][s] and
                         (post["free"][s] < FB_DRAIN_BELOW) != bool(was[s]))
    assert n_applied > 0


@pytest.mark.parametrize("name", sorted(SCRIPTED))
def test_scripted(name):
    st, now, tte, ev, n, _ = SCRIPTED[name]
    m = DrainModel(len(st["reg"]), LOG_CAP)
    m.load(st["reg"], st["free"], st["hb"], st["epoch"], st["queue"], st["log"])
    out = m.tick(now, tte, *ev, n)
    check_scripted(name, out, m.export())
    if name == "drain_queued":  # ... and later ticks hand it nothing, while its results still count
        nxt = m.tick(now + 1.0, tte, *NONE, 9)
        assert 1 not in nxt["assign"] and len(nxt["orphans"]) == 0
