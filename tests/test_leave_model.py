"""The leave model (tests/leave_model.py) pinned to the C oracle -- CPU.

The model is what the GPU tests of the goodbye message compare against, and it is trusted
only as far as these tests tie it to oracle/push_oracle.c: (a) without leaves it is the
oracle, output for output and state for state; (b) a leave that is its slot's first
message of the tick equals the oracle run on the same state with that record's heartbeat
overwritten by ts_leave - tte - 1 and the leave taken out of the batch; (c) scripted
cases with expectations written by hand.
"""
import numpy as np
import pytest

from faasbal import synth
from leave_cases import SCRIPTED, check_scripted, cmp_out, cmp_state, resolve_seq, state
from leave_model import EV_LEAVE, LeaveModel
from oracle import Oracle

ROOM = 8000


def _pair(st, cap):
    W = len(st["reg"])
    m, o = LeaveModel(W, cap), Oracle(W, cap)
    for x in (m, o):
        x.load(st["reg"], st["free"], st["hb"], st["epoch"], st["queue"], st["log"])
    return m, o


@pytest.mark.parametrize("W", [5, 37, 300])
@pytest.mark.parametrize("seed", range(16))
def test_leave_free_scenarios_equal_the_oracle(seed, W):
    scen = synth.random_scenario(seed, W=W, n_ticks=6, max_events=[20, 200][seed % 2],
                                 max_new=[50, 400][(seed // 2) % 2])
    m, o = _pair(state(scen), len(scen["init_log"]) + ROOM)
    carried = 0
    for t, tk in enumerate(scen["ticks"]):
        seq = resolve_seq(tk, o.export()["log"])
        n = carried + tk["n_new"]
        args = (tk["now"], scen["tte"], tk["ev_kind"], tk["ev_slot"], tk["ev_val"], tk["ev_ts"], seq, n)
        a, b = m.tick(*args), o.tick(*args)
        cmp_out(a, b, "tick %d" % t)
        sm, so = m.export(), o.export()
        cmp_state(sm, so, "tick %d" % t)
        for k in ("free", "hb", "epoch"):  # the whole state: the records of deleted slots too
            np.testing.assert_array_equal(sm[k], so[k], err_msg="tick %d %s (all slots)" % (t, k))
        assert sm["head"] == so["head"]
        carried = n + len(b["orphans"]) - len(b["assign"])


@pytest.mark.parametrize("W", [5, 37, 300])
@pytest.mark.parametrize("seed", range(8))
def test_leading_leaves_equal_forced_expiry_in_the_oracle(seed, W):
    """Every tick from the model's state: a seeded part of the slots has its first message
    of the tick replaced by a leave; the oracle gets the same state with hb = ts_leave -
    tte - 1 for the leaving slots that hold a record, and the batch without the leaves."""
    scen = synth.random_scenario(2000 + seed, W=W, n_ticks=6, max_events=[20, 200][seed % 2], max_new=200)
    rng = np.random.default_rng(seed)
    tte = scen["tte"]
    cap = len(scen["init_log"]) + ROOM
    m, o = _pair(state(scen), cap)
    carried, n_leaves = 0, 0
    for t, tk in enumerate(scen["ticks"]):
        kind = tk["ev_kind"].copy()
        first = {}
        for i, s in enumerate(tk["ev_slot"]):
            first.setdefault(int(s), i)
        lead = [i for s, i in first.items() if rng.random() < 0.25]
        kind[lead] = EV_LEAVE
        n_leaves += len(lead)
        st = m.export()
        seq = resolve_seq(dict(tk, ev_kind=kind), st["log"])
        n = carried + tk["n_new"]
        a = m.tick(tk["now"], tte, kind, tk["ev_slot"], tk["ev_val"], tk["ev_ts"], seq, n)
        # the oracle's side
        hb = st["hb"].copy()
        for i in lead:
            s = int(tk["ev_slot"][i])
            if st["reg"][s]:
                hb[s] = tk["ev_ts"][i] - tte - 1.0
        o.load(st["reg"], st["free"], hb, st["epoch"], st["queue"], st["log"])
        keep = kind != EV_LEAVE
        b = o.tick(tk["now"], tte, kind[keep], tk["ev_slot"][keep], tk["ev_val"][keep], tk["ev_ts"][keep], seq[keep], n)
        where = "tick %d" % t
        np.testing.assert_array_equal(a["assign"], b["assign"], err_msg=where)
        np.testing.assert_array_equal(a["orphans"], b["orphans"], err_msg=where)
        np.testing.assert_array_equal(a["reconnect"][keep], b["reconnect"], err_msg=where)
        assert not a["reconnect"][~keep].any(), where
        # the evicted rule: a slot whose only messages were leaves and that held no record is
        # listed by the model (it got a message, it holds no record); the oracle never saw it
        others = set(int(s) for s in tk["ev_slot"][keep])
        extra = [int(tk["ev_slot"][i]) for i in lead
                 if not st["reg"][int(tk["ev_slot"][i])] and int(tk["ev_slot"][i]) not in others]
        np.testing.assert_array_equal(a["evicted"], np.union1d(b["evicted"], extra).astype(np.int32), err_msg=where)
        cmp_state(m.export(), o.export(), where)
        carried = n + len(b["orphans"]) - len(b["assign"])
    assert n_leaves > 0


@pytest.mark.parametrize("name", sorted(SCRIPTED))
def test_scripted(name):
    st, now, tte, ev, n, _ = SCRIPTED[name]
    m = LeaveModel(len(st["reg"]), 64)
    m.load(st["reg"], st["free"], st["hb"], st["epoch"], st["queue"], st["log"])
    out = m.tick(now, tte, *ev, n)
    check_scripted(name, out, m.export())
    assert all(int(s) not in m.export()["queue"] for s in out["evicted"])
    if name == "queued_three_inflight":  # ... and the next tick does not hand it anything
        nxt = m.tick(now + 1.0, tte, *(np.zeros(0, d) for d in (np.uint8, np.int32, np.int32, np.float64, np.int64)), 1)
        assert list(nxt["assign"]) == [3] and len(nxt["orphans"]) == 0


def test_expired_anyway_equals_the_oracle_without_the_leave():
    st, now, tte, ev, n, _ = SCRIPTED["expired_anyway"]
    m, o = _pair(st, 64)
    a = m.tick(now, tte, *ev, n)
    b = o.tick(now, tte, [], [], [], [], np.zeros(0, np.int64), n)
    for k in ("assign", "orphans", "evicted"):
        np.testing.assert_array_equal(a[k], b[k])
    cmp_state(m.export(), o.export(), "expired")
