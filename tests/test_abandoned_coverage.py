"""The cases of tests/abandoned.py reach what they are there for (oracle only, no GPU): the
abandoned launch's results name entries that are live in the committed state, those entries
are still in flight after the committed ticks that follow, and on heartbeat contexts the
last tick redistributes every one of them.  The numbers are deterministic, so they are
stated exactly: a change to a state, a seed or a batch that loses a condition fails here,
not silently on the GPU."""
import numpy as np
import pytest

import abandoned
from faasbal import synth

# case -> (targets, results repeating one, results naming stale entries, results naming
#          another worker's entry) per abandoned launch; then, of all targets: live when
#          named, in flight after the committed ticks, orphans of the death tick
#          (None: a deque context, nobody dies)
EXPECT = {
    "h-large-one": ([2000], [200], [100], [50], 2000, 2000, 2000),
    "h-large-two": ([2000, 2000], [200, 200], [100, 100], [50, 50], 4000, 4000, 4000),
    "h-large-committed": ([2000], [200], [100], [50], 2000, 0, 0),
    "d-zipf-one": ([1000], [100], [0], [50], 1000, 1000, None),
    "d-zipf-two": ([1000, 1000], [100, 100], [0, 0], [50, 50], 2000, 2000, None),
    "d-zipf-committed": ([1000], [100], [0], [50], 1000, 0, None),
    "h-small-2-one": ([31], [7], [20], [3], 31, 31, 31),
    "h-small-2-two": ([31, 31], [7, 7], [20, 20], [3, 3], 62, 62, 62),
    "h-small-2-committed": ([31], [7], [20], [3], 31, 0, 0),
    "h-small-11-one": ([41], [10], [20], [5], 41, 41, 41),
    "h-small-11-two": ([41, 41], [10, 10], [20, 20], [5, 5], 82, 82, 82),
    "h-small-11-committed": ([41], [10], [20], [5], 41, 0, 0),
    "d-small-1-one": ([155], [38], [0], [19], 155, 155, None),
    "d-small-2-one": ([176], [44], [0], [22], 176, 176, None),
}


def test_every_case_is_stated():
    assert sorted(EXPECT) == sorted(abandoned.CASES)


@pytest.mark.parametrize("name", sorted(EXPECT))
def test_case_reaches_its_conditions(name):
    c = abandoned.case(name)
    got = ([len(t) for t in c.targets], c.n_dup, c.n_stale, c.n_foreign, c.live_named, c.in_flight_after,
           c.orphaned)
    print(name, got)
    assert got == EXPECT[name]
    # every launch fits the context the GPU test creates, and times are valid for the device
    for op, a in c.steps:
        assert len(a[2]) <= c.max_events
        assert np.all(np.diff(a[5]) >= 0) and (not len(a[5]) or a[5][-1] <= a[0])
    assert c.final["head"] <= c.log_cap


def test_h_large_is_the_state_of_the_figures():
    """The first table size past the deferred clears, every entry live; the first tick's
    figures; a device that left the 2000 entries completed reports 2000 orphans fewer."""
    c = abandoned.case("h-large-one")
    assert len(c.st["reg"]) == (1 << 17) + 5 and len(c.st["log"]) == 954_495 and (c.st["log"] >= 0).all()
    w = c.want[0]
    assert (len(w["assign"]), len(w["orphans"]), len(w["evicted"])) == (52_100, 48_004, 6_554)
    assert [op for op, _ in c.steps] == ["tick", "abandon", "tick", "tick", "tick"]
    assert len(c.want[c.death]["orphans"]) == 960_214
    assert len(c.steps) <= 5 and len(abandoned.case("h-large-two").steps) <= 5


def test_stale_names_reach_the_liveness_test():
    """The stale names of a heartbeat case: entries a committed tick redistributed (the
    oracle cleared them, the device's log still holds them) of slots that have no record
    (they register in the batch first) or re-registered past the entry."""
    for name in ("h-large-one", "h-small-2-one", "h-small-11-one"):
        c = abandoned.case(name)
        i = [op for op, _ in c.steps].index("abandon")
        _now, _tte, kind, slot, _val, _ts, seq, _n = c.steps[i][1]
        run = c.run()
        for op, a in c.steps[:i]:
            run.tick(a)
        ex = run.export()
        stale = {(s, q) for s, qs in run.stale.items() for q in qs}
        named = [(int(s), int(q)) for k, s, q in zip(kind, slot, seq) if k == synth.EV_RESULT and (int(s), int(q)) in stale]
        assert len(named) == c.n_stale[0]
        assert all(ex["log"][q] == -1 and (not ex["reg"][s] or q < ex["epoch"][s]) for s, q in named)
