"""The scenarios of tests/test_gpu_carried.py reach the cases they are there for (oracle
only, no GPU): ticks that begin with stale log entries, slots that die with orphans while
older stale entries still name them, results aimed at stale entries.  Counted over exactly
the seed sets the GPU tests use; a change to a scenario family, to the seeds or to the
aiming rule that loses the cases fails here, not silently on the GPU."""
import pytest

import carried

# seed set -> floors (ticks that begin with stale entries, scenarios with such a death,
# results aimed at stale entries).  The first row's floors are round numbers well below the
# measured values; the others lie about 15 % below what the oracle gave (beside them).
FLOORS = {
    "multitick": (150, 20, 1500),        # measured 175 / 27 / 2391  (of 240 ticks, 40 scenarios)
    "any_entry": (80, 11, 1990),         # measured  95 / 13 / 2344  (of 128 ticks, 16 scenarios)
    "window": (183, 20, 2960),           # measured 216 / 24 / 3486  (of 240 ticks, 24 scenarios)
    "window_eager": (61, 6, 935),        # measured  72 /  8 / 1100  (of  80 ticks,  8 scenarios)
    "paths": (17, 3, 1045),              # measured  20 /  4 / 1232  (of  24 ticks,  4 scenarios)
    "window_wtiles": (30, 3, 1240),      # measured  36 /  4 / 1464  (of  40 ticks,  4 scenarios)
}


def test_every_seed_set_has_floors():
    assert sorted(FLOORS) == sorted(carried.SEEDS)


@pytest.mark.parametrize("name", sorted(FLOORS))
def test_scenarios_reach_the_stale_cases(name):
    family, seeds = carried.SEEDS[name]
    ticks, scenarios, deaths, aimed = carried.coverage(family, seeds)
    print(name, "ticks %d scenarios %d (deaths %d) aimed %d" % (ticks, scenarios, deaths, aimed))
    assert (ticks >= FLOORS[name][0], scenarios >= FLOORS[name][1], aimed >= FLOORS[name][2]) == (True,) * 3, \
        (ticks, scenarios, aimed)
