"""tests/test_group_wire.py's script on a LocalShardGroup of real ShardedBalancer ranks
(world 2, every rank's context on one device), step by step against the same script on the
in-process group of model ranks: the outputs, the refusals' codes and every rank's state.
Every comparison is exact; the record of a slot that holds none (its free count, heartbeat and
epoch) is nobody's, as in tests/leave_cases.cmp_state."""
import numpy as np
import pytest

from faasbal.poolstats import diff_summary
from faasbal.sharded import LocalShardGroup
from test_group_wire import STEPS, W, WORLD, model_run, run_script, scenario

pytestmark = pytest.mark.gpu


def _same_rank(got, want, what):
    """A real rank's read-back state against the model rank's (its shard may keep dead
    entries in place, at -1, where the model drops them: compared over the global log)."""
    for k in ("base", "head"):
        assert got[k] == want[k], (what, k)
    for k in ("reg", "queue"):
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s: %s" % (what, k))
    held = np.asarray(want["reg"]) != 0
    for k in ("free", "hb", "epoch"):
        np.testing.assert_array_equal(got[k][held], want[k][held], err_msg="%s: %s" % (what, k))
    logs = []
    for st in (got, want):
        log = np.full(st["head"], -1, np.int32)
        log[np.asarray(st["log_seq"], np.int64)] = st["log"]
        logs.append(log)
    np.testing.assert_array_equal(logs[0], logs[1], err_msg=what + ": log")


def _same_result(name, got, want):
    if name in ("stats", "stats_two_edges"):
        assert not diff_summary(got, want), (name, diff_summary(got, want))
    elif name == "read":
        held = want["reg"] != 0
        for k in ("reg", "queue", "log", "head"):
            np.testing.assert_array_equal(got[k], want[k], err_msg="read: " + k)
        for k in ("free", "hb", "epoch"):
            np.testing.assert_array_equal(got[k][held], want[k][held], err_msg="read: " + k)
    elif isinstance(want, dict):
        for k, v in want.items():
            if k == "result":  # (the library's record holds more than the model's)
                assert {r: int(got[k][r]) for r in v} == {r: int(v[r]) for r in v}, (name, got[k], v)
            else:
                np.testing.assert_array_equal(got[k], v, err_msg="%s: %s" % (name, k))
    else:
        assert got == want, name


def test_script_on_real_ranks_is_the_model_groups():
    want, want_states = model_run()
    _, st = scenario()
    g = LocalShardGroup(WORLD, W, len(st["log"]) + 4096, max_events=64)
    states = []
    got = run_script(g, lambda name: states.append(None if name == "close" else [b.read_state() for b in g.bals]))
    for i, ((name, a), (_, b)) in enumerate(zip(got, want)):
        assert a[0] == b[0], (name, a, b)
        if a[0] == "error":
            # the verdict's text is the group's own; the refused bound's is the library's
            assert a[1] == b[1] and (a[2] == b[2] or name == "reclaim_refused" and "below_seq" in a[2]), (name, a, b)
        else:
            _same_result(name, a[1], b[1])
        if states[i] is not None:
            for r in range(WORLD):
                _same_rank(states[i][r], want_states[i][r], "%s: rank %d" % (name, r))
    assert [n for n, _ in got] == list(STEPS)
