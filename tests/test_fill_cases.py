"""Every case of tests/fill_cases.py sits on the seam it names -- checked without a GPU
against the C oracle and the numpy water-fill (S(r) = sum min(c, r)): the oracle dispatches
the intended number of tasks, the fill level is the intended one with a partial round L, and
the launch's table follows from choose_R of what the host can know at launch."""
import numpy as np
import pytest

import fill_cases as fc
from oracle import DequeOracle, Oracle
from plan_cases import ROW_LIMIT, choose_R


def _check(case, L, deque=False):
    st = case["st"]
    W = len(st["reg"])
    o = (DequeOracle if deque else Oracle)(W, case["log_cap"])
    o.load(st["reg"], st["free"], st["hb"], st["epoch"], st["queue"], st["log"])
    out = o.tick(*fc.tick_args(case))
    n = case["T"] + len(out["orphans"])
    assert len(out["orphans"]) == case["n_orph"]
    assert len(out["assign"]) == n  # capacity is never the limit: round L + 1 is populated
    got_L, S_L, A_L, n_eff = fc.water_fill(case["c"], n)
    assert (got_L, n_eff) == (L, n) and case["L"] == L
    assert 0 < n - S_L < A_L or (A_L < 3 and n == S_L)  # round L is partial
    # the population: most workers beyond L + 1, some poor, some expired, three queue blocks
    c = case["c"]
    assert (c > L + 1).sum() > 0.7 * W or case["maxc"] > c[c > 0].min() >= 1
    assert ((c >= 1) & (c <= 3)).sum() >= 1
    if not deque:
        assert (c == 0).sum() >= 1 and case["n_orph"] >= 8
    # every served worker's count after the tick, from the closed form
    po = o.export()
    live = c > 0
    served = np.bincount(out["assign"], minlength=W)
    assert np.all(served[live] >= np.minimum(c, L)[live]) and np.all(served[live] <= np.minimum(c, L + 1)[live])
    assert po["head"] == len(st["log"]) + n
    return out


@pytest.mark.parametrize("L", fc.KNOWN_LEVELS)
def test_known_levels(L):
    case = fc.known_case(L)
    _check(case, L)
    assert len(case["st"]["queue"]) > 2 * fc.BLOCK
    assert case["maxc"] <= case["R_launch"] == choose_R(L + 2) and not case["reruns"] and not case["erange"]
    if L in fc.DEQUE_LEVELS:
        _check(fc.known_case(L, expire=False), L, deque=True)


def test_unfused_case():
    case = fc.known_case(126, W=fc.UNFUSED_W)
    _check(case, 126)
    nbq = -(-len(case["st"]["queue"]) // fc.BLOCK)
    assert case["R_launch"] == 128 and nbq * 128 > 16 * fc.BLOCK * 4  # kTabLd * kBS * 4


@pytest.mark.parametrize("way,batch", [("result", "host"), ("register", "pinned"), ("register", "device"),
                                       ("register", "host")])
def test_wide_cases(way, batch):
    for R, L, maxc in fc.wide_cases(way):
        case = fc.wide_case(R, L, maxc, way, batch)
        _check(case, L)
        assert case["maxc"] == maxc
        if batch == "host" and way == "register":  # the host saw the value: the table is known
            assert case["R_launch"] == choose_R(maxc) and not case["reruns"]
            continue
        assert case["R_launch"] == R
        assert case["reruns"] == (L >= R - 1) and not case["erange"]


@pytest.mark.parametrize("way", ["load", "register"])
@pytest.mark.parametrize("maxc", fc.LIMIT_MAXC)
def test_limit_cases(maxc, way):
    for L in (5, ROW_LIMIT - 2, ROW_LIMIT - 1):
        case = fc.limit_case(L, maxc, way)
        _check(case, L)
        assert case["maxc"] == maxc and case["erange"] == (L == ROW_LIMIT - 1)
        assert case["R_launch"] <= ROW_LIMIT
        # no table beyond limit x nbq rows, whichever way the count arrives
        assert choose_R(case["maxc"]) == ROW_LIMIT


def test_shard_cases():
    for R, maxc in fc.SHARD_FIRST:
        for L in (R - 2, R - 1):
            case = fc.shard_case(L, R, maxc)
            _check(case, L)
            assert case["maxc"] == maxc > R
    for L in fc.SHARD_WIDE_LEVELS + (ROW_LIMIT - 1,):
        for maxc in fc.SHARD_WIDE_MAXC[:1] if L > 200 else fc.SHARD_WIDE_MAXC:
            case = fc.shard_case(L, 128 if L >= 127 else 64 if L >= 63 else 32, maxc)
            _check(case, L)
            assert case["erange"] == (L == ROW_LIMIT - 1)


def test_large_queue_and_window_cases():
    """The sharded cases of more than 256 queue blocks and the window-mode case (in one tick here; the
    GPU test runs a small window tick first)."""
    W = 257 * fc.BLOCK + 5
    for L in (30, 31):
        case = fc.shard_case(L, 32, 33, W=W)
        _check(case, L)
        assert case["maxc"] == 33 and -(-len(case["st"]["queue"]) // fc.BLOCK) > 256
        case = fc.fill_case(L, cap0=32, maxc=33, way="load", W=20000, seed=5)
        _check(case, L)
        assert case["maxc"] == 33 and case["R_launch"] == 64  # (the GPU test states a stale hint of 32)
