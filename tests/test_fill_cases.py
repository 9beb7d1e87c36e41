"""Every case of tests/fill_cases.py sits on the seam it names -- checked without a GPU
against the C oracle and the numpy water-fill (S(r) = sum min(c, r)): the oracle dispatches
the intended number of tasks, the fill level is the intended one with a partial round L, and
the launch's table follows from choose_R of what the host can know at launch.

The second half runs the closed form the kernels share (csrc/faasbal_fill.h: fill_demand,
fill_verdict, fill_next) on the same cases through tests/fill_probe.cpp, compiled here: the
fill level, the partial round and the rerun verdict against water_fill and the case's own
figures, every position's next state against the C oracle's assignments and next queue."""
import os
import shutil
import subprocess

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


# ---------------------------------------------------------------------------------------
# csrc/faasbal_fill.h on the CPU

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
BIG = 1 << 40


@pytest.fixture(scope="module")
def fill_probe(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.fail("hipcc not found: the fill probe cannot be compiled")
    exe = str(tmp_path_factory.mktemp("fill") / "fill_probe")
    subprocess.run(["hipcc", "-std=c++17", "-O1", "-I" + os.path.join(REPO, "distributed-faas_amd", "csrc"),
                    os.path.join(HERE, "fill_probe.cpp"), "-o", exe], check=True)

    def ask(c, R, T, O=0, redist=1, head=0, log_cap=BIG, timeout=20):
        """One tick over the logical queue c (LRU order) with a table of R rows."""
        c = np.asarray(c, np.int64)
        maxc = int(c.max()) if len(c) else 0
        rlim = min(maxc, R)
        A = (c[None, :] > np.arange(rlim)[:, None]).sum(1)  # the table: A(r) = positions with c > r
        words = [R, maxc, int(c.sum()), O, T, redist, head, log_cap, rlim, *A, len(c), *c]
        # (a time limit: a probe that never ends fails its test instead of stalling the run)
        out = subprocess.run([exe], input=" ".join(str(int(w)) for w in words) + "\n", capture_output=True, text=True,
                             check=True, timeout=timeout).stdout
        a = dict(w.split("=", 1) for w in out.split())
        assert "error" not in a, out
        nxt = a.pop("next", "")
        a = {k: int(v) for k, v in a.items()}
        a["next"] = np.array([int(x) for x in nxt.split(",") if x], np.int64)
        return a

    return ask


def _logical_queue(case):
    """The positions the emission ranks, in LRU order: the slots and their c.  A register
    message moves its worker to the front (the last message first); the position it held
    is empty."""
    st, (kind, slot) = case["st"], case["ev"][:2]
    front = slot[kind == fc.EV_REGISTER][::-1].astype(np.int64)
    lq = np.concatenate([front, st["queue"].astype(np.int64)])
    c = case["c"][lq].copy()
    c[len(front):][np.isin(st["queue"], front)] = 0
    return lq, c


def _oracle_tick(case):
    st = case["st"]
    o = Oracle(len(st["reg"]), case["log_cap"])
    o.load(st["reg"], st["free"], st["hb"], st["epoch"], st["queue"], st["log"])
    out = o.tick(*fc.tick_args(case))
    return out["assign"], o.export()["queue"]


def _exact(a, lq, c, n, assign, next_queue):
    """A tick without a status: the level and the partial round are water_fill's, the
    positions' next states the oracle's."""
    L, S_L, A_L, n_eff = fc.water_fill(c, n)
    assert (a["status"], a["L"], a["S_L"], a["AL"], a["N_eff"], a["p"]) == (0, L, S_L, A_L, n_eff, n_eff - S_L), a
    assert a["ok"] and a["served"] == len(assign) == n_eff and a["partial"] == a["p"]
    # the one position of rank p in A_L reports the queue length; nobody when every worker is saturated
    assert (a["setters"], a["qlen"]) == ((1, len(next_queue)) if A_L else (0, -1)), a
    assert np.array_equal(lq[a["next"]], next_queue)


def _check_fill(ask, case, L, R_first=None):
    """The case at its first table (status 1 exactly where the case says it reruns or fails),
    then, rerun, at the table of the largest count."""
    lq, c = _logical_queue(case)
    n = case["T"] + case["n_orph"]
    R = R_first or case["R_launch"]
    head = len(case["st"]["log"])
    rerun = case["maxc"] > R and L >= R - 1 if R_first else case["reruns"] or case["erange"]
    a = ask(c, R, case["T"], O=case["n_orph"], head=head, log_cap=case["log_cap"])
    assert a["status"] == int(rerun) and a["rlim"] == min(case["maxc"], R), a
    if rerun:
        if R >= ROW_LIMIT:
            assert case["erange"]
            return
        a = ask(c, choose_R(case["maxc"]), case["T"], O=case["n_orph"], head=head, log_cap=case["log_cap"])
        if case["erange"]:  # the widest table is still too narrow
            assert a["status"] == 1
            return
    assert a["L"] == L == case["L"]
    _exact(a, lq, c, n, *_oracle_tick(case))


@pytest.mark.parametrize("L", fc.KNOWN_LEVELS)
def test_fill_known_levels(fill_probe, L):
    _check_fill(fill_probe, fc.known_case(L), L)


@pytest.mark.parametrize("way,batch", [("result", "host"), ("register", "pinned"), ("load", "host"),
                                       ("register", "host")])
def test_fill_wide_cases(fill_probe, way, batch):
    for R, L, maxc in fc.wide_cases(way):
        case = fc.wide_case(R, L, maxc, way, batch)
        assert case["reruns"] == (L >= R - 1 and case["R_launch"] == R)
        _check_fill(fill_probe, case, L)


@pytest.mark.parametrize("maxc", fc.LIMIT_MAXC)
def test_fill_limit_cases(fill_probe, maxc):
    for way in ("load", "register"):
        for L in (5, ROW_LIMIT - 2, ROW_LIMIT - 1):
            _check_fill(fill_probe, fc.limit_case(L, maxc, way), L)


def test_fill_shard_cases(fill_probe):
    """The first table is the one the caller's stale hint states (fb_set_round_hint)."""
    for R, maxc in fc.SHARD_FIRST:
        for L in (R - 2, R - 1):
            _check_fill(fill_probe, fc.shard_case(L, R, maxc), L, R_first=R)
    for L in fc.SHARD_WIDE_LEVELS + (ROW_LIMIT - 1,):
        _check_fill(fill_probe, fc.shard_case(L, 128 if L >= 127 else 64 if L >= 63 else 32, fc.SHARD_WIDE_MAXC[0]), L,
                    R_first=128)


def _hand(ask, c, T, R, **kw):
    """A queue of len(c) live workers 0 .. len(c) - 1 with free counts c and an empty log."""
    c = np.asarray(c, np.int64)
    W = len(c)
    o = Oracle(W, BIG >> 20)
    o.load(np.ones(W, np.uint8), c.astype(np.int32), np.full(W, 999.0), np.zeros(W, np.uint32),
           np.arange(W, dtype=np.int32), np.zeros(0, np.int32))
    z = np.zeros(0)
    out = o.tick(fc.NOW, fc.TTE, z.astype(np.uint8), z.astype(np.int32), z.astype(np.int32), z, z.astype(np.int64), T)
    a = ask(c, R, T, **kw)
    return a, (np.arange(W), c, T, out["assign"], o.export()["queue"])


@pytest.mark.parametrize("maxc", [32, 33])
@pytest.mark.parametrize("L", [30, 31])
def test_fill_hand_edge_of_32_rows(fill_probe, L, maxc):
    """The smallest table at its edge: with max c = R the level is exact up to R - 1; one
    worker beyond the table and L = R - 1 needs a 64-row table, L = R - 2 does not."""
    c = [maxc] * 5 + [2, 40 if maxc > 32 else 31, 1]
    T = int(np.minimum(c, L).sum()) + 2
    a, ref = _hand(fill_probe, c, T, 32)
    assert a["status"] == int(max(c) > 32 and L == 31)
    if a["status"]:
        a, ref = _hand(fill_probe, c, T, 64)
    assert a["L"] == L and a["p"] == 2
    _exact(a, *ref)


def test_fill_hand_small_cases(fill_probe):
    c = [3, 1, 2, 5]
    # no task: level 0, everybody keeps their place
    a, ref = _hand(fill_probe, c, 0, 32)
    assert (a["L"], a["p"], a["N_eff"], list(a["next"])) == (0, 0, 0, [0, 1, 2, 3])
    _exact(a, *ref)
    # more tasks than capacity: every worker saturated, nobody of rank p, an empty next queue
    a, ref = _hand(fill_probe, c, 100, 32)
    assert (a["N_eff"], a["L"], a["AL"], a["setters"], len(a["next"])) == (11, 5, 0, 0, 0)
    _exact(a, ref[0], ref[1], 100, *ref[3:])
    # exactly the capacity, and exactly a whole number of rounds (p = 0: round L unserved)
    for T in (11, 4, 7):
        a, ref = _hand(fill_probe, c, T, 32)
        _exact(a, *ref)
    # the log: full to its last entry is fine, one more is status 2 -- behind status 1
    assert fill_probe(c, 32, 6, head=10, log_cap=16)["status"] == 0
    assert fill_probe(c, 32, 6, head=10, log_cap=15)["status"] == 2
    assert fill_probe([40] * 4, 32, 4 * 31 + 1, head=10, log_cap=15)["status"] == 1
    # a purge-only tick reports its orphans and dispatches none; otherwise they come first
    assert fill_probe(c, 32, 0, O=7, redist=0)["N_eff"] == 0
    assert fill_probe(c, 32, 1, O=7)["N_eff"] == 8
