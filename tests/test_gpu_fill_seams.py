"""Fill levels at every seam of the round table, bit-exact against the oracle.

The water-filling closed form (fill level L, partial round A(L), prefixes S(r)) is stated once,
in csrc/faasbal_fill.h -- fill_verdict carries the edge rule `maxc > R && L >= R - 1` (a table
of R rows is exact while L + 2 rows fit) -- and the seven emissions below call it, each
finding L in the round table its own way (fill_scan in wave registers; k_emit and
k_emit_shard_wide their own search).  tests/fill_cases.py builds one tick per seam and
tests/test_fill_cases.py proves on the CPU that it sits there and that the closed form gives
the oracle's tick; here each runs on the GPU and
its outputs, result record (fill_level, max_free, reruns, n_assigned) and committed state
must equal the oracle's.  fb_timing_read's launch counts say which emission ran ("plan"
beside "emit": k_plan / k_plan2 ahead of it; "scan2": the sharded recount).

  implementation            exact side (L = R - 2)                     rerun side (L = R - 1)
  k_plan2 (+ k_emit2)       known[126] plan=1 gp=0; wide[plan1_gp0]    wide[plan1_gp0]
  emit2_rounds, fused       known[126] auto; wide[default, logscan]    wide[default, logscan, ev_ll0]
  emit2_rounds, gp          known[126] plan=1 gp=1; unfused R = 128    wide[plan1_gp1]
  k_plan + chunked k_emit   known[254, 510, 1022] auto; plan=2 every   wide[plan2]; limit[4095]: FB_ERANGE
                            level; limit[4094]
  k_emit_shard (rows)       shard_first[L = R - 2]                     shard_first[L = R - 1]: FB_ERERUN
  k_emit_shard_wide         shard_wide[4094]                           shard_limit[4095]: FB_ERANGE
  k_emit_shard_xp           large_queue[xplan 1, L = 30]                large_queue[xplan 1, L = 31]: FB_ERERUN
  k_emit_shard (recount)    large_queue[xplan 0, L = 30]                large_queue[xplan 0, L = 31]: FB_ERERUN
  window tick's fallback    beyond_a_window_tick[30]: a window tick that never saw the wide workers, then the
                            general tick at L = R - 2 / [31] at R - 1 (a window tick itself ends at level 0:
                            any level above it reruns as a general tick, tests/test_gpu_window.py)

The whole file: 200 tests, 6 s on an MI355X (the slowest, the first to load the library, 0.25 s).
"""
import numpy as np
import pytest

import fill_cases as fc
from faasbal import FaasbalError, GpuBalancer
from faasbal._lib import FB_ERANGE, FB_ERERUN
from oracle import DequeOracle, Oracle
from plan_cases import ROW_LIMIT, choose_R

pytestmark = pytest.mark.gpu
R_FUSED = 128
OUT_KEYS = ("reconnect", "assign", "orphans", "evicted")


def _ctx(W, log_cap, paths=None, deque=False):
    import torch  # noqa: F401  (loads the HIP runtime before libfaasbal)
    g = GpuBalancer(W, log_cap, max_events=64, mode="deque" if deque else "heartbeat")
    for k, v in (paths or {}).items():
        g.set_path(k, v)
    g.timing_enable(True)
    return g


def _load(g, case, deque=False):
    st = case["st"]
    g.load(st)
    o = (DequeOracle if deque else Oracle)(len(st["reg"]), g.max_log)
    o.load(st["reg"], st["free"], st["hb"], st["epoch"], st["queue"], st["log"])
    return o


def _launch(g, case, batch="host"):
    k, s, v, ts, q = case["ev"]
    g.timing_read()
    if batch == "host" or not len(k):
        g.launch(fc.NOW, fc.TTE, k, s, v, ts, q, case["T"])
        return
    if batch == "pinned":
        g._held = g.pin_events(k, s, v, ts, q)
        g.stage(fc.NOW, *g._held)
    else:
        import torch
        g._held = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (k, s, v, ts, q)]
        g.stage_device(fc.NOW, *g._held)
    g.launch_staged(fc.TTE, case["T"])


def _outputs(g, res):
    return dict(result=res, reconnect=g.event_status(), assign=g.assignments(), orphans=g.orphans(),
                evicted=g.evicted())


def _cmp_state(g, o, where, deque=False):
    sg, so = g.read_state(), o.export()
    np.testing.assert_array_equal(sg["reg"], so["reg"], err_msg="%s reg" % (where,))
    reg = so["reg"].astype(bool)
    for k in ("free", "hb") if deque else ("free", "hb", "epoch"):
        np.testing.assert_array_equal(sg[k][reg], so[k][reg], err_msg="%s %s" % (where, k))
    np.testing.assert_array_equal(sg["queue"], so["queue"], err_msg="%s queue" % (where,))
    np.testing.assert_array_equal(sg["log"], so["log"], err_msg="%s log" % (where,))


def _cmp_tick(g, o, case, out, where, deque=False):
    b = o.tick(*fc.tick_args(case))
    for k in OUT_KEYS:
        np.testing.assert_array_equal(out[k], b[k], err_msg="%s: %s" % (where, k))
    r = out["result"]
    assert r["fill_level"] == case["L"] and r["max_free"] == case["maxc"], (where, r)
    assert r["n_assigned"] == len(b["assign"]) and r["n_orphans"] == len(b["orphans"]), (where, r)
    assert (r["reruns"] >= 1) == case["reruns"], (where, r)
    _cmp_state(g, o, where, deque)


def _plan_launched(R, paths, deque=False):
    """Whether a one-GPU tick of R rows launches k_plan / k_plan2 ahead of its emission (small
    queues: the fused tick otherwise; plan_tick, tests/test_plan.py)."""
    plan = (paths or {}).get("plan", 0)
    if plan == 2 or R > R_FUSED:
        return True  # k_plan + the chunked k_emit
    return plan == 1 and ((paths or {}).get("gp", 1) == 0 or deque)  # k_plan2 + k_emit2


def _check_launches(g, case, res, paths, where, deque=False):
    """The emissions this tick was meant for ran: one per launch, with or without a plan."""
    got = {k: int(v[1]) for k, v in g.timing_read().items()}
    tables = [case["R_launch"]] + ([choose_R(case["maxc"])] if case["reruns"] else [])
    assert res["reruns"] == len(tables) - 1, (where, res)
    assert got.get("emit", 0) == len(tables) and got.get("scan", 0) == len(tables), (where, got)
    assert got.get("plan", 0) == sum(_plan_launched(R, paths, deque) for R in tables), (where, got, tables)


def _one_tick(g, case, batch, paths, where, deque=False):
    o = _load(g, case, deque)
    _launch(g, case, batch)
    res = g.wait()
    out = _outputs(g, res)
    g.commit()
    _check_launches(g, case, res, paths, where, deque)
    _cmp_tick(g, o, case, out, where, deque)
    return o


# ---------------------------------------------------------------------------------------
# a. the table known at launch (maxc <= R)
KNOWN_PATHS = {"auto": {}, "plan1_gp0": {"plan": 1, "gp": 0}, "plan1_gp1": {"plan": 1, "gp": 1}, "plan2": {"plan": 2}}


@pytest.fixture(scope="module")
def known_cases():
    return {L: fc.known_case(L) for L in fc.KNOWN_LEVELS}


# (plan=1 only where a k_emit2 path exists: tables of at most 128 rows)
KNOWN = [(L, p) for L in fc.KNOWN_LEVELS for p in KNOWN_PATHS if not p.startswith("plan1") or choose_R(L + 2) <= R_FUSED]


@pytest.mark.parametrize("L,path", KNOWN)
def test_known_table_levels(known_cases, L, path):
    """L + 2 <= R with the largest free count known at launch: the fused k_emit2 up to 128 rows
    (126 = R - 2), k_plan2 + k_emit2 and the group-row k_emit2 under plan=1 (R <= 128 only:
    wider tables have no such path), the chunked k_emit from 256 rows by itself and under
    plan=2 at every level."""
    case, paths = known_cases[L], KNOWN_PATHS[path]
    g = _ctx(len(case["st"]["reg"]), case["log_cap"], paths)
    try:
        _one_tick(g, case, "host", paths, (L, path))
    finally:
        g.close()


@pytest.mark.parametrize("L", fc.DEQUE_LEVELS)
def test_known_table_levels_deque(L):
    case = fc.known_case(L, expire=False)
    g = _ctx(len(case["st"]["reg"]), case["log_cap"], deque=True)
    try:
        _one_tick(g, case, "host", {}, (L, "deque"), deque=True)
    finally:
        g.close()


def test_unfused_128_rows_without_forcing():
    """A queue of more than 128 blocks: the 128-row table is too large for the fused tick
    (tests/test_plan.py holds plan_tick to fused = 0 at this shape), L = R - 2."""
    case = fc.known_case(126, W=fc.UNFUSED_W)
    g = _ctx(fc.UNFUSED_W, case["log_cap"])
    try:
        _one_tick(g, case, "host", {}, "unfused")
    finally:
        g.close()


# ---------------------------------------------------------------------------------------
# b. a worker wider than the launch's table
WIDE_PATHS = {"default": {}, "ev_ll0": {"ev_ll": 0}, "plan1_gp0": {"plan": 1, "gp": 0},
              "plan1_gp1": {"plan": 1, "gp": 1}, "plan2": {"plan": 2}, "logscan": {"logscan": 1}}
WIDE_WAYS = [("result", "host"), ("register", "pinned"), ("register", "device")]
# (a device-resident batch needs the linked-list grouping: ev_ll=0 refuses it)
WIDE = [(R, w, b, p) for R in fc.WIDE_TABLES for w, b in WIDE_WAYS for p in WIDE_PATHS
        if not (b == "device" and p == "ev_ll0")]


@pytest.mark.parametrize("R,way,batch,path", WIDE)
def test_wider_than_the_launch_table(R, way, batch, path):
    """maxc > R unknown to the host at launch (a result on a worker that held R; a register in
    a batch the device checks: pinned, device-resident): exact without a rerun up to
    L = R - 2 (capacity beyond the table unknown), rerun wider and exact from L = R - 1."""
    paths = WIDE_PATHS[path]
    ll = paths.get("ev_ll", 1) == 1  # (ev_ll=0: the host checks pinned batches too and sees the value)
    cases = [fc.wide_case(R, L, m, way, batch, device_checked=ll) for r, L, m in fc.wide_cases(way) if r == R]
    g = _ctx(600, max(c["log_cap"] for c in cases), paths)
    try:
        for case in cases:
            if ll or way == "result":
                assert case["R_launch"] == R and case["reruns"] == (case["L"] >= R - 1)
            _one_tick(g, case, batch, paths, (R, case["L"], case["maxc"], way, batch, path))
    finally:
        g.close()


@pytest.mark.parametrize("L", [30, 31])
def test_wide_worker_beyond_a_window_tick(L):
    """Window mode: workers of 33 free processes sit at the queue's tail under a stale hint of
    32 (fb_set_round_hint); a window tick scans a prefix only and never sees them (its max_free
    stays at most 32, and so does the next launch's table); the general tick that follows
    reaches them at L = R - 2 without a rerun and at L = R - 1 with one."""
    R, W = 32, 20000
    case = fc.fill_case(L, cap0=R, maxc=R + 1, way="load", W=W, seed=5)
    st = dict(case["st"])
    q = st["queue"]
    st["queue"] = np.concatenate([q[~np.isin(q, case["wide"])], case["wide"].astype(np.int32)])
    beat = st["queue"][:40][st["hb"][st["queue"][:40]] > 990.0][:5]  # (a window tick needs messages)
    ev = (np.full(5, 2, np.uint8), beat.astype(np.int32), np.zeros(5, np.int32), np.linspace(999.1, 999.9, 5),
          np.full(5, -1, np.int64))
    first = dict(case, st=st, T=100, ev=ev)
    g = _ctx(W, case["log_cap"] + 4096)
    try:
        g.set_window(1)
        o = _load(g, first)
        g._chk(g.lib.fb_set_round_hint(g.h, R))
        _launch(g, first)
        res = g.wait()
        out = _outputs(g, res)
        g.commit()
        assert g.window_stats() == (1, 0) and res["fill_level"] == 0 and res["max_free"] <= R, (res, g.window_stats())
        b = o.tick(*fc.tick_args(first))
        for k in OUT_KEYS:
            np.testing.assert_array_equal(out[k], b[k], err_msg="window tick: %s" % k)
        # the general tick: T from the committed queue (the oracle's), round L served to a third
        so = o.export()
        c = np.maximum(so["free"][so["queue"]].astype(np.int64), 1)
        T = int(np.minimum(c, L).sum()) + int((c > L).sum()) // 3
        assert fc.water_fill(c, T)[0] == L and int(c.max()) == R + 1
        args = (fc.NOW + 0.5, fc.TTE, [], [], [], [], [], T)
        g.timing_read()
        a, b = g.tick(*args), o.tick(*args)
        for k in OUT_KEYS:
            np.testing.assert_array_equal(a[k], b[k], err_msg="general tick: %s" % k)
        r = a["result"]
        assert (r["fill_level"], r["max_free"], r["reruns"]) == (L, R + 1, int(L >= R - 1)), r
        got = {k: int(v[1]) for k, v in g.timing_read().items()}
        assert got.get("emit", 0) == 1 + r["reruns"] and "plan" not in got, got
        _cmp_state(g, o, ("window", L))
    finally:
        g.close()


# ---------------------------------------------------------------------------------------
# c. the byte of the compact form
@pytest.mark.parametrize("mode", ["compact", "compact_out"])
@pytest.mark.parametrize("rounds", [254, 255, 256])
def test_compact_form_at_the_byte(known_cases, rounds, mode):
    """c = min(c, L + 1) as a byte: exact up to L + 1 = 255; at 256 the compact readback and
    its expansion are refused with FB_ERANGE, fb_get_outputs is still exact, the tick commits
    and the next one is exact."""
    L = rounds - 1
    case = known_cases[L]
    W = len(case["st"]["reg"])
    g = _ctx(W, case["log_cap"] + 2000)
    try:
        if mode == "compact":
            g.set_compact(True)
            bufs = (np.zeros(W + 16, np.int32), np.zeros(W + 16, np.uint8), np.zeros(g.max_log, np.int64),
                    np.zeros(W, np.int32))
        else:
            bufs = g._compact_out()
        o = _load(g, case)
        _launch(g, case)
        res = g.wait()
        b = o.tick(*fc.tick_args(case))
        assert res["fill_level"] == L and res["n_assigned"] == len(b["assign"])
        if rounds <= 255:
            sl, cc, orph, ev = g.outputs_compact(*bufs)
            assert int(cc.max()) == rounds
            got = g.expand(sl, cc)
            np.testing.assert_array_equal(got, g.assignments())
            np.testing.assert_array_equal(got, b["assign"])
            np.testing.assert_array_equal(orph, b["orphans"])
            np.testing.assert_array_equal(ev, b["evicted"])
        else:
            with pytest.raises(FaasbalError) as e:
                g.outputs_compact(*bufs)
            assert e.value.code == FB_ERANGE and "rounds beyond a byte, read fb_get_outputs" in str(e.value)
            with pytest.raises(FaasbalError) as e:
                g.expand(bufs[0][:W], bufs[1][:W])
            assert e.value.code == FB_ERANGE and "beyond the compact form" in str(e.value)
            a, orph, ev = g.outputs(np.zeros(res["n_assigned"], np.int32), np.zeros(max(res["n_orphans"], 1), np.int64),
                                    np.zeros(W, np.int32))
            np.testing.assert_array_equal(a, b["assign"])
            np.testing.assert_array_equal(orph, b["orphans"])
            np.testing.assert_array_equal(ev, b["evicted"])
        g.commit()
        _cmp_state(g, o, (rounds, mode))
        args = (fc.NOW + 1.0, fc.TTE, [], [], [], [], [], 1000)
        a2, b2 = g.tick(*args), o.tick(*args)
        for k in OUT_KEYS:
            np.testing.assert_array_equal(a2[k], b2[k], err_msg="next tick: %s" % k)
        _cmp_state(g, o, (rounds, mode, "next"))
    finally:
        g.close()


# ---------------------------------------------------------------------------------------
# d. the one-GPU row limit
@pytest.mark.parametrize("way", ["load", "register"])
@pytest.mark.parametrize("maxc", fc.LIMIT_MAXC)
def test_row_limit(maxc, way):
    """Free counts far beyond the widest table (ROW_LIMIT rows), loaded or registered: exact at
    a small fill level and at L = limit - 2; at L = limit - 1 the wait fails with FB_ERANGE,
    nothing is committed, and the next, smaller tick is exact."""
    cases = {L: fc.limit_case(L, maxc, way) for L in (5, ROW_LIMIT - 2, ROW_LIMIT - 1)}
    g = _ctx(fc.LIMIT_W, max(c["log_cap"] for c in cases.values()))
    try:
        for L in (5, ROW_LIMIT - 2):
            assert cases[L]["R_launch"] <= ROW_LIMIT and not cases[L]["erange"]
            _one_tick(g, cases[L], "host", {}, (maxc, way, L))
        case = cases[ROW_LIMIT - 1]
        assert case["erange"]
        o = _load(g, case)
        before = g.read_state()
        _launch(g, case)
        with pytest.raises(FaasbalError) as e:
            g.wait()
        assert e.value.code == FB_ERANGE, e.value
        after = g.read_state()
        for k in before:
            np.testing.assert_array_equal(before[k], after[k], err_msg="after FB_ERANGE: %s" % k)
        _cmp_state(g, o, "after FB_ERANGE")
        args = (fc.NOW, fc.TTE, [], [], [], [], [], 100)
        a, b = g.tick(*args), o.tick(*args)
        for k in OUT_KEYS:
            np.testing.assert_array_equal(a[k], b[k], err_msg="after FB_ERANGE, next tick: %s" % k)
        assert a["result"]["max_free"] == (maxc if way == "load" else case["st"]["free"].max())
        _cmp_state(g, o, "after FB_ERANGE, next tick")
    finally:
        g.close()


# ---------------------------------------------------------------------------------------
# e. sharded
SHARD_KNOBS = [(1, 1), (0, 1), (1, 0), (0, 0)]


def _shard_group(world, log_cap, xplan, xself, W=600):
    import torch  # noqa: F401
    from faasbal.sharded import ShardedBalancer
    bals = [ShardedBalancer(r, world, W, log_cap, max_events=64) for r in range(world)]
    for b in bals:
        b.set_path("xplan", xplan)
        b.set_path("xself", xself)
    bals[0].timing_enable(True)
    return bals


def _shard_load(bals, case, R_first):
    st = case["st"]
    for b in bals:
        b.load(st)
        b._chk(b.lib.fb_set_round_hint(b.h, R_first))  # the table of the first launch, on every rank alike
    o = Oracle(len(st["reg"]), bals[0].max_log)
    o.load(st["reg"], st["free"], st["hb"], st["epoch"], st["queue"], st["log"])
    return o


def _shard_attempt(bals, args):
    """One launch of the group (the exchange summed on the device): (results, error codes)."""
    import torch
    bals[0].timing_read()
    for b in bals:
        b.launch(*args)
    torch.cuda.synchronize()
    total = bals[0].exchange().clone()
    for b in bals[1:]:
        total += b.exchange()
    for b in bals:
        b.exchange().copy_(total)
    torch.cuda.synchronize()
    for b in bals:
        b.cont()
    res, codes = [], []
    for b in bals:
        try:
            res.append(b.wait())
        except FaasbalError as e:
            codes.append(e.code)
    return res, codes, {k: int(v[1]) for k, v in bals[0].timing_read().items()}


def _shard_finish(bals, o, res, args, where):
    from faasbal.sharded import merge_outputs
    from test_gpu_sharded import _cmp_outputs, _cmp_state as _cmp_shard_state
    for k in ("n_assigned", "n_orphans", "queue_len", "log_head", "fill_level", "max_free"):
        assert len({r[k] for r in res}) == 1, (where, k)
    outs = []
    for b in bals:
        task, slot = b.local_assignments()
        outs.append(dict(task=task, slot=slot, orphans=b.orphans(), evicted=b.evicted(), reconnect=b.event_status()))
    merged = merge_outputs(outs, res[0]["n_assigned"])
    for b in bals:
        b.commit()
    _cmp_outputs(merged, o.tick(*args), 0)
    _cmp_shard_state(bals, o, 0)


def _shard_tick(bals, case, R_first, where):
    """The case on the group: FB_ERERUN on every rank alike exactly when L >= R - 1 under a
    wider worker, the relaunch with the table of the largest free count; then exact."""
    o = _shard_load(bals, case, R_first)
    args = fc.tick_args(case)
    world = len(bals)
    relaunch = case["maxc"] > R_first and case["L"] >= R_first - 1
    res, codes, got = _shard_attempt(bals, args)
    if relaunch:
        assert codes == [FB_ERERUN] * world and not res, (where, codes)
        assert "plan" not in got and "scan2" not in got, (where, got)  # k_emit_shard on the exchanged rows
        res, codes, got = _shard_attempt(bals, args)
        wide = choose_R(case["maxc"]) > R_FUSED
        # two-byte counts, the recount, k_plan and k_emit_shard_wide -- or a table that still has <= 128 rows
        assert (got.get("plan", 0), got.get("scan2", 0)) == ((1, 1) if wide else (0, 0)), (where, got)
    assert not codes and len(res) == world, (where, codes)
    assert got.get("emit", 0) == 1, (where, got)
    assert res[0]["fill_level"] == case["L"] and res[0]["max_free"] == case["maxc"], (where, res[0])
    _shard_finish(bals, o, res, args, where)


@pytest.mark.parametrize("xplan,xself", SHARD_KNOBS)
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_first_launch_seam(world, xplan, xself):
    """The first launch at 32 / 64 / 128 rows under a worker of R + 1, 255, 256 (the one-byte
    clamp) or 70 000 (beyond the two-byte clamp) free processes: no relaunch at L = R - 2,
    FB_ERERUN on every rank at L = R - 1."""
    cases = [(R, fc.shard_case(L, R, m)) for R, m in fc.SHARD_FIRST for L in (R - 2, R - 1)]
    bals = _shard_group(world, max(c["log_cap"] for _, c in cases), xplan, xself)
    try:
        for R, case in cases:
            _shard_tick(bals, case, R, (world, R, case["L"], case["maxc"]))
    finally:
        for b in bals:
            b.close()


@pytest.mark.parametrize("xplan,xself", SHARD_KNOBS)
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("L", fc.SHARD_WIDE_LEVELS)
def test_sharded_levels_after_the_relaunch(L, world, xplan, xself):
    """After the relaunch (two-byte counts, k_emit_shard_wide): the 64-round chunk seams, the
    last chunk and L = limit - 2, under workers at and beyond the two-byte clamp."""
    R_first = 128 if L >= 127 else 64
    cases = [fc.shard_case(L, R_first, m) for m in fc.SHARD_WIDE_MAXC]
    bals = _shard_group(world, max(c["log_cap"] for c in cases), xplan, xself)
    try:
        for case in cases:
            _shard_tick(bals, case, R_first, (world, L, case["maxc"]))
    finally:
        for b in bals:
            b.close()


@pytest.mark.parametrize("xplan,xself", SHARD_KNOBS)
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_row_limit(world, xplan, xself):
    """L = 4095 under a worker beyond 4096: FB_ERERUN, then FB_ERANGE on every rank, nothing
    committed on any; the group's next, smaller tick is exact."""
    from test_gpu_sharded import _cmp_state as _cmp_shard_state
    case = fc.shard_case(ROW_LIMIT - 1, R_FUSED, 70000)
    assert case["erange"]
    bals = _shard_group(world, case["log_cap"], xplan, xself)
    try:
        o = _shard_load(bals, case, R_FUSED)
        args = fc.tick_args(case)
        res, codes, _ = _shard_attempt(bals, args)
        assert codes == [FB_ERERUN] * world and not res
        res, codes, _ = _shard_attempt(bals, args)
        assert codes == [FB_ERANGE] * world and not res
        _cmp_shard_state(bals, o, 0)
        small = dict(case, T=1000, ev=case["ev"])
        args = fc.tick_args(small)
        for attempt in range(3):
            res, codes, _ = _shard_attempt(bals, args)
            if not codes:
                break
            assert codes == [FB_ERERUN] * world
        assert len(res) == world
        _shard_finish(bals, o, res, args, (world, "after FB_ERANGE"))
    finally:
        for b in bals:
            b.close()


XP_W = 257 * 256 + 5  # more than 256 queue blocks: no one-launch phase 2


@pytest.mark.parametrize("xplan", [1, 0])
def test_sharded_large_queue_seam(xplan):
    """A queue of more than 256 blocks at 32 rows: k_xscan + k_emit_shard_xp (xplan), or the
    recount into group rows + k_emit_shard (xplan 0), either side of L = R - 1 under a worker
    of R + 1; the relaunch has 64 rows and re-counts."""
    R, world = 32, 2
    cases = [fc.shard_case(L, R, R + 1, W=XP_W) for L in (R - 2, R - 1)]
    bals = _shard_group(world, max(c["log_cap"] for c in cases), xplan, 1, W=XP_W)
    try:
        for case in cases:
            o = _shard_load(bals, case, R)
            args = fc.tick_args(case)
            res, codes, got = _shard_attempt(bals, args)
            assert (got.get("plan", 0), got.get("scan2", 0), got.get("emit", 0)) == ((1, 0, 1) if xplan else (0, 1, 1)), got
            if case["L"] == R - 1:
                assert codes == [FB_ERERUN] * world and not res, codes
                res, codes, got = _shard_attempt(bals, args)
                assert (got.get("plan", 0), got.get("scan2", 0), got.get("emit", 0)) == (0, 1, 1), got
            assert not codes and len(res) == world, codes
            assert (res[0]["fill_level"], res[0]["max_free"]) == (case["L"], R + 1), res[0]
            _shard_finish(bals, o, res, args, (xplan, case["L"]))
    finally:
        for b in bals:
            b.close()
