"""Launches that carry results and are never committed: abandoned, or failed at their wait.

fb_tick_launch promises that "launching again without fb_tick_commit recomputes the same
tick", a failed fb_tick_wait that "nothing is committed", and fb_read_state / fb_log_compact /
fb_pool_stats read "the committed state".  A context without deferred clears -- a deque
context, one GPU past 128 K workers, a shard -- completes the log entries its results name in
place, at launch, and notes them; k_log_undo takes them back before the next launch and
before anything reads or replaces the committed log after a failed wait.  Contexts of at most
128 K workers defer their clears (ctag / ev_clr) and never touch the log before the commit.
Every case runs on that kind as well (H-small): it needs no undo, and these tests keep it so.

The cases come from tests/abandoned.py (tests/test_abandoned_coverage.py states what they
reach); everything is compared with the oracle that never saw the abandoned launch, bit for
bit: event status, assignments, orphans and evicted slots every tick, the whole state -- log
included -- at the end.  On a heartbeat context the last tick lets every worker expire: an
entry that an abandoned launch left completed is missing from its orphans.

Every H-large test runs at most five launches on a context of (1 << 17) + 5 slots (the
FB_ENOSPC and dispatcher tests: on each of their two contexts, whose logs hold under 100
entries); the whole file takes under three seconds.
"""
import numpy as np
import pytest

import abandoned
from faasbal import FaasbalError, GpuBalancer, _lib, synth
from faasbal.balancer import TEST_PATHS
from faasbal.poolstats import pool_stats_model
from lc_model import compact_model
from oracle import DequeOracle, Oracle

pytestmark = pytest.mark.gpu

TTE = 10.0
REG, HB, RES = synth.EV_REGISTER, synth.EV_HEARTBEAT, synth.EV_RESULT
H_LARGE_W = abandoned.H_LARGE_W
OUT_KEYS = ("reconnect", "assign", "orphans", "evicted")


# ------------------------------------------------------------------ helpers
def _context(case):
    W = len(case.st["reg"])
    if case.deque:
        g = GpuBalancer(W, case.log_cap, max_events=case.max_events, mode="deque", max_tokens=8 * W + 4096)
    else:
        g = GpuBalancer(W, case.log_cap, max_events=case.max_events)
    g.load(case.st)
    return g


def _cmp_out(a, b, what):
    for k in OUT_KEYS:
        np.testing.assert_array_equal(a[k], b[k], err_msg="%s: %s" % (what, k))


def _cmp_state(sg, so, what, log=True, epoch=True):
    """epoch=False: a deque context (the deque oracle keeps no epochs: nothing is redistributed)."""
    np.testing.assert_array_equal(sg["reg"], so["reg"], err_msg=what + ": reg")
    np.testing.assert_array_equal(sg["queue"], so["queue"], err_msg=what + ": queue")
    assert sg["head"] == so["head"], what + ": head"
    reg = so["reg"].astype(bool)
    for k in ("free", "hb", "epoch") if epoch else ("free", "hb"):
        np.testing.assert_array_equal(sg[k][reg], so[k][reg], err_msg="%s: %s" % (what, k))
    if log:
        diff = int(np.sum(sg["log"] != so["log"]))
        assert diff == 0, "%s: %d log entries differ, first at %d" % (
            what, diff, int(np.flatnonzero(sg["log"] != so["log"])[0]))


def _launch(g, args, wait=True):
    g.launch(*args)
    return g.wait() if wait else None


def replay(case, g, wait=True):
    """The case's launches on g, every committed tick against the oracle's outputs, the
    whole state at the end."""
    for i, ((op, args), want) in enumerate(zip(case.steps, case.want)):
        if op == "abandon":
            _launch(g, args, wait)
            continue
        a = g.tick(*args)
        _cmp_out(a, want, "%s launch %d" % (case.name, i))
    _cmp_state(g.read_state(), case.final, case.name + " final state", epoch=not case.deque)


ONE = [k for k in abandoned.CASES if k.endswith("-one")]
TWO = [k for k in abandoned.CASES if k.endswith("-two")]
COMMITTED = [k for k in abandoned.CASES if k.endswith("-committed")]


# ------------------------------------------------------------------ 1-3, 5: the replayed cases
@pytest.mark.parametrize("wait", [True, False], ids=["waited", "not-waited"])
@pytest.mark.parametrize("name", ONE)
def test_abandoned_launch(name, wait):
    """1, 2. A launch whose results name live entries, waited for or not, never committed; two
    committed ticks with other messages (the second: the notes are not applied twice); on
    heartbeat contexts the tick at which everybody has expired."""
    case = abandoned.case(name)
    g = _context(case)
    replay(case, g, wait)
    g.close()


@pytest.mark.parametrize("name", TWO)
def test_two_abandoned_launches_in_a_row(name):
    """3. Two abandoned launches with different result sets, then a committed third: the
    second launch takes the first one's clears back before it runs, the third the second's."""
    case = abandoned.case(name)
    g = _context(case)
    replay(case, g, wait=False)
    g.close()


@pytest.mark.parametrize("name", COMMITTED)
def test_committed_then_next_launch(name):
    """5. The launch with results is committed: the next launch must not put the committed
    clears back (the notes are dropped at the commit)."""
    case = abandoned.case(name)
    g = _context(case)
    replay(case, g)
    g.close()


@pytest.mark.parametrize("knob", [("ev_ll", 0), ("plan", 1)], ids=["ev_ll0", "plan1"])
@pytest.mark.parametrize("name", [k for k in ONE if k.startswith("h-small")])
def test_abandoned_launch_deferred_other_paths(monkeypatch, name, knob):
    """H-small through the sort (its atomicExch on ctag) and through the three-launch path."""
    monkeypatch.setitem(TEST_PATHS, *knob)
    case = abandoned.case(name)
    g = _context(case)
    replay(case, g)
    g.close()


def test_h_large_window_attempt_falls_back():
    """4c. H-large with the window in auto mode: the abandoned launch starts as a window tick
    (the tick before it ended at fill level 0 without orphans), cannot finish inside its window
    -- its registrations go to the front and no task serves them -- and reruns on the general
    path under a stamp of its own; the notes of both passes belong to the one launch.  The
    case's abandoned batch, launched one committed tick later (its entries are still in
    flight, its times lie before that tick's clock)."""
    case = abandoned.case("h-large-one")
    g = _context(case)
    assert [op for op, _ in case.steps] == ["tick", "abandon", "tick", "tick", "tick"]
    batch = case.steps[1][1][2:7]
    assert (batch[0] == REG).sum() == 100
    for i in (0, 2):
        _cmp_out(g.tick(*case.steps[i][1]), case.want[i], "launch %d" % i)
    r = _launch(g, (case.steps[3][1][0], TTE, *batch, 0))
    assert r["reruns"] >= 1 and g.window_stats()[1] == 1, (r, g.window_stats())
    for i in (3, 4):
        _cmp_out(g.tick(*case.steps[i][1]), case.want[i], "launch %d" % i)
    _cmp_state(g.read_state(), case.final, "window attempt fell back")
    g.close()


def test_reader_between_wait_and_commit_sees_the_launched_clears():
    """The documented exception (include/faasbal.h, fb_read_state): between a successful wait
    and the commit a context without deferred clears shows the launched tick's completed
    entries; the commit relies on them.  A deferred context shows the committed log."""
    for name in ("d-zipf-committed", "h-small-2-one"):
        case = abandoned.case(name)
        g = _context(case)
        i = [op for op, _ in case.steps].index("abandon" if "small" in name else "tick", 1)
        for op, args in case.steps[:i]:
            g.tick(*args)
        before = g.read_state()["log"].copy()
        _launch(g, case.steps[i][1])
        seen = g.read_state()["log"]
        T = case.targets[0]
        assert (before[T] >= 0).all()
        if case.deque:
            assert (seen[T] == -1).all() and np.array_equal(np.delete(seen, T), np.delete(before, T))
            g.commit()
            for (op, args), want in zip(case.steps[i + 1:], case.want[i + 1:]):
                _cmp_out(g.tick(*args), want, name)
            _cmp_state(g.read_state(), case.final, name, epoch=False)
        else:
            np.testing.assert_array_equal(seen, before)
        g.close()


# ------------------------------------------------------------------ directed states
def _state(kind, free, hb, queue, log):
    """A few registered workers; kind "h-large": in a table of (1 << 17) + 5 slots (clears in
    place), "h-small": a table of their number (deferred clears), "deque": a deque context."""
    n = len(free)
    W = H_LARGE_W if kind == "h-large" else n
    pad = lambda a, dt: np.concatenate([np.asarray(a, dt), np.zeros(W - n, dt)])
    return dict(reg=pad(np.ones(n), np.uint8), free=pad(free, np.int32), hb=pad(hb, np.float64),
                epoch=np.zeros(W, np.uint32), queue=np.asarray(queue, np.int32), log=np.asarray(log, np.int32))


def _pair(kind, st, cap, max_events=64):
    W = len(st["reg"])
    if kind == "deque":
        g, o = GpuBalancer(W, cap, max_events=max_events, mode="deque"), DequeOracle(W, cap)
    else:
        g, o = GpuBalancer(W, cap, max_events=max_events), Oracle(W, cap)
    g.load(st)
    o.load(st["reg"], st["free"], st["hb"], st["epoch"], st["queue"], st["log"])
    return g, o


def _ev(events):
    """(kind, slot, val, ts, seq) columns of (kind, slot, val, ts, seq) rows."""
    col = lambda j, dt: np.asarray([e[j] for e in events], dt)
    return col(0, np.uint8), col(1, np.int32), col(2, np.int32), col(3, np.float64), col(4, np.int64)


def _both(g, o, args, what):
    a, b = g.tick(*args), o.tick(*args)
    _cmp_out(a, b, what)
    return a, b


def _end(g, o, what):
    _cmp_state(g.read_state(), o.export(), what, epoch=not isinstance(o, DequeOracle))


def _death(g, o, now, completed, ev=()):
    """Everybody without a message in `ev` has expired at `now`: every in-flight entry of
    theirs is an orphan, and none of `completed` is."""
    live = np.flatnonzero(o.export()["log"] >= 0)
    a, b = _both(g, o, (now, TTE, *(_ev(list(ev)) if ev else ([], [], [], [], [])), 0), "death")
    assert len(b["orphans"]) > 0 and np.isin(b["orphans"], live).all() and not np.isin(completed, b["orphans"]).any()
    return b


KINDS = ["h-large", "h-small", "deque"]
HEARTBEAT = ["h-large", "h-small"]


# ------------------------------------------------------------------ 4: launches that reran internally
@pytest.mark.parametrize("kind", HEARTBEAT)
def test_abandoned_launch_that_reran_through_the_sort(kind):
    """4a. 17 results of slot 0 in one launch (more than the linked lists hold: fb_tick_wait
    reruns the tick through the sort, under a new stamp).  The first pass completed slot 1's
    entries, the rerun slot 0's: both passes' notes are the launch's, and both are taken
    back.  One result repeats an entry, one names an entry of slot 1.  H-small: the rerun's
    stamp over the first pass's ctag marks."""
    st = _state(kind, free=[0, 0, 4], hb=[999.0, 999.0, 999.0], queue=[2], log=[0] * 20 + [1] * 5)
    g, o = _pair(kind, st, 4096)
    _both(g, o, (999.5, TTE, *_ev([(HB, 2, 0, 999.25, -1)]), 2), "before")
    seqs = list(range(15)) + [3, 21]
    ev = [(RES, 0, 0, 999.5 + i / 64.0, q) for i, q in enumerate(seqs)] + [(RES, 1, 0, 999.875, q) for q in (20, 22, 24)]
    r = _launch(g, (1000.0, TTE, *_ev(ev), 3))
    if TEST_PATHS.get("ev_ll", 1) != 0:
        assert r["reruns"] >= 1, r
    _both(g, o, (1000.5, TTE, *_ev([(HB, 2, 0, 1000.25, -1)]), 1), "after")
    _both(g, o, (1001.0, TTE, *_ev([(RES, 1, 0, 1000.75, 23)]), 1), "after, second")
    b = _death(g, o, 1012.0, [23])
    assert set(range(23)) | {24} <= set(b["orphans"].tolist())
    _end(g, o, "reran through the sort (%s)" % kind)
    g.close()


@pytest.mark.parametrize("kind", KINDS)
def test_abandoned_launch_that_reran_with_a_wider_round_table(kind):
    """4b. A result pushes a free count past the launch's round table: fb_tick_wait reruns
    the tick wider.  The first pass completed the entry; the rerun finds it completed and
    notes nothing -- the first pass's note must survive the rerun's new stamp."""
    st = _state(kind, free=[64, 3, 200], hb=[999.0] * 3, queue=[0, 1], log=[0, 0, 1])
    g, o = _pair(kind, st, 10_000)
    r = _launch(g, (1000.0, TTE, *_ev([(RES, 0, 0, 999.5, 1), (RES, 1, 0, 999.75, 2)]), 1000))
    assert r["reruns"] >= 1, r
    _both(g, o, (1000.5, TTE, *_ev([(HB, 1, 0, 1000.25, -1)]), 10), "after")
    _both(g, o, (1001.0, TTE, *_ev([(RES, 0, 0, 1000.75, 0)]), 10), "after, second")
    if kind != "deque":
        b = _death(g, o, 1020.0, [0])
        assert {1, 2} <= set(b["orphans"].tolist())
    _end(g, o, "reran wider (%s)" % kind)
    g.close()


# ------------------------------------------------------------------ 6: fb_load_state
@pytest.mark.parametrize("name", ["h-large-one", "d-zipf-one", "h-small-2-one", "h-small-11-one"])
def test_load_state_after_an_abandoned_launch(name):
    """6. fb_load_state replaces the log: the notes of a launch abandoned before it are dropped
    with it, else the next launch writes the old owners at the old indices into the loaded log
    (whose entries belong to other workers)."""
    case = abandoned.case(name)
    g = _context(case)
    i = [op for op, _ in case.steps].index("abandon")
    for op, args in case.steps[:i]:
        g.tick(*args)
    _launch(g, case.steps[i][1])
    W = len(case.st["reg"])
    st2 = synth.zipf_deque_state(W=W, seed=9, dup_frac=0.1) if case.deque else \
        synth.zipf_state(W=W, seed=9, dead_frac=0.0)
    T = case.targets[0][case.targets[0] < len(st2["log"])]
    assert len(T) > len(case.targets[0]) // 2 and (st2["log"][T] != case.at_launch["log"][T]).mean() > 0.9
    g.load(st2)
    o = (DequeOracle if case.deque else Oracle)(W, case.log_cap)
    o.load(st2["reg"], st2["free"], st2["hb"], st2["epoch"], st2["queue"], st2["log"])
    rng = np.random.default_rng(5)
    for t in range(2):
        now = 1000.0 + (t + 1) / 64.0
        ev = abandoned.other_messages(rng, o.export(), 200, 200, [], now - 1 / 64.0, now)
        _both(g, o, (now, TTE, *ev, 500), "%s after the load, tick %d" % (name, t))
    _end(g, o, name + " after the load")
    g.close()


# ------------------------------------------------------------------ 7, 8: failed waits and the readers
def _pool_state(kind):
    """64 workers with 3 free processes and 4 in-flight entries each, all queued."""
    rng = np.random.default_rng(11)
    n = 64
    return _state(kind, free=[3] * n, hb=1000.0 - 0.25 * rng.integers(0, 32, n), queue=rng.permutation(n),
                  log=rng.permutation(np.repeat(np.arange(n), 4)))


def _results(st, slots, ts):
    """One result per slot naming the slot's first in-flight entry."""
    return [(RES, s, 0, t, int(np.flatnonzero(st["log"] == s)[0])) for s, t in zip(slots, ts)]


def _invalid_batch(st, bad):
    """Valid results before and after the first invalid message (index 2 or 3)."""
    ev = _results(st, (1, 2), (999.0, 999.5)) + [(HB, 3, 0, 999.6, -1), (HB, 4, 0, 999.7, -1)] + \
        _results(st, (5, 6), (999.8, 999.9))
    k, s, v, ts, q = _ev(ev)
    if bad == "decreasing":
        ts[2] = 998.0
    if bad == "future":
        ts[3] = 1000.5
    if bad == "slot":
        s[2] = 1 << 20
    if bad == "kind":
        k[3] = 9
    return (k, s, v, ts, q), (2 if bad in ("decreasing", "slot") else 3)


def _fail_invalid(g, st, bad, resident):
    (k, s, v, ts, q), first = _invalid_batch(st, bad)
    with pytest.raises(FaasbalError, match="event %d" % first) as e:
        if resident:
            import torch
            d = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (k, s, v, ts, q)]
            g.stage_device(1000.0, *d)
            g.launch_staged(TTE, 10)
            g.wait()
        else:
            g.tick(1000.0, TTE, *g.pin_events(k, s, v, ts, q), 10)
    assert e.value.code == _lib.FB_EINVAL


def _valid_tick(st, then="same"):
    """The failed batch without its fault ("same"), or results of other workers ("other": the
    entries the failed batch named stay in flight until their workers expire)."""
    a, b = ((1, 2), (5, 6)) if then == "same" else ((7, 8), (9, 10))
    ev = _results(st, a, (999.0, 999.5)) + [(HB, 3, 0, 999.6, -1)] + _results(st, b, (999.8, 999.9))
    return (1000.0, TTE, *_ev(ev), 10)


def _named(st, then):
    """The entries the valid tick completed."""
    return [e[4] for e in _results(st, (1, 2, 5, 6) if then == "same" else (7, 8, 9, 10), (0,) * 4)]


@pytest.mark.parametrize("then", ["same", "other"])
@pytest.mark.parametrize("resident", [False, True], ids=["pinned", "resident"])
@pytest.mark.parametrize("bad", ["decreasing", "future", "slot", "kind"])
@pytest.mark.parametrize("kind", HEARTBEAT)
def test_invalid_message_among_results(kind, bad, resident, then):
    """7. An invalid message in a pinned or device-resident batch, results before and after it:
    the wait fails, nothing is committed -- the entries the valid results named are in flight.
    Then the same tick without the invalid message, or a tick with other workers' results
    (the failed batch's entries are then orphans when everybody expires), equals the oracle."""
    st = _pool_state(kind)
    g, o = _pair(kind, st, 4096)
    _fail_invalid(g, st, bad, resident)
    _both(g, o, _valid_tick(st, then), "after the failure")
    b = _death(g, o, 1030.0, _named(st, then))
    assert len(b["orphans"]) == 256 - 4 + 10
    _end(g, o, "invalid message (%s, %s)" % (kind, bad))
    g.close()


def _view_log(g):
    """The log through fb_device_view_get's pointer (read with torch)."""
    import torch

    v = g.device_view()

    class Dev:
        __cuda_array_interface__ = dict(shape=(int(v.log_head),), typestr="<i4", data=(int(v.log_slot), False),
                                        version=2)

    return torch.as_tensor(Dev(), device="cuda:0").cpu().numpy()


# (fb_read_inflight exists on contexts with deferred clears only)
READERS = [(k, r) for k in HEARTBEAT for r in ("read_state", "compact_log", "pool_stats", "device_view", "inflight")
           if r != "inflight" or k == "h-small"]


@pytest.mark.parametrize("kind,reader", READERS)
def test_readers_after_a_failed_wait(kind, reader):
    """8. After a wait that failed and before any new launch, each reader of the committed
    state alone: the log read, the compaction (the caller's live count holds, kept is the
    model's), the pool summary's in-flight counts, the device view's log, and where they
    exist (H-small) the per-slot in-flight counts.  The tick before the failed one is
    committed but, on the linked-list path, its commit still rides in the failed launch."""
    st = _pool_state(kind)
    g, o = _pair(kind, st, 4096)
    _both(g, o, (999.0, TTE, [], [], [], [], [], 30), "before")
    _fail_invalid(g, st, "slot", False)
    so = o.export()
    live = int((so["log"] >= 0).sum())
    if reader == "read_state":
        np.testing.assert_array_equal(g.read_state()["log"], so["log"])
    elif reader == "device_view":
        np.testing.assert_array_equal(_view_log(g), so["log"])
    elif reader == "inflight":
        np.testing.assert_array_equal(g.inflight(), np.bincount(so["log"][so["log"] >= 0], minlength=64))
    elif reader == "pool_stats":
        got, want = g.pool_stats(1000.0, TTE), pool_stats_model(so, 1000.0, TTE)
        assert (got["inflight"], got["inflight_expired"]) == (want["inflight"], want["inflight_expired"]) == (live, 0)
    else:
        want, kept = compact_model(dict(so, log=so["log"]))
        out = g.compact_log(expect=live)
        assert out["n_kept"] == live
        np.testing.assert_array_equal(out["kept"], kept)
        _cmp_state(g.read_state(), want, "after the compaction")
    if reader != "compact_log":
        _both(g, o, _valid_tick(st), "after the reader")
        _end(g, o, reader)
    g.close()


@pytest.mark.parametrize("kind", KINDS)
def test_enospc_with_results_then_readers(kind):
    """7, 8. test_enospc_then_compact_then_rerun's shape on every context kind:
    the tick's results name live entries, its dispatches overflow the log (FB_ENOSPC, nothing
    committed).  The log read equals the committed one, the compaction finds the caller's live
    count and the model's kept list, and the same tick, renumbered, equals the oracle's."""
    from test_gpu_log_compact import SeqMap, _final, _tick_pair

    log = np.full(60, -1, np.int32)
    log[[5, 17, 30, 31, 59]] = [1, 2, 1, 4, 2]
    st = _state(kind, free=[3] * 8, hb=[1000.0] * 8, queue=np.arange(8), log=log)
    g, _ = _pair(kind, st, 64, max_events=16)
    o = (DequeOracle if kind == "deque" else Oracle)(len(st["reg"]), 4096)
    o.load(st["reg"], st["free"], st["hb"], st["epoch"], st["queue"], st["log"])
    m = SeqMap(60)
    tk = dict(ev_kind=np.asarray([RES, RES, HB], np.uint8), ev_slot=np.asarray([1, 2, 3], np.int32),
              ev_val=np.zeros(3, np.int32), ev_ts=np.full(3, 1001.0), now=1001.0)
    seq_o = np.asarray([30, 59, -1], np.int64)
    before = g.read_state()
    with pytest.raises(FaasbalError) as e:
        g.tick(tk["now"], TTE, tk["ev_kind"], tk["ev_slot"], tk["ev_val"], tk["ev_ts"], m.to_gpu(seq_o), 20)
    assert e.value.code == _lib.FB_ENOSPC
    np.testing.assert_array_equal(g.read_state()["log"], before["log"], err_msg="the log after FB_ENOSPC")
    g.close()
    # ... and the compaction as the first reader
    g, _ = _pair(kind, st, 64, max_events=16)
    with pytest.raises(FaasbalError):
        g.tick(tk["now"], TTE, tk["ev_kind"], tk["ev_slot"], tk["ev_val"], tk["ev_ts"], m.to_gpu(seq_o), 20)
    out = g.compact_log(expect=5)
    np.testing.assert_array_equal(out["kept"], [5, 17, 30, 31, 59])
    m.compacted(out["kept"])
    want, _ = compact_model(before, deque=kind == "deque")
    _cmp_state(g.read_state(), want, "after the compaction", epoch=kind != "deque")
    if kind != "deque":
        assert g.pool_stats(1001.0, TTE)["inflight"] == 5
    b = _tick_pair(g, o, m, tk, TTE, 20, 0, seq_o=seq_o)
    assert len(b["assign"]) == 20
    _final(g, o, m)
    g.close()


@pytest.mark.parametrize("then", ["same", "other"])
@pytest.mark.parametrize("kind,eager", [("h-large", False), ("h-large", True), ("h-small", False),
                                        ("h-small", True), ("deque", False)])
def test_length_check_failure_with_results(kind, eager, then):
    """7. The device-reported queue length fails fb_tick_wait's check (fault_qlen) on a tick
    whose results completed entries (in place, or on H-small as ctag / ev_clr marks) -- on the
    heartbeat kinds with window ticks on, with the eager commit behind the tick or not:
    nothing is committed, its notes are taken back, and the same tick, or one with other
    workers' results, runs."""
    st = _pool_state(kind)
    g, o = _pair(kind, st, 4096)
    if kind != "deque":
        g.set_window(1)  # (auto mode wants a queue several times the scanned prefix)
        g.set_eager_commit(eager)
    _both(g, o, (999.0, TTE, [], [], [], [], [], 30), "before")
    g.set_path("fault_qlen", 1 << 30)
    with pytest.raises(FaasbalError, match="queue length|window|deque of"):
        g.tick(*_valid_tick(st))
    _both(g, o, _valid_tick(st, then), "after the failure")
    if kind != "deque":
        assert g.window_stats()[0] >= 1
        b = _death(g, o, 1030.0, _named(st, then))
        assert len(b["orphans"]) == 256 + 30 + 10 - 4
    _end(g, o, "length check (%s, eager %d)" % (kind, eager))
    g.close()


def test_sharded_readers_after_a_length_check_failure():
    """8, S. A sharded tick with results fails the length check on every rank: fb_read_state
    on each rank shows its shard of the committed log before any new launch, and the same
    tick then equals the oracle."""
    import torch
    from test_gpu_shard_forms import RESULT, _Batch, _close, _group_of, _small
    from test_gpu_sharded import _cmp, _cmp_state as _cmp_shards, _group_tick

    st, cap = _small(4096)
    rng = np.random.default_rng(7)
    bals, o = _group_of(st, cap, 2)
    try:
        live = rng.choice(np.nonzero(o.export()["log"] >= 0)[0], 300, replace=False)
        b = _Batch()
        b.add(RESULT, o.export()["log"][live], seq=live)
        args = (1000.0, TTE, *b.events(rng, 1000.0), 100)
        for x in bals:
            x.set_path("fault_qlen", 1 << 30)
            x.launch(*args)
        torch.cuda.synchronize()
        total = bals[0].exchange().clone()
        for x in bals[1:]:
            total += x.exchange()
        for x in bals:
            x.exchange().copy_(total)
        torch.cuda.synchronize()
        for x in bals:
            x.cont()
        for x in bals:
            with pytest.raises(FaasbalError, match="queue length"):
                x.wait()
        _cmp_shards(bals, o, 0)
        a, _r = _group_tick(bals, *args)
        _cmp(bals, o, a, o.tick(*args), 0)
    finally:
        _close(bals)


# ------------------------------------------------------------------ 9: the drop-in dispatcher
@pytest.mark.parametrize("kind", ["deque", "h-large"])
def test_dispatcher_enospc_with_results_compacts_on_the_device(kind):
    """9. The drop-in on a context that clears in place: a tick that carries results overflows
    the in-flight log (FB_ENOSPC).  The failed launch's clears are taken back before
    fb_log_compact counts, so the device's live count is the dispatcher's and the recovery is
    the device compaction (not the host fallback after FB_ESTATE); every message sent equals
    a run whose log never fills, and the device log is the dispatcher's in-flight table."""
    from faasbal import codec
    from faasbal.dispatcher import GpuPushDispatcher
    from test_dispatcher import FakeEnv, wid

    def msg(w, typ, data, now):
        return (wid(w), codec.serialize({"type": typ, "data": data}).encode(), now)

    W = H_LARGE_W if kind == "h-large" else 8
    runs, comp = [], []
    for cap in (1 << 12, 73):
        env = FakeEnv()
        bal = GpuBalancer(W, cap, max_events=128) if kind == "h-large" else None
        d = GpuPushDispatcher("127.0.0.1", 0, 10, max_workers=W, max_events=128, max_inflight=cap,
                              redis_client=env, subscriber=env, socket=env, poller=env, clock=env.clock,
                              balancer=bal)
        if kind == "deque":
            d.use_loop("deque")
        env.tasks.extend("e%d" % j for j in range(80))
        sent, prev = [], []
        for t in range(4):
            env.now = 1000.0 + t
            if t == 0:  # two workers with one process each
                env.inbound += [msg(w, "register", {"num_processes": 1}, env.now) for w in range(2)]
            if t == 1:  # a worker that takes ten tasks and never answers
                env.inbound.append(msg(2, "register", {"num_processes": 10}, env.now))
            if t == 2:  # 13 entries + 61 dispatches > 73: FB_ENOSPC; 12 after the compaction fit
                env.inbound.append(msg(3, "register", {"num_processes": 59}, env.now))
            for (dst, m) in prev:
                if m["type"] == "task" and dst == wid(0) and t <= 2:
                    env.inbound.append(msg(0, "result", {"task_id": m["data"]["task_id"], "status": "COMPLETED",
                                                         "result": 1}, env.now))
            if t == 2:
                first = [m for dst, m in sent[0] if m["type"] == "task" and dst == wid(1)]
                env.inbound.append(msg(1, "result", {"task_id": first[0]["data"]["task_id"], "status": "COMPLETED",
                                                     "result": 1}, env.now))
            env.sent.clear()
            d.tick()
            prev = list(env.sent)
            sent.append(prev)
            st = d.balancer.read_state()
            want = np.full(d.head, -1, np.int32)
            for q, (_tid, s) in d.inflight.items():
                want[q] = s
            np.testing.assert_array_equal(st["log"], want, err_msg="cap %d tick %d" % (cap, t))
        runs.append(sent)
        comp.append((d.compactions, d.device_compactions))
        d.balancer.close()
    assert comp == [(0, 0), (1, 1)], comp
    assert runs[0] == runs[1]
    assert sum(m["type"] == "task" for _, m in runs[1][2]) == 61
