"""Ticks back to back: what a one-GPU heartbeat context carries from one tick to the next.

A commit leaves the log entries it redistributed in the log (lazy clears; an entry q naming
slot s is live only if s holds a record and q >= epoch[s]) and rides in the next tick's
first launch (deferred commits).  A state read with the log settles both -- it clears the
stale entries (k_log_normalize) and flushes the commit -- so a test that reads the state
after every tick never runs a tick on what a dispatcher that never reads leaves behind.
Here the same oracle-compared scenarios run in three read modes:

  settled  read_state() after every tick, as the rest of the suite does (for contrast)
  columns  read_state(with_log=False) + inflight() after every tick: the commit is flushed
           as its own launch, the log keeps its stale entries
  none     nothing read until the last tick: every commit folded into the next launch

with results aimed at stale entries (tests/carried.py; tests/test_carried_coverage.py
counts what the scenarios reach).  Bit-exact against oracle.Oracle on every output every
tick, and on the whole state -- log and epoch included -- after the last one.
"""
import numpy as np
import pytest

import carried
from faasbal import GpuBalancer, synth
from faasbal.balancer import TEST_PATHS

pytestmark = pytest.mark.gpu

TTE = 10.0
EV_REG, EV_RECON, EV_HB, EV_RES = synth.EV_REGISTER, synth.EV_RECONNECT, synth.EV_HEARTBEAT, synth.EV_RESULT


class Unsettled:
    """A GpuBalancer on which nothing that settles the log can be called by accident: a
    state read with the log, the device view, a load and fb_set_path("lazy") raise."""

    def __init__(self, g):
        self._g = g

    def __getattr__(self, name):
        if name in ("device_view", "load", "load_state"):
            raise AssertionError("%s() would settle the log" % name)
        return getattr(self._g, name)

    def read_state(self, with_log=True):
        if with_log:
            raise AssertionError("read_state() with the log would settle it")
        return self._g.read_state(with_log)

    def set_path(self, name, value):
        if name == "lazy":
            raise AssertionError('set_path("lazy") would settle the log')
        return self._g.set_path(name, value)


def _cmp_out(a, b, t):
    for k in ("reconnect", "assign", "orphans", "evicted"):
        np.testing.assert_array_equal(a[k], b[k], err_msg="tick %d: %s" % (t, k))


def _cmp_columns(g, o, t):
    """The committed columns without the log (neither call settles it), and the in-flight
    counts against the oracle's live entries."""
    sg, so = g.read_state(with_log=False), o.export()
    assert "log" not in sg
    np.testing.assert_array_equal(sg["reg"], so["reg"], err_msg="tick %d reg" % t)
    np.testing.assert_array_equal(sg["queue"], so["queue"], err_msg="tick %d queue" % t)
    assert sg["head"] == so["head"], "tick %d head" % t
    reg = so["reg"].astype(bool)
    for k in ("free", "hb", "epoch"):
        np.testing.assert_array_equal(sg[k][reg], so[k][reg], err_msg="tick %d %s" % (t, k))
    if g.max_workers <= 1 << 17:  # contexts that keep in-flight counts
        live = so["log"][so["log"] >= 0]
        np.testing.assert_array_equal(g.inflight(), np.bincount(live, minlength=len(reg)).astype(np.uint32),
                                      err_msg="tick %d in-flight counts" % t)


def _cmp_full(g, o, t):
    _cmp_columns(g, o, t)
    sg, so = g.read_state(), o.export()
    np.testing.assert_array_equal(sg["log"], so["log"], err_msg="tick %d log" % t)
    reg = so["reg"].astype(bool)
    np.testing.assert_array_equal(sg["reg"], so["reg"], err_msg="tick %d reg" % t)
    np.testing.assert_array_equal(sg["queue"], so["queue"], err_msg="tick %d queue" % t)
    for k in ("free", "hb", "epoch"):
        np.testing.assert_array_equal(sg[k][reg], so[k][reg], err_msg="tick %d %s (settled)" % (t, k))


def _pair(st, log_cap, max_events=4096, window=None, eager=False, purge_mode=1):
    g = GpuBalancer(len(st["reg"]), log_cap, max_events=max_events)
    if window is not None:
        g.set_window(window)
        g.set_eager_commit(eager)
    g.load(st)
    return g, carried.OracleRun(st, log_cap, purge_mode=purge_mode)


def drive(g, run, ticks, tte, resolve, mode, t0=0, last=True, aim=True, timing=None):
    """Run ``ticks`` on the pair: the four outputs compared every tick, between ticks what
    ``mode`` reads; after the last tick (``last``) the whole state.  ``timing``: a dict that
    receives fb_timing_read's launches between the first tick and the end of the last."""
    u = g if mode == "settled" else Unsettled(g)
    outs = []
    for i, tk in enumerate(ticks):
        t = t0 + i
        if callable(tk):  # a tick shaped by what the oracle has seen so far
            tk = tk(run)
        args = run.args(tk, tte, resolve, aim)
        a, b = u.tick(*args), run.tick(args)
        _cmp_out(a, b, t)
        assert a["result"]["queue_len"] == len(run.o.export()["queue"]), "tick %d: queue length" % t
        outs.append((a, b))
        if timing is not None and i == 0:
            u.timing_enable(True)
            u.timing_read()
        if i + 1 == len(ticks):
            break
        if mode == "settled":
            _cmp_full(g, run.o, t)
        elif mode == "columns":
            _cmp_columns(u, run.o, t)
    if timing is not None:
        timing.update(u.timing_read())
        u.timing_enable(False)
    if last:
        _cmp_full(g, run.o, t0 + len(ticks) - 1)
    return outs


def _run_family(family, seed, mode, window=None, eager=False, timing=None):
    scen, cap, max_events, resolve = family(seed)
    g, run = _pair(carried.state_of(scen), cap, max_events, window, eager)
    outs = drive(g, run, scen["ticks"], scen["tte"], resolve, mode, timing=timing)
    if window is not None:
        print("seed %d %s: window ticks %d, fallbacks %d" % ((seed, mode) + g.window_stats()))
    g.close()
    return run, outs


# ------------------------------------------------------------------ §2: the random families
@pytest.mark.parametrize("mode", ["columns", "none"])
@pytest.mark.parametrize("seed", carried.SEEDS["multitick"][1])
def test_carried_random_multitick(seed, mode):
    _run_family(carried.multitick, seed, mode)


@pytest.mark.parametrize("seed", [7, 11, 23, 35])
def test_settled_random_multitick(seed):
    """The same driver reading the whole state every tick (the suite's habit): the stale
    entries are cleared before every launch."""
    _run_family(carried.multitick, seed, "settled")


@pytest.mark.parametrize("mode", ["columns", "none"])
@pytest.mark.parametrize("seed", carried.SEEDS["any_entry"][1])
def test_carried_random_results_any_entry(seed, mode):
    """Results naming any log entry: another worker's, a completed, a redistributed (stale)
    one, the same entry twice in a tick."""
    _run_family(carried.any_entry, seed, mode)


@pytest.mark.parametrize("mode", ["columns", "none"])
@pytest.mark.parametrize("seed", carried.SEEDS["window"][1])
def test_carried_window_random(seed, mode):
    _run_family(carried.window, seed, mode, window=1)


@pytest.mark.parametrize("mode", ["columns", "none"])
@pytest.mark.parametrize("seed", carried.SEEDS["window_eager"][1])
def test_carried_window_random_eager(seed, mode):
    _run_family(carried.window, seed, mode, window=1, eager=True)


def test_none_mode_launches_no_commit_of_its_own():
    """Message ticks on the linked-list path, nothing read in between: every commit rides in
    the next tick's k_ev_link, and nothing settles the log -- no "commit" and no "settle"
    stage between the first tick and the last."""
    scen, cap, max_events, resolve = carried.multitick(10)
    ticks = scen["ticks"]
    # (a tick without messages after one with messages launches the commit on its own)
    assert all(len(tk["ev_kind"]) > 0 for tk in ticks[1:])
    g, run = _pair(carried.state_of(scen), cap, max_events)
    timing = {}
    outs = drive(g, run, ticks, scen["tte"], resolve, "none", timing=timing)
    assert run.ticks_with_stale >= 3 and sum(len(b["orphans"]) for _, b in outs[:-1]) > 0
    assert timing["ev_link"][1] >= len(ticks) - 1, timing
    assert "commit" not in timing and "settle" not in timing, timing
    g.close()


# ------------------------------------------------------------------ §3: other launch sequences
PATHS = {
    "sorted": dict(ev_ll=0),                       # radix sort, atomicExch on ctag, lseq-free step
    "plan_gp0": dict(plan=1, gp=0),
    "plan_gp1": dict(plan=1, gp=1),
    "chunked_emit": dict(plan=2),
    "logscan": dict(logscan=1),
    "split_slots": dict(logscan=0, split_slots=1),
}


@pytest.mark.parametrize("seed", carried.SEEDS["paths"][1])
@pytest.mark.parametrize("path", sorted(PATHS))
def test_carried_other_paths(monkeypatch, path, seed):
    for k, v in PATHS[path].items():
        monkeypatch.setitem(TEST_PATHS, k, v)
    _run_family(carried.multitick, seed, "none")


@pytest.mark.parametrize("seed", carried.SEEDS["window_wtiles"][1])
def test_carried_window_four_slot_tiles(monkeypatch, seed):
    monkeypatch.setitem(TEST_PATHS, "wtiles", 4)
    _run_family(carried.window, seed, "none", window=1)


def _window_stream(mode, eager, W=8192, T=512, n_ticks=20, dt=0.75, trace=None):
    """A stream that stays at fill level 0 (window ticks) for longer than the timeout, shaped
    tick by tick from what the oracle has seen.  Seven workers in eight are heartbeated round
    robin (every tenth tick) and live; the eighth kind is mortal and expires over the first
    10 s.  Each tick: the results and joins of synth.stream_ticks; half of the joins become
    re-registrations of dead mortal workers that stale entries name -- half of those then
    stay silent and expire again -- and 40 results of the other half name their stale entries."""
    st = synth.zipf_state(W=W, seed=12, dead_frac=0.0)
    base = synth.stream_ticks(st, n_ticks=n_ticks, seed=19, tasks_per_tick=T, results_per_tick=T // 2, dt=dt,
                              hb_frac=0.0002, join_frac=0.004)
    rng = np.random.default_rng(5)
    count = dict(rejoins=0, aimed=0)
    slots_all = np.arange(W)
    mortal = slots_all % 8 == 0
    talks = (slots_all // 8) % 2 == 0      # the re-registered mortal workers that send results
    st["hb"][~mortal] = 1000.0 - 2.0 * rng.random(int((~mortal).sum()))  # fresh enough for their first turn

    def shaped(t, tk):
        def make(run):
            ex = run.o.export()
            named = np.array(sorted(s for s, v in run.stale.items() if v and mortal[s]), np.int64)
            gone = named[ex["reg"][named] == 0] if len(named) else named
            back = named[(ex["reg"][named] == 1) & talks[named]] if len(named) else named
            keep = tk["ev_kind"] != EV_HB
            kind, slot, val, seq = (tk[k][keep] for k in ("ev_kind", "ev_slot", "ev_val", "ev_seq"))
            slot = slot.copy()
            joins = np.nonzero(kind == EV_REG)[0]
            if len(gone):
                j = joins[: len(joins) // 2]
                slot[j] = rng.choice(gone, len(j))
                count["rejoins"] += len(j)
            hbs = slots_all[~mortal & (slots_all % 10 == t % 10)]
            res = rng.choice(back, 40) if len(back) else np.zeros(0, np.int64)
            res_seq = np.array([run.stale[int(s)][rng.integers(0, len(run.stale[int(s)]))] for s in res], np.int64)
            count["aimed"] += len(res)
            kind = np.concatenate([kind, np.full(len(hbs), EV_HB), np.full(len(res), EV_RES)]).astype(np.uint8)
            slot = np.concatenate([slot, hbs, res]).astype(np.int32)
            val = np.concatenate([val, np.zeros(len(hbs) + len(res), np.int32)]).astype(np.int32)
            seq = np.concatenate([seq, np.full(len(hbs), -1), res_seq]).astype(np.int64)
            perm = rng.permutation(len(kind))
            ts = np.sort(tk["now"] - dt * rng.random(len(kind)))
            return dict(now=tk["now"], n_new=tk["n_new"], ev_kind=kind[perm], ev_slot=slot[perm], ev_val=val[perm],
                        ev_ts=ts, ev_seq=seq[perm])
        return make

    cap = 3 * len(st["log"]) + 2 * n_ticks * T + 16
    g, run = _pair(st, cap, max_events=2048, window=1, eager=eager, purge_mode=2)
    outs = drive(g, run, [shaped(t, tk) for t, tk in enumerate(base)], TTE, _given_seq, mode, aim=False)
    if trace is not None:
        trace.extend((a["result"]["fill_level"], a["result"]["queue_len"], len(b["orphans"]), len(b["evicted"]))
                     for a, b in outs)
    wt, fb = g.window_stats()
    g.close()
    return wt, fb, count, run


@pytest.mark.parametrize("mode", ["columns", "none"])
@pytest.mark.parametrize("eager", [False, True], ids=["deferred", "eager"])
def test_carried_window_stream(mode, eager):
    """Window ticks on carried state (the random window scenarios mostly run general ticks and
    fallbacks)."""
    wt, fb, count, run = _window_stream(mode, eager)
    print("window ticks %d, fallbacks %d, %r, re-deaths %d" % (wt, fb, count, run.redeaths))
    # (the oracle alone gives 304 re-registrations, 720 aimed results and 31 deaths, with
    # orphans, of slots that older stale entries name)
    assert count["rejoins"] >= 250 and count["aimed"] >= 600 and run.redeaths >= 26, (count, run.redeaths)
    assert wt >= 10, "window ticks: %d (fallbacks %d)" % (wt, fb)


def test_carried_window_stream_four_slot_tiles(monkeypatch):
    """... with four 256-slot tiles per workgroup in the slot purge of k_ev_apply_ll."""
    monkeypatch.setitem(TEST_PATHS, "wtiles", 4)
    wt, fb, count, run = _window_stream("none", False)
    assert wt >= 10 and run.redeaths >= 26, (wt, fb, run.redeaths)


def test_carried_large_table():
    """Past 128 K slots (no died bitmap in LDS, lazily written post records, the touched-slot
    list of the deaths): churn_ticks' event mix at about 2000 messages per tick, a clock that
    advances 3 s per tick so that workers die, rejoin and die again, results aimed at the
    rejoined workers' stale entries; outputs every tick, the state at the end."""
    W, n_ticks, dt, T = (1 << 17) + 5, 5, 3.0, 4096
    st = synth.zipf_state(W=W, seed=4, dead_frac=0.05)
    rng = np.random.default_rng(77)
    # dead at the first message (hb = now - 10.5).  400 of them rejoin in tick 0 and are served
    # first (a register moves to the front): `silent` sends nothing more and expires again in
    # tick 3 or 4, `talking` sends results from tick 1 on; 200 more rejoin in tick 1
    dead = np.nonzero(st["hb"] == st["hb"].min())[0]
    assert len(dead) > 2000 and np.isin(st["log"], dead[:600]).sum() > 100
    silent, talking = dead[:200], dead[200:400]
    ticks, now = [], 1000.0
    for t in range(n_ticks):
        prev, now = now, now + dt
        joins = dead[:400] if t == 0 else dead[400:600] if t == 1 else rng.choice(dead[600:], 200)
        hbs = rng.choice(dead[600:], 800)
        res = np.concatenate([rng.choice(talking, 500) if t else rng.choice(dead[600:], 500),
                              rng.choice(dead[600:], 500)])
        kinds = np.concatenate([np.full(len(joins), EV_REG), np.full(len(hbs), EV_HB), np.full(len(res), EV_RES)])
        slots = np.concatenate([joins, hbs, res])
        vals = np.concatenate([rng.integers(1, 33, len(joins)), np.zeros(len(hbs) + len(res), np.int64)])
        perm = rng.permutation(len(kinds))
        E = len(kinds)
        ticks.append(dict(now=now, n_new=T, ev_kind=kinds[perm].astype(np.uint8), ev_slot=slots[perm].astype(np.int32),
                          ev_val=vals[perm].astype(np.int32), ev_ts=np.sort(prev + dt * rng.random(E)),
                          ev_pick=rng.integers(0, 2 ** 31, E).astype(np.uint32)))

    def resolve(tk, log, head):  # one of the sender's in-flight entries (sorted once per tick)
        order = np.argsort(log, kind="stable")
        sl = log[order]
        seq = np.full(len(tk["ev_kind"]), -1, np.int64)
        for i in np.nonzero(tk["ev_kind"] == EV_RES)[0]:
            lo, hi = np.searchsorted(sl, tk["ev_slot"][i]), np.searchsorted(sl, tk["ev_slot"][i], side="right")
            if hi > lo:
                seq[i] = order[lo + tk["ev_pick"][i] % (hi - lo)]
        return seq

    cap = 2 * len(st["log"]) + n_ticks * T + 16
    g, run = _pair(st, cap, max_events=4096, purge_mode=2)
    outs = drive(g, run, ticks, 10.0, resolve, "none")
    # the silent ones died again, with entries of both registrations in the log
    again = np.isin(silent, np.concatenate([b["evicted"] for _, b in outs[2:]]))
    assert again.sum() >= 100, again.sum()
    assert run.redeaths >= 100 and run.aimed >= 100, (run.redeaths, run.aimed)
    g.close()


# ------------------------------------------------------------------ §4: directed cases
def _st(free, hb, queue, log, epoch=None, reg=None):
    W = len(free)
    return dict(reg=np.ones(W, np.uint8) if reg is None else np.asarray(reg, np.uint8),
                free=np.asarray(free, np.int32), hb=np.asarray(hb, np.float64),
                epoch=np.zeros(W, np.uint32) if epoch is None else np.asarray(epoch, np.uint32),
                queue=np.asarray(queue, np.int32), log=np.asarray(log, np.int32))


def _tk(now, events=(), n_new=0):
    """events: (kind, slot, val, ts, seq) in arrival order."""
    ev = list(events)
    col = lambda j, dt: np.asarray([e[j] for e in ev], dt)
    return dict(now=float(now), n_new=int(n_new), ev_kind=col(0, np.uint8), ev_slot=col(1, np.int32),
                ev_val=col(2, np.int32), ev_ts=col(3, np.float64), ev_seq=col(4, np.int64),
                ev_pick=np.zeros(len(ev), np.uint32))


def _given_seq(tk, log, head):
    return tk["ev_seq"].copy()


def _directed(st, ticks, cap=256, mode="none"):
    g, run = _pair(st, cap, max_events=64)
    outs = drive(g, run, ticks, TTE, _given_seq, mode, aim=False)
    g.close()
    return run, [b for _, b in outs]


def test_die_reregister_die():
    """a. Slot 0 holds 3 in-flight entries and expires; it registers again, is given new
    tasks and expires again: the second death's orphans are exactly the new entries."""
    st = _st(free=[0, 8], hb=[989.0, 999.0], queue=[1], log=[0, 1, 0, 0])
    hb1 = lambda ts: (EV_HB, 1, 0, ts, -1)
    run, b = _directed(st, [
        _tk(1000.0, [hb1(999.5)]),                                  # 0 dies: [0, 2, 3] -> slot 1
        _tk(1001.0, [(EV_REG, 0, 4, 1000.5, -1), hb1(1000.75)], 5),  # 0, 1, 0, 1, 0: entries 7, 9, 11
        _tk(1005.0, [hb1(1004.5)]),
        _tk(1012.0, [hb1(1011.5)]),                                  # 1012 - 1000.5 > 10
    ])
    assert list(b[0]["orphans"]) == [0, 2, 3] and list(b[0]["evicted"]) == [0]
    assert list(b[1]["assign"]) == [0, 1, 0, 1, 0]
    assert list(b[3]["evicted"]) == [0]
    assert list(b[3]["orphans"]) == [7, 9, 11]      # fewer than the 6 entries that ever named it
    assert sorted(run.stale[0]) == [0, 2, 3, 7, 9, 11]


def test_epoch_boundary():
    """b. The log's last entry H - 1 is slot 0's, which expires while nobody has capacity: the
    orphan stays pending and the head stays H.  Slot 0 registers with one process and receives
    the task as entry H, equal to its epoch; when it expires again the orphans are [H], never
    H - 1."""
    st = _st(free=[0, 0], hb=[989.0, 999.0], queue=[], log=[1, 0])
    H = 2
    hb1 = lambda ts: (EV_HB, 1, 0, ts, -1)
    run, b = _directed(st, [
        _tk(1000.0, [hb1(999.5)]),
        _tk(1001.0, [(EV_REG, 0, 1, 1000.5, -1), hb1(1000.75)]),
        _tk(1011.0, [hb1(1010.75)]),
    ])
    assert list(b[0]["orphans"]) == [H - 1] and len(b[0]["assign"]) == 0
    assert list(b[1]["assign"]) == [0] and len(b[1]["orphans"]) == 0
    assert list(b[2]["evicted"]) == [0] and list(b[2]["orphans"]) == [H]
    ex = run.o.export()
    assert ex["head"] == H + 1 and list(ex["log"]) == [1, -1, -1]


def _result_on_stale(first_tick_result):
    """Slot 0 dies with entries 0 and 1 (redistributed to slot 1 as 3 and 4) and sends a
    result naming entry 0 -- in the tick of its death, after it (d), or re-registered, two
    ticks later (c)."""
    st = _st(free=[0, 8, 0], hb=[989.5, 999.0, 999.0], queue=[1], log=[0, 0, 1])
    hb = lambda ts: [(EV_HB, 1, 0, ts, -1), (EV_HB, 2, 0, ts, -1)]
    if first_tick_result:
        ticks = [
            # 0 dies at the first message's purge; its result finds no record (reconnect, payload
            # dropped, new record with epoch = head and no free process)
            _tk(1000.0, hb(999.75) + [(EV_RES, 0, 0, 999.875, 0)]),
            # the same result again: free 0 -> 1, to the back of the queue; one task each
            _tk(1001.0, hb(1000.25) + [(EV_RES, 0, 0, 1000.5, 0)] + hb(1001.0), 2),
            _tk(1011.0, hb(1010.75)),                                # 0 expires: its new entry only
        ]
    else:
        ticks = [
            _tk(1000.0, hb(999.75)),
            _tk(1001.0, [(EV_REG, 0, 2, 1000.25, -1)] + hb(1000.5), 1),   # entry 5 -> slot 0
            _tk(1002.0, hb(1001.25) + [(EV_RES, 0, 0, 1001.5, 0)]),      # names its stale entry 0
            _tk(1002.5, hb(1002.25)),
        ]
    return _directed(st, ticks)


def test_result_names_stale_entry_of_reregistered_slot():
    """c. The free count still rises, nothing is completed, the redistributed task's new entry
    on slot 1 is untouched, and both slots' in-flight counts equal the oracle's (the final
    compare reads them before anything settles the log)."""
    run, b = _result_on_stale(False)
    assert list(b[0]["orphans"]) == [0, 1] and list(b[0]["assign"]) == [1, 1]
    assert list(b[1]["assign"]) == [0]
    ex = run.o.export()
    assert list(ex["log"]) == [-1, -1, 1, 1, 1, 0]     # 3, 4 (slot 1) and 5 (slot 0) still in flight
    assert ex["free"][0] == 2 and ex["epoch"][0] == 5   # 2 - 1 task + 1 result


def test_result_names_entry_in_the_tick_of_its_slots_death():
    """d. The entry is live at tick start and its slot dies before the result arrives: it is
    redistributed, not completed; the record the result creates owns nothing older."""
    run, b = _result_on_stale(True)
    assert list(b[0]["orphans"]) == [0, 1] and list(b[0]["reconnect"]) == [0, 0, 1]
    assert len(b[0]["evicted"]) == 0                    # re-created in the same tick
    assert list(b[1]["assign"]) == [1, 0] and not b[1]["reconnect"].any()
    assert list(b[2]["evicted"]) == [0] and list(b[2]["orphans"]) == [6]


def test_result_after_death_and_reregistration_in_one_tick():
    """Slot 0, re-registered once already (stale entries 0 and 1, live entry 5 = its epoch),
    expires, registers again and sends two results in one tick: the one naming entry 5 -- in
    flight at tick start -- completes it, so it is no orphan; the one naming entry 0 completes
    nothing; both raise the free count."""
    st = _st(free=[0, 8, 0], hb=[989.5, 999.0, 999.0], queue=[1], log=[0, 0, 1])
    hb = lambda ts: [(EV_HB, 1, 0, ts, -1), (EV_HB, 2, 0, ts, -1)]
    run, b = _directed(st, [
        _tk(1000.0, hb(999.75)),
        _tk(1001.0, [(EV_REG, 0, 2, 1000.25, -1)] + hb(1001.0), 2),      # 5 -> slot 0, 6 -> slot 1
        _tk(1011.0, hb(1010.5) + [(EV_REG, 0, 1, 1010.75, -1), (EV_RES, 0, 0, 1010.875, 5),
                                  (EV_RES, 0, 0, 1010.875, 0)]),
        _tk(1011.5, hb(1011.25), 1),
    ])
    assert list(b[1]["assign"]) == [0, 1]
    assert len(b[2]["orphans"]) == 0 and len(b[2]["evicted"]) == 0
    ex = run.o.export()
    assert list(ex["log"]) == [-1, -1, 1, 1, 1, -1, 1, 0] and ex["epoch"][0] == 7 and ex["free"][0] == 2


def test_unknown_id_record_with_stale_entries():
    """e. Slot 0 has stale entries and no record; a heartbeat from it creates one (status
    reconnect, epoch = head); when that expires there are no orphans."""
    st = _st(free=[0, 8], hb=[989.0, 999.0], queue=[1], log=[0, 1, 0])
    hb1 = lambda ts: (EV_HB, 1, 0, ts, -1)
    run, b = _directed(st, [
        _tk(1000.0, [hb1(999.5)]),
        _tk(1001.0, [(EV_HB, 0, 0, 1000.5, -1), hb1(1001.0)]),
        _tk(1011.0, [hb1(1010.75)]),                                 # 1010.75 - 1000.5 > 10
    ])
    assert list(b[0]["orphans"]) == [0, 2] and list(b[0]["evicted"]) == [0]
    assert list(b[1]["reconnect"]) == [1, 0] and len(b[1]["evicted"]) == 0
    assert list(b[2]["evicted"]) == [0] and len(b[2]["orphans"]) == 0
    assert run.stale[0] == [0, 2]


def test_resort_rerun_with_stale_entries():
    """f. 17 results for slot 0 in one tick (more than the linked lists hold: the tick reruns
    through the sort): several name stale entries, two the same live entry."""
    st = _st(free=[0, 4], hb=[989.0, 999.0], queue=[1], log=[0, 0, 0, 0])
    hb1 = lambda ts: (EV_HB, 1, 0, ts, -1)
    seqs = [0, 8, 1, 2, 8, 3, -1, 0, 9, 1, 99, 4, 10, 2, 5, -1, 3]
    assert len(seqs) == 17
    g, run = _pair(st, 256, max_events=64)
    ticks = [
        _tk(1000.0, [hb1(999.5)]),                                   # 0 dies: 0..3 -> slot 1 as 4..7
        _tk(1001.0, [(EV_REG, 0, 6, 1000.5, -1), hb1(1000.75)], 5),  # slot 1 is full: 8..12 -> slot 0
        _tk(1002.0, [hb1(1001.25)] + [(EV_RES, 0, 0, 1001.5 + i / 64.0, q) for i, q in enumerate(seqs)] +
            [hb1(1002.0)]),
        _tk(1012.0, [hb1(1011.875)]),                                # 1011.875 - 1001.75 > 10: 0 expires
    ]
    outs = drive(g, run, ticks, TTE, _given_seq, "none", aim=False)
    b = [x for _, x in outs]
    assert list(b[0]["orphans"]) == [0, 1, 2, 3] and list(b[1]["assign"]) == [0] * 5
    if TEST_PATHS.get("ev_ll", 1) != 0:
        assert outs[2][0]["result"]["reruns"] >= 1
    assert list(b[3]["orphans"]) == [11, 12]    # 8, 9, 10 completed, nothing below the epoch
    g.close()


def test_nonzero_initial_epoch():
    """g. A state loaded with non-zero epochs and entries of the same slot on both sides of
    them: the load drops the older ones (read back at once, equal to the oracle's), a death
    orphans only the entries at or above the epoch."""
    st = _st(free=[1, 8, 1, 0], hb=[989.0, 999.0, 999.0, 999.0], queue=[1], epoch=[3, 0, 2, 0],
             log=[2, 0, 0, 2, 0, 0, 1, 0])
    g, run = _pair(st, 256, max_events=64)
    sg, so = g.read_state(), run.o.export()
    assert list(so["log"]) == [-1, -1, -1, 2, 0, 0, 1, 0]
    for k in ("reg", "free", "hb", "epoch", "queue", "log"):
        np.testing.assert_array_equal(sg[k], so[k], err_msg=k)
    np.testing.assert_array_equal(g.inflight(), [3, 1, 1, 0])
    hb = lambda ts: [(EV_HB, s, 0, ts, -1) for s in (1, 2, 3)]
    outs = drive(g, run, [_tk(1000.0, hb(999.5)), _tk(1001.0, hb(1000.5), 2)], TTE, _given_seq, "none", aim=False)
    assert list(outs[0][1]["orphans"]) == [4, 5, 7] and list(outs[0][1]["evicted"]) == [0]
    g.close()


def test_lazy_off_and_on_with_stale_entries():
    """h. fb_set_path("lazy", 0) while stale entries exist (it settles the log), three ticks
    with eager clears, then lazy again for three more."""
    scen = synth.random_scenario(1011, W=300, n_ticks=9, max_events=2000, max_new=3000)
    g, run = _pair(carried.state_of(scen), len(scen["init_log"]) + 60000)
    tk = scen["ticks"]
    drive(g, run, tk[:3], scen["tte"], carried.resolve_own, "none", last=False)
    n0 = sum(len(v) for v in run.stale.values())
    assert n0 > 0
    g.set_path("lazy", 0)
    drive(g, run, tk[3:6], scen["tte"], carried.resolve_own, "none", t0=3)
    assert sum(len(v) for v in run.stale.values()) > n0     # deaths with eager clears too
    g.set_path("lazy", 1)
    drive(g, run, tk[6:], scen["tte"], carried.resolve_own, "none", t0=6)
    assert run.aimed > 0
    g.close()


DIRECTED = [test_die_reregister_die, test_epoch_boundary, test_result_names_stale_entry_of_reregistered_slot,
            test_result_names_entry_in_the_tick_of_its_slots_death,
            test_result_after_death_and_reregistration_in_one_tick, test_unknown_id_record_with_stale_entries,
            test_resort_rerun_with_stale_entries, test_nonzero_initial_epoch]


@pytest.mark.parametrize("path", ["sorted", "plan_gp1", "logscan", "split_slots"])
@pytest.mark.parametrize("case", DIRECTED, ids=[f.__name__[5:] for f in DIRECTED])
def test_directed_cases_other_paths(monkeypatch, case, path):
    """The directed cases through the launch sequences of other table sizes."""
    for k, v in PATHS[path].items():
        monkeypatch.setitem(TEST_PATHS, k, v)
    case()


# ------------------------------------------------------------------ §6: what settles the log
def test_settle_contract():
    """After a committed tick with orphans, read_state(with_log=False) and inflight() launch
    no "settle" stage (k_log_normalize), read_state() launches one, a second read_state()
    none; fb_set_path("lazy", 0) with stale entries present launches one."""
    st = synth.zipf_state(W=4096, seed=3, dead_frac=0.05)
    g = GpuBalancer(4096, 3 * len(st["log"]) + 4096)
    g.load(st)
    g.timing_enable(True)

    def launches(stage):
        return int(g.timing_read().get(stage, (0.0, 0))[1])

    a = g.tick(1000.0, TTE, n_pending=100)
    assert len(a["orphans"]) > 0
    g.timing_read()
    g.read_state(with_log=False)
    g.inflight()
    kt = g.timing_read()
    assert "settle" not in kt and int(kt["commit"][1]) == 1, kt   # the deferred commit, flushed
    g.read_state()
    assert launches("settle") == 1
    g.read_state()
    assert launches("settle") == 0
    # stale entries again: 5 % more of the workers expire
    a = g.tick(1009.9, TTE, n_pending=100)
    assert len(a["orphans"]) > 0
    g.timing_read()
    g.set_path("lazy", 0)
    assert launches("settle") == 1
    g.set_path("lazy", 0)
    g.read_state()
    assert launches("settle") == 0
    g.close()
