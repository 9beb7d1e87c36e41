"""Launches that carry results and are never committed, driven from the oracle alone (no
GPU here).

A context that does not defer its clears (deque, one GPU past 128 K workers, sharded) clears
the log entries a launch's results complete in place, at launch; a launch that is abandoned
or whose wait fails must leave them in flight (k_log_undo).  A case is: an initial state,
committed ticks before (`pre`: they leave stale entries in a heartbeat context's log), the
launch that is never committed, the committed ticks after it, and -- on heartbeat contexts --
a tick at which every worker has expired, so that every entry still in flight is an orphan.
The oracle never sees the abandoned launch: its outputs and its final state are what the
device must give.  tests/test_gpu_abandoned.py replays the cases; tests/
test_abandoned_coverage.py states what each of them reaches.
"""
from collections import defaultdict

import numpy as np

import carried
from faasbal import synth
from oracle import DequeOracle, Oracle

REG, RECON, HB, RES = synth.EV_REGISTER, synth.EV_RECONNECT, synth.EV_HEARTBEAT, synth.EV_RESULT
TTE = 10.0
H_LARGE_W = (1 << 17) + 5   # the first table size without deferred clears


class Run:
    """An oracle, the tasks carried from tick to tick and -- as carried.OracleRun -- the
    entries each committed tick redistributed (what a heartbeat context's log still holds)."""

    def __init__(self, st, log_cap, deque=False, purge_mode=1):
        W = len(st["reg"])
        self.deque = deque
        self.o = DequeOracle(W, log_cap) if deque else Oracle(W, log_cap, purge_mode=purge_mode)
        self.o.load(st["reg"], st["free"], st["hb"], st["epoch"], st["queue"], st["log"])
        self.stale = defaultdict(list)
        self.carried = 0

    def export(self):
        return self.o.export()

    def tick(self, args, track=True):
        before = self.o.export()["log"] if track else None
        b = self.o.tick(*args)
        if track:
            for q in b["orphans"]:
                self.stale[int(before[q])].append(int(q))
        self.carried = args[-1] + len(b["orphans"]) - len(b["assign"])
        return b


class Case:
    """steps: ("tick" | "abandon", args) in launch order; want[i]: the oracle's outputs of a
    "tick" step (None for "abandon"); final: the oracle's state after the last step.
    targets: the live entries the abandoned launches' results are meant to complete (one
    array per abandoned launch); n_dup / n_stale / n_foreign: results that repeat a target,
    name a stale entry, name another worker's live entry (per abandoned launch)."""

    def __init__(self, name, st, log_cap, max_events, deque, purge_mode=1):
        self.name, self.st, self.log_cap, self.max_events, self.deque = name, st, log_cap, max_events, deque
        self.purge_mode = purge_mode
        self.steps, self.want = [], []
        self.targets, self.n_dup, self.n_stale, self.n_foreign = [], [], [], []
        # of all targets: live in the committed state at the launch / still in flight after
        # the committed ticks that follow / among the death tick's orphans
        self.live_named = self.in_flight_after = self.orphaned = None
        self.death = None      # index of the death tick in steps (heartbeat cases)
        self.at_launch = None  # the committed state the launch(es) with results ran on
        self.final = None

    def run(self):
        return Run(self.st, self.log_cap, self.deque, self.purge_mode)


# ------------------------------------------------------------------ batches
def _owned(log):
    """(order, sorted slots): the entries of slot s are order[lo:hi] of searchsorted."""
    order = np.argsort(log, kind="stable")
    return order, log[order]


def results_batch(rng, ex, targets, n_dup, stale, n_foreign, prev, now):
    """The messages of a launch whose results name `targets` (live entries of ex["log"]),
    n_dup of them twice, every (slot, entry) of `stale` (a slot without a record registers
    first) and n_foreign live entries of other workers.  Arrival order is random; times
    ascend in (prev, now]."""
    log = ex["log"]
    ev = [(RES, int(log[q]), 0, int(q)) for q in targets]
    ev += [(RES, int(log[q]), 0, int(q)) for q in rng.choice(targets, n_dup, replace=False)]
    senders = log[targets]
    others = np.unique(senders)
    for q in rng.choice(targets, n_foreign, replace=False):
        k = int(rng.integers(0, len(others)))
        ev.append((RES, int(others[k] if others[k] != log[q] else others[k - 1]), 0, int(q)))
    key = list(rng.random(len(ev)))
    for s, q in stale:
        k = rng.random()
        if not ex["reg"][s]:
            ev.append((REG, int(s), 1, -1))
            key.append(k - 1e-9)
        ev.append((RES, int(s), 0, int(q)))
        key.append(k)
    order = np.argsort(np.asarray(key), kind="stable")
    ts = np.sort(prev + (now - prev) * rng.integers(1, 65, len(ev)) / 64.0)
    col = lambda j, dt: np.asarray([ev[i][j] for i in order], dt)
    return col(0, np.uint8), col(1, np.int32), col(2, np.int32), ts, col(3, np.int64)


def other_messages(rng, ex, n_hb, n_res, avoid, prev, now):
    """Heartbeats and results (each naming one of its sender's live entries) of registered
    workers outside `avoid`."""
    ok = np.flatnonzero(ex["reg"].astype(bool) & ~np.isin(np.arange(len(ex["reg"])), avoid))
    order, sl = _owned(ex["log"])
    ev = [(HB, int(s), 0, -1) for s in rng.choice(ok, n_hb)]
    for s in rng.choice(ok, n_res):
        lo, hi = np.searchsorted(sl, s), np.searchsorted(sl, s, side="right")
        ev.append((RES, int(s), 0, int(order[lo + rng.integers(0, hi - lo)]) if hi > lo else -1))
    perm = rng.permutation(len(ev))
    ts = np.sort(prev + (now - prev) * rng.integers(1, 65, len(ev)) / 64.0)
    col = lambda j, dt: np.asarray([ev[i][j] for i in perm], dt)
    return col(0, np.uint8), col(1, np.int32), col(2, np.int32), ts, col(3, np.int64)


def _stale_pairs(rng, run, ex, n):
    """Up to n (slot, stale entry): entries a committed tick redistributed, which a heartbeat
    context's log still holds; the slot re-registered since (entry < epoch) or has no record."""
    pairs = [(s, q) for s, qs in sorted(run.stale.items()) for q in qs
             if not ex["reg"][s] or q < int(ex["epoch"][s])]
    if len(pairs) > n:
        pairs = [pairs[i] for i in np.sort(rng.choice(len(pairs), n, replace=False))]
    return pairs


def _finish(case, run, at_abandon):
    """The conditions of a case, from the oracle alone, and its final state."""
    T = np.concatenate(case.targets) if case.targets else np.zeros(0, np.int64)
    log0, reg0, ep0 = at_abandon["log"], at_abandon["reg"], at_abandon["epoch"]
    s0 = log0[T]
    case.live_named = int(np.sum((s0 >= 0) & (reg0[np.maximum(s0, 0)] == 1) &
                                 (T >= ep0[np.maximum(s0, 0)].astype(np.int64))))
    case.at_launch = at_abandon
    case.final = run.export()
    if case.death is not None:
        case.orphaned = int(np.isin(T, case.want[case.death]["orphans"]).sum())
    return case


# ------------------------------------------------------------------ H-large and zipf deque
def _directed(name, st, log_cap, max_events, deque, variant, n_targets, n_dup, n_stale, n_foreign,
              pending=4096, n_other=(500, 300), purge_mode=1):
    """variant: "one" abandoned launch; "two" in a row, with different targets; "committed":
    the launch with results is committed (the oracle sees it)."""
    case = Case(name + "-" + variant, st, log_cap, max_events, deque, purge_mode)
    run, rng = case.run(), np.random.default_rng(1)
    none = ([], [], [], [], [])
    # (the loaded heartbeats lie in (now - 9.9, now]: nobody else expires before the death tick)
    STEP = 1.0 / 64

    def commit(args, track=True):
        case.steps.append(("tick", args))
        case.want.append(run.tick(args, track))

    # the tick of the issue's figures: no messages, the dead of the loaded state expire
    commit((1000.0, TTE, *none, pending))
    ex = run.export()
    alive = ex["reg"].astype(bool) & (st["hb"] > st["hb"].min()) if not deque else ex["reg"].astype(bool)
    cand = np.flatnonzero((ex["log"] >= 0) & alive[np.maximum(ex["log"], 0)])
    picks = [rng.choice(cand, n_targets, replace=False)]
    if variant == "two":
        picks.append(np.random.default_rng(2).choice(cand, n_targets, replace=False))
    stale = _stale_pairs(rng, run, ex, n_stale)
    now = 1000.0
    for T in picks:
        prev, now = now, now + STEP
        T = np.sort(T)
        args = (now, TTE, *results_batch(rng, ex, T, n_dup, stale, n_foreign, prev, now), run.carried + 100)
        case.targets.append(T)
        case.n_dup.append(n_dup)
        case.n_stale.append(len(stale))
        case.n_foreign.append(n_foreign)
        if variant == "committed":
            commit(args)
        else:
            case.steps.append(("abandon", args))
            case.want.append(None)
    avoid = np.unique(ex["log"][np.concatenate(picks)])
    for k in range(1 if variant == "two" else 2):
        prev, now = now, now + STEP
        exk = run.export()
        commit((now, TTE, *other_messages(rng, exk, n_other[0] >> k, n_other[1] >> k, avoid, prev, now),
                run.carried + 1000))
    after = run.export()["log"]
    T = np.concatenate(case.targets)
    case.in_flight_after = int(np.sum(after[T] == ex["log"][T]))
    if not deque:
        case.death = len(case.steps)
        commit((now + 2 * TTE, TTE, *none, run.carried), track=False)
    return _finish(case, run, ex)


def h_large(variant="one"):
    """One GPU past 128 K workers: clears in place, lazily cleared orphans."""
    st = synth.zipf_state(W=H_LARGE_W, seed=4, dead_frac=0.05)
    return _directed("h-large", st, 2 * len(st["log"]) + 50000, 4096, False, variant, 2000, 200, 100, 50,
                     purge_mode=2)


def d_zipf(variant="one"):
    """A deque context (no liveness, no stale entries)."""
    st = synth.zipf_deque_state(W=4096, seed=5, dup_frac=0.1)
    return _directed("d-zipf", st, 2 * len(st["log"]) + 50000, 4096, True, variant, 1000, 100, 0, 50)


# ------------------------------------------------------------------ the random families
def _family(name, scen, log_cap, max_events, deque, n_pre, n_after, variant="one", frac=0.5):
    """scen's first n_pre ticks committed, the launch(es) with results, n_after more ticks, and
    (not deque) a tick at which everybody has expired.  variant as _directed's.  The targets:
    `frac` of the entries live after the first n_pre ticks that the ticks after them leave in
    flight in an oracle that never sees the launch (their results name only their senders' own
    entries, by the oracle's log: carried.resolve_own); "two": a second draw of them."""
    case = Case(name, carried.state_of(scen), log_cap, max_events, deque)
    tte = scen["tte"] if not deque else TTE
    pre, post = scen["ticks"][:n_pre], scen["ticks"][n_pre:n_pre + n_after]

    def args_of(run, tk):
        ex = run.export()
        seq = carried.resolve_own(tk, ex["log"], ex["head"])
        return (tk["now"], tte, tk["ev_kind"], tk["ev_slot"], tk["ev_val"], tk["ev_ts"], seq, run.carried + tk["n_new"])

    # a first pass without the launch: what survives the ticks after it
    scratch = case.run()
    for tk in pre:
        scratch.tick(args_of(scratch, tk))
    ex = scratch.export()
    stale = [] if deque else _stale_pairs(np.random.default_rng(5), scratch, ex, 20)
    for tk in post:
        scratch.tick(args_of(scratch, tk))
    after = scratch.export()
    s0 = ex["log"]
    live = (s0 >= 0) & (ex["reg"][np.maximum(s0, 0)] == 1) & \
        (np.arange(len(s0)) >= ex["epoch"][np.maximum(s0, 0)].astype(np.int64))
    keep = np.flatnonzero(live & (after["log"][:len(s0)] == s0) & (after["reg"][np.maximum(s0, 0)] == 1))
    n = max(1, int(frac * len(keep)))
    picks = [np.sort(np.random.default_rng(3 + k).choice(keep, n, replace=False))
             for k in range(2 if variant == "two" else 1)]

    run, rng = case.run(), np.random.default_rng(3)

    def commit(args, track=True):
        case.steps.append(("tick", args))
        case.want.append(run.tick(args, track))

    for tk in pre:
        commit(args_of(run, tk))
    prev, now = pre[-1]["now"], post[0]["now"]
    for T in picks:
        n_dup, n_foreign = len(T) // 4, len(T) // 8
        args = (now, tte, *results_batch(rng, ex, T, n_dup, stale, n_foreign, prev, now), run.carried)
        case.targets.append(T)
        case.n_dup.append(n_dup)
        case.n_stale.append(len(stale))
        case.n_foreign.append(n_foreign)
        if variant == "committed":
            commit(args)
        else:
            case.steps.append(("abandon", args))
            case.want.append(None)
    for tk in post:
        commit(args_of(run, tk))
    T = np.concatenate(case.targets)
    case.in_flight_after = int(np.sum(run.export()["log"][T] == s0[T]))
    if not deque:
        case.death = len(case.steps)
        commit(args_of(run, synth.empty_tick(post[-1]["now"] + 2 * tte + 1.0)), track=False)
    return _finish(case, run, ex)


H_SMALL_SEEDS = (2, 11)     # carried.multitick: W = 300 and W = 1000, up to 2000 messages a tick
D_SMALL_SEEDS = (1, 2)


def h_small(seed, variant="one"):
    """One GPU, deferred clears (ctag / ev_clr): no entry is touched before the commit."""
    scen, cap, max_events, _ = carried.multitick(seed)
    return _family("h-small-%d-%s" % (seed, variant), scen, cap, max_events, False, 2, 2, variant)


def d_small(seed):
    scen = synth.random_deque_scenario(seed, W=300, n_ticks=5, max_events=400, max_new=200)
    return _family("d-small-%d-one" % seed, scen, len(scen["init_log"]) + 20000, 4096, True, 2, 2)


CASES = {
    "h-large-one": lambda: h_large("one"),
    "h-large-two": lambda: h_large("two"),
    "h-large-committed": lambda: h_large("committed"),
    "d-zipf-one": lambda: d_zipf("one"),
    "d-zipf-two": lambda: d_zipf("two"),
    "d-zipf-committed": lambda: d_zipf("committed"),
    **{"h-small-%d-%s" % (s, v): (lambda s=s, v=v: h_small(s, v)) for s in H_SMALL_SEEDS
       for v in ("one", "two", "committed")},
    **{"d-small-%d-one" % s: (lambda s=s: d_small(s)) for s in D_SMALL_SEEDS},
}

_built = {}


def case(name):
    """The case, built once per process (the oracle's expected outputs are shared)."""
    if name not in _built:
        _built[name] = CASES[name]()
    return _built[name]
