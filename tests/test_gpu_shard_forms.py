"""Sharded ticks back to back across the four phase-2 forms and the fb_set_path knobs.

A sharded tick picks its phase 2 at launch (xrows_mode / plan_tick, csrc/faasbal_plan.h) from
the queue blocks ``nbq = ceil((queue + 2 x messages) / 256)`` and the round-table width R
(32 / 64 / 128 from the last tick's max free count and this tick's registration values; wider
only in a relaunch asked by FB_ERERUN):

    rows     nbq <= 256, R <= 128        rank 0's phase 2 launches: emit
    xplan    nbq >  256, R == 32                                    plan + emit
    recount  nbq >  256, R in {64, 128}                             scan2 + emit
    wide     R > 128                                                scan2 + plan + emit

The forms hand state to each other between ticks (the exchange records' parity and the
``xz_ok`` memset skip, the exchange layout, a second phase 1 after a phase 2 that already
flipped the parity), so a mistake shows in the NEXT tick.  Every test here runs a group of
rank contexts on GPU 0 against the one-table oracle, bit for bit (tests/test_gpu_sharded.py's
_group_tick / _cmp): event status, merged assignments, orphans, evicted slots and the
reassembled state.  The oracle's answers of a scenario are computed once and replayed for
every world size and knob setting.

Inputs are vectorised numpy, every time a multiple of 0.25 (exact liveness subtraction).
The shapes are the smallest that reach xplan and the large-queue recount: more than
256 x 256 = 65 536 queue positions.

Wide directly followed by xplan does not happen by itself: a wide tick saw a free count
beyond 128, fb_tick_commit keeps that tick's max free count as the next tick's hint, so the
tick after a wide one has a 128-row table (rows or recount) and R is back at 32 one tick
later.  Only fb_set_round_hint between the two ticks arranges the pair:
test_wide_then_xplan_by_round_hint does, outside the ladder.  Likewise a registration's
value sizes the table of its own tick (128 rows at most),
so an FB_ERERUN out of an xplan first attempt needs a free count that grew past the table
through results alone: the ladder sends one worker 130 results in one tick.
"""
import functools

import numpy as np
import pytest

import test_gpu_sharded as tgs
from faasbal import synth
from faasbal.balancer import TEST_PATHS
from oracle import Oracle
from test_gpu_sharded import _cmp, _cmp_outputs, _group_tick

pytestmark = pytest.mark.gpu

TTE = 10.0
REG, RECONN, HB, RESULT = synth.EV_REGISTER, synth.EV_RECONNECT, synth.EV_HEARTBEAT, synth.EV_RESULT
FORMS = {(0, 0, 1): "rows", (0, 1, 1): "xplan", (1, 0, 1): "recount", (1, 1, 1): "wide"}
KNOBS = [{"xplan": 0}, {"xself": 0}, {"xcfirst": 0}, {"wfirst": 0}, {"logscan": 1}, {"wtiles": 4},
         {"xself": 0, "xcfirst": 0}]
KNOB_IDS = ["-".join("%s%d" % kv for kv in k.items()) for k in KNOBS]


# ------------------------------------------------------------------------------ inputs
class _Batch:
    """A tick's messages, collected in parts and shuffled into one batch."""

    def __init__(self):
        self.parts = []

    def add(self, kind, slot, val=0, seq=-1):
        slot = np.asarray(slot, np.int32).reshape(-1)
        n = len(slot)
        self.parts.append((np.broadcast_to(np.asarray(kind, np.uint8), (n,)), slot,
                           np.broadcast_to(np.asarray(val, np.int32), (n,)),
                           np.broadcast_to(np.asarray(seq, np.int64), (n,))))

    def events(self, rng, now):
        """(kind, slot, val, ts, seq): shuffled; a random prefix a quarter second before now."""
        if not self.parts:
            return [np.zeros(0, dt) for dt in (np.uint8, np.int32, np.int32, np.float64, np.int64)]
        kind, slot, val, seq = (np.concatenate([p[i] for p in self.parts]) for i in range(4))
        order = rng.permutation(len(kind))
        ts = np.where(np.arange(len(kind)) < rng.integers(0, len(kind) + 1), now - 0.25, now)
        return [kind[order], slot[order], val[order], ts, seq[order]]


def _mixed(rng, st, n, calm=None):
    """n mixed messages against the oracle's state ``st``: heartbeats, results naming live
    log entries, results naming completed or no entries, reconnects and small
    registrations of known ids, and every kind from ids without a record (answered with
    'reconnect').  ``calm``: slots that get no message (the scenario scripts theirs)."""
    b = _Batch()
    k = max(n // 10, 1)
    ok = np.ones(len(st["reg"]), bool)
    if calm is not None:
        ok[calm] = False
    regd, unknown = np.nonzero((st["reg"] == 1) & ok)[0], np.nonzero(st["reg"] == 0)[0]
    log = st["log"]
    live, done = np.nonzero(log >= 0)[0], np.nonzero(log < 0)[0]
    s = rng.choice(live, min(2 * k, len(live)), replace=False)
    s = s[ok[log[s]]]
    b.add(RESULT, log[s], seq=s)
    r = rng.choice(regd, k)
    b.add(RESULT, r, seq=rng.choice(done, len(r)) if len(done) else -1)
    b.add(RESULT, rng.choice(regd, k // 2))
    b.add(RECONN, rng.choice(regd, k), val=rng.integers(0, 6, k))
    b.add(REG, rng.choice(regd, k), val=rng.integers(0, 6, k))
    u = rng.choice(unknown, min(k, len(unknown)), replace=False)
    b.add(rng.choice([RECONN, HB, RESULT], len(u)).astype(np.uint8), u, val=rng.integers(0, 6, len(u)))
    u = rng.choice(unknown, min(k // 2, len(unknown)), replace=False)
    b.add(REG, u, val=rng.integers(0, 6, len(u)))
    b.add(HB, rng.choice(regd, n - sum(len(p[1]) for p in b.parts)))  # (the rest: heartbeats, ~3 in 10)
    return b


def _join(b, rng, st, n):
    """A burst of n registrations of ids without a record, 1..5 processes each."""
    u = np.nonzero(st["reg"] == 0)[0]
    b.add(REG, rng.choice(u, n, replace=False), val=rng.integers(1, 6, n))


def _after_messages(st, cap, now, ev):
    """(c per queue position, orphans) once the tick's messages and purges ran: a scratch
    oracle on a copy of the state, nothing dispatched."""
    o = Oracle(len(st["reg"]), cap)
    o.load(st["reg"], st["free"], st["hb"], st["epoch"], st["queue"], st["log"])
    x = o.tick(now, TTE, *ev, 0, dispatch_limit=0)
    s = o.export()
    return np.maximum(s["free"][s["queue"]], 1).astype(np.int64), len(x["orphans"])


def _tasks_for_level(c, level, part=2):
    """A number of dispatches that ends inside round ``level`` (after 1 / part of it)."""
    lo, hi = int(np.minimum(c, level).sum()), int(np.minimum(c, level + 1).sum())
    assert hi > lo, "no round %d in this queue" % level
    return lo + (hi - lo) // part


class _Scenario:
    """Initial state, the ticks' arguments and the oracle's outputs and state after each."""

    def __init__(self, st, cap):
        self.st, self.cap, self.ticks = st, cap, []
        self.o = Oracle(len(st["reg"]), cap)
        self.o.load(st["reg"], st["free"], st["hb"], st["epoch"], st["queue"], st["log"])
        self.state = self.o.export()
        self.carried = 0

    def tick(self, now, ev, n_new, **note):
        n = self.carried + n_new
        args = (now, TTE, *ev, n)
        out = self.o.tick(*args)
        self.state = self.o.export()
        self.carried = n + len(out["orphans"]) - len(out["assign"])
        self.ticks.append(dict(args=args, out=out, state=self.state, idle=not len(ev[0]) and n == 0, **note))
        return out

    def done(self):
        del self.o  # (replayed from here on)
        return self


class _Replay:
    """The recorded oracle behind Oracle's tick() / export(), for _cmp."""

    def __init__(self, scen):
        self.scen, self.t = scen, -1

    def tick(self, *args):
        self.t += 1
        return self.scen.ticks[self.t]["out"]

    def export(self):
        return self.scen.ticks[self.t]["state"] if self.t >= 0 else self.scen.st


def _bals(scen, world, max_events=4096):
    import torch  # noqa: F401  (loads the HIP runtime before libfaasbal)
    from faasbal.sharded import ShardedBalancer

    bals = []
    try:
        for r in range(world):
            bals.append(ShardedBalancer(r, world, len(scen.st["reg"]), scen.cap, max_events=max_events))
            bals[-1].load(scen.st)
    except BaseException:
        _close(bals)
        raise
    return bals


def _close(bals):
    for b in bals:
        b.close()


# ------------------------------------------------------------------------------ 1. the ladder
LADDER_IDLE = (1, 3, 4, 6, 10, 18)  # ticks without messages and tasks (a quarter second after the last)
LADDER_NOW = [1000.0 + 0.5 * t - 0.25 * sum(i <= t for i in LADDER_IDLE) for t in range(22)]
# the form of every launch of every tick the ladder is written for (a relaunch: two entries)
LADDER_FORMS = [["xplan"], ["xplan"], ["xplan"], ["xplan"], ["xplan"], ["recount"], ["recount"], ["recount"],
                ["xplan"], ["rows"], ["rows"], ["rows"], ["xplan"], ["rows"], ["recount"], ["rows"], ["xplan"],
                ["xplan", "wide"], ["rows"], ["rows", "wide"], ["wide"], ["rows"]]
LADDER_PAIRS = {("rows", "xplan"), ("xplan", "rows"), ("xplan", "recount"), ("recount", "xplan"),
                ("rows", "recount"), ("recount", "rows"), ("wide", "rows"),
                ("xplan", "FB_ERERUN", "wide"), ("rows", "FB_ERERUN", "wide")}


@functools.lru_cache(maxsize=1)
def _ladder():
    """22 ticks that walk one group through every reachable change of form.  The clock
    expires three blocks of workers that never send a heartbeat (B at tick 8, C at 12, D at
    14; 300 more in ticks 0, 2, 5, 9 and 17: orphans right before the idle ticks), bursts of
    registrations grow the queue again, worker X registers with 80 and later 2 processes
    (R = 128 and back), Y with 60 and 2 (R = 64 and back), V gets 130 results in a tick that
    dispatches 40 rounds (FB_ERERUN out of an xplan launch), U registers with 5 000 processes
    in a tick of 140 rounds (FB_ERERUN out of a rows launch).  The expired workers' in-flight
    tasks are redistributed once; those who write again after expiring are answered with
    'reconnect' and start a new registration."""
    rng = np.random.default_rng(20261020)
    W, n0 = 81_000, 72_800
    now = LADDER_NOW
    reg = np.zeros(W, np.uint8)
    reg[:n0] = 1
    free = np.zeros(W, np.int32)
    free[:n0] = rng.integers(1, 6, n0)
    hb = np.zeros(W)
    hb[:n0] = 1000.0 - 0.25 * rng.integers(0, 2, n0)
    B, C, D = np.arange(40_000, 47_500), np.arange(47_500, 49_100), np.arange(49_100, 51_500)
    hb[B], hb[C], hb[D] = now[8] - 10.25, now[12] - 10.25, now[14] - 10.25
    # 300 more expire in the tick before each idle tick: the exchange records then carry an
    # orphan count, which the idle tick (no memset of the records) must not see again
    for i, t in enumerate((0, 2, 5, 9, 17)):
        hb[52_000 + 300 * i:52_300 + 300 * i] = now[t] - 10.25
    X, Y, V, U = 100, 200, 300, 400
    log = rng.integers(-1, n0 + 2000, 30_000).astype(np.int32)  # (entries of ids without a record included)
    st = dict(reg=reg, free=free, hb=hb, epoch=np.zeros(W, np.uint32), queue=rng.permutation(n0).astype(np.int32),
              log=log)
    sc = _Scenario(st, len(log) + 420_000)

    def msgs(t, n, extra=None):
        b = _mixed(rng, sc.state, n, calm=[X, Y, V, U])
        if extra:
            extra(b)
        return b.events(rng, now[t])

    idle = [np.zeros(0, dt) for dt in (np.uint8, np.int32, np.int32, np.float64, np.int64)]
    sc.tick(now[0], msgs(0, 600), 1500)
    sc.tick(now[1], idle, 0)
    sc.tick(now[2], msgs(2, 600), 1500)
    sc.tick(now[3], idle, 0)
    sc.tick(now[4], idle, 0)   # (the records this one reads were last written by tick 2 and zeroed by tick 3)
    sc.tick(now[5], msgs(5, 600, lambda b: b.add(REG, [X], val=80)), 1500)
    sc.tick(now[6], idle, 0)
    sc.tick(now[7], msgs(7, 600, lambda b: b.add(REG, [X], val=2)), 1500)
    sc.tick(now[8], msgs(8, 600), 1500)                                        # B expires
    sc.tick(now[9], msgs(9, 600), 1500)
    sc.tick(now[10], idle, 0)
    sc.tick(now[11], msgs(11, 500, lambda b: _join(b, rng, sc.state, 1000)), 1500)
    sc.tick(now[12], msgs(12, 500, lambda b: _join(b, rng, sc.state, 1500)), 1500)    # C expires
    sc.tick(now[13], msgs(13, 400, lambda b: _join(b, rng, sc.state, 800)), 1500)
    sc.tick(now[14], msgs(14, 500, lambda b: (_join(b, rng, sc.state, 1500), b.add(REG, [Y], val=60))), 1500)  # D expires
    sc.tick(now[15], msgs(15, 600, lambda b: b.add(REG, [Y], val=2)), 1500)
    sc.tick(now[16], msgs(16, 600, lambda b: _join(b, rng, sc.state, 1800)), 1500)
    # 130 results for V: a free count past 128 that no registration announced
    ev = msgs(17, 600, lambda b: (_join(b, rng, sc.state, 900), b.add(RESULT, np.full(130, V))))
    c, orph = _after_messages(sc.state, sc.cap, now[17], ev)
    sc.tick(now[17], ev, _tasks_for_level(c, 40) - orph - sc.carried)
    sc.tick(now[18], idle, 0)
    # 3 000 drained workers return with one free process each; U registers with 5 000
    back = rng.choice(np.nonzero((sc.state["reg"] == 1) & (sc.state["free"] == 0))[0], 3000, replace=False)
    ev = msgs(19, 300, lambda b: (b.add(RESULT, back), b.add(REG, [U], val=5000)))
    c, orph = _after_messages(sc.state, sc.cap, now[19], ev)
    sc.tick(now[19], ev, _tasks_for_level(c, 140) - orph - sc.carried)
    for t, n, level in ((20, 500, 2), (21, 300, 1)):  # the wide table stays for one tick, then 128 rows
        ev = msgs(t, n)
        c, orph = _after_messages(sc.state, sc.cap, now[t], ev)
        sc.tick(now[t], ev, _tasks_for_level(c, level) - orph - sc.carried)
    assert [t for t, tk in enumerate(sc.ticks) if tk["idle"]] == list(LADDER_IDLE)
    assert sc.carried == 0
    return sc.done()


def _run_forms(scen, world, states=True, forms=None):
    """The scenario on a group of ``world`` ranks against its recorded oracle; returns the
    form of every launch of every tick, from rank 0's launch counts."""
    bals = _bals(scen, world)
    seen = []
    try:
        o = _Replay(scen)
        bals[0].timing_enable(True)
        for t, tk in enumerate(scen.ticks):
            bals[0].timing_read()
            mine = []

            def classify(attempt):
                n = {k: int(v[1]) for k, v in bals[0].timing_read().items()}
                mine.append(FORMS[(n.get("scan2", 0), n.get("plan", 0), n.get("emit", 0))])

            a, r = _group_tick(bals, *tk["args"], on_attempt=classify)
            seen.append(mine)
            assert r["fill_level"] == tk.get("level", r["fill_level"])
            b = o.tick(*tk["args"])
            if states or t == len(scen.ticks) - 1:
                _cmp(bals, o, a, b, t)
            else:
                _cmp_outputs(a, b, t)
        if forms is not None:
            assert seen == forms, seen
    finally:
        _close(bals)
    return seen


def _pairs(scen, seen):
    """The consecutive pairs of forms a run contained; (form, 'idle'): that form's tick was
    followed by an idle tick and then a tick with work."""
    got = set()
    for t, mine in enumerate(seen):
        if len(mine) > 1:
            got.add((mine[0], "FB_ERERUN", mine[-1]))
        if t:
            got.add((seen[t - 1][-1], mine[0]))
        if t >= 2 and scen.ticks[t - 1]["idle"] and not scen.ticks[t]["idle"] and not scen.ticks[t - 2]["idle"]:
            got.add((seen[t - 2][-1], "idle"))
    return got


def plan_fields(scen, world):
    """PlanIn fields (tests/plan_probe) of every rank's phase 2 of every tick of a scenario on
    ``world`` ranks, as (tick, rank, fields): tests/test_plan.py asks plan_tick for them on the
    CPU (the xcfirst = 0 cases mean something only where xcfirst defaults to 1)."""
    from faasbal.sharded import shard_range

    W = len(scen.st["reg"])
    raw = np.asarray(scen.st["log"])
    out, state, given = [], scen.st, np.zeros(0, np.int32)
    for t, tk in enumerate(scen.ticks):
        for r in range(world):
            base, n = shard_range(W, world, r)
            mine = lambda x: int(np.count_nonzero((x >= base) & (x < base + n)))  # noqa: E731
            out.append((t, r, dict(shard=1, phase=2, world=world, W=n, W_global=W, E=len(tk["args"][2]), R=32,
                                   head=len(state["log"]), head_local=mine(raw) + mine(given), Qn=len(state["queue"]),
                                   T=tk["args"][-1], ncu=256, max_lds=160 * 1024, win_occ=4)))
        state, given = tk["state"], np.concatenate([given, tk["out"]["assign"]])
    return out


@pytest.mark.parametrize("world", [2, 3])
def test_form_ladder(world):
    """Every tick's outputs and the whole state after it equal the oracle's, and the run
    contained every pair of LADDER_PAIRS plus every form followed by an idle tick."""
    scen = _ladder()
    seen = _run_forms(scen, world)
    print("world %d forms:" % world, " ".join("+".join(m) + ("(idle)" if tk["idle"] else "")
                                                for m, tk in zip(seen, scen.ticks)))
    want = LADDER_PAIRS | {(f, "idle") for f in FORMS.values()}
    got = _pairs(scen, seen)
    assert not want - got, "pairs not visited: %s (forms %s)" % (sorted(want - got), seen)
    assert seen == LADDER_FORMS


@pytest.mark.parametrize("world", [2, 3])
def test_form_ladder_without_state_reads(world):
    """The same ladder with no state read between the ticks (outputs only; the whole state
    once, after the last tick): reading the state is not what keeps the group consistent."""
    _run_forms(_ladder(), world, states=False, forms=LADDER_FORMS)


@functools.lru_cache(maxsize=1)
def _forced():
    """66 000 queued workers with 40 free processes each and one with 200, three ticks: 32
    whole rounds (2.1 M tasks), then two ticks of a few thousand tasks and messages."""
    rng = np.random.default_rng(66)
    W, Q = 68_000, 66_000
    reg = np.zeros(W, np.uint8)
    reg[:Q] = 1
    free = np.zeros(W, np.int32)
    free[:Q] = 40
    free[7] = 200
    hb = np.where(reg == 1, 1000.0 - 0.25 * rng.integers(0, 9, W), 0.0)
    st = dict(reg=reg, free=free, hb=hb, epoch=np.zeros(W, np.uint32), queue=rng.permutation(Q).astype(np.int32),
              log=rng.integers(-1, W, 20_000).astype(np.int32))
    sc = _Scenario(st, len(st["log"]) + 33 * Q + 20_000)
    idle = [np.zeros(0, dt) for dt in (np.uint8, np.int32, np.int32, np.float64, np.int64)]
    sc.tick(1000.0, idle, 32 * Q + 500)
    for t in (1, 2):
        sc.tick(1000.0 + 0.5 * t, _mixed(rng, sc.state, 600, calm=[7]).events(rng, 1000.0 + 0.5 * t), 1500)
    return sc.done()


def test_wide_then_xplan_by_round_hint():
    """Wide directly followed by xplan, which only fb_set_round_hint can arrange (the commit
    of a wide tick leaves a hint beyond 128).  With the hint at 32 on every rank the first
    tick launches as xplan, reaches the table's last row with free counts of 40 and 200 in
    the queue and relaunches 256 rows wide; the hint lowered to 32 again, the next tick is
    xplan (free counts of 7 and 167: beyond no row it needs); the one after, left to the
    commit's hint of 167, re-counts with 128 rows."""
    scen = _forced()
    bals = _bals(scen, 2)
    seen = []
    try:
        o = _Replay(scen)
        bals[0].timing_enable(True)
        for t, tk in enumerate(scen.ticks):
            if t < 2:
                for b in bals:
                    b._chk(b.lib.fb_set_round_hint(b.h, 32))
            bals[0].timing_read()
            mine = []

            def classify(attempt):
                n = {k: int(v[1]) for k, v in bals[0].timing_read().items()}
                mine.append(FORMS[(n.get("scan2", 0), n.get("plan", 0), n.get("emit", 0))])

            a, _r = _group_tick(bals, *tk["args"], on_attempt=classify)
            seen.append(mine)
            _cmp(bals, o, a, o.tick(*tk["args"]), t)
    finally:
        _close(bals)
    assert seen == [["xplan", "wide"], ["xplan"], ["recount"]], seen


# ------------------------------------------------------------------------------ 2. the edges
EDGE_Q = [65_537, 65_792, 77_824, 81_920, 81_921]


def _edge_state(rng, Q, cap, now=1000.0):
    """Q queued workers (3 % of them expired; free counts 2..4, 1 % one, 2 % more -- ``cap``;
    cap 32: up to 20, and the last 40 of the queue have 32), 1 000 known workers outside
    the queue, 2 000 ids without a record, and a log whose entries also name expired
    workers and ids without a record."""
    W = Q + 3000
    perm = rng.permutation(W)
    queued, rest = perm[:Q], perm[Q:Q + 1000]
    reg = np.zeros(W, np.uint8)
    reg[queued] = reg[rest] = 1
    free = np.zeros(W, np.int32)
    more = rng.integers(4, 21, Q) if cap == 32 else np.full(Q, cap)
    free[queued] = np.where(rng.random(Q) < 0.02, more, np.where(rng.random(Q) < 0.01, 1, rng.integers(2, 5, Q)))
    hb = np.zeros(W)
    hb[reg == 1] = now - 0.25 * rng.integers(0, 33, Q + 1000)
    hb[queued[rng.random(Q) < 0.03]] = now - 10.5
    if cap == 32:
        free[queued[-40:]], hb[queued[-40:]] = 32, now
    return dict(reg=reg, free=free, hb=hb, epoch=np.zeros(W, np.uint32), queue=queued.astype(np.int32),
                log=rng.integers(-1, W, 60_000).astype(np.int32))


@functools.lru_cache(maxsize=2)
def _edge(Q, cap, n_msgs=(2048, 2000, 2000)):
    """Three ticks from a queue of Q positions whose largest free count is ``cap`` (R = 32,
    64, 128 for 32, 40, 100).  The first tick carries 2 048 messages: 4 096 more positions,
    16 whole blocks, so the block count keeps Q's parity and the last block Q's fill
    (77 824 + 4 096: exactly five k_xscan chunks).  The ticks end in rounds 0, 1 and 3 of
    the round table; at R = 32 the last one in round 31, the table's last row: the 40
    workers at the queue's end start with 32 free processes, the first two ticks serve
    them once, and a result each brings them back to 32 (a 33rd would widen the table)."""
    rng = np.random.default_rng(Q * 1000 + cap)
    st = _edge_state(rng, Q, cap)
    sc = _Scenario(st, len(st["log"]) + 6 * Q)
    top = st["queue"][-40:] if cap == 32 else None
    levels = (0, 1, 31 if cap == 32 else 3)
    for t, level in enumerate(levels):
        now = 1000.0 + 0.5 * t
        lost = 32 - sc.state["free"][top] if cap == 32 else np.zeros(0, int)
        assert lost.min(initial=0) >= 0 and (t < 2 or cap != 32 or lost.max() == 1)
        b = _mixed(rng, sc.state, n_msgs[t] - int(lost.sum()), calm=top)
        if lost.sum():
            b.add(RESULT, np.repeat(top, lost))
        ev = b.events(rng, now)
        assert len(ev[0]) == n_msgs[t]
        c, orph = _after_messages(sc.state, sc.cap, now, ev)
        # (round 1 ends early: before the queue's end, and few workers leave the queue)
        n = 3000 if level == 0 else _tasks_for_level(c, level, 64 if level == 1 else 2)
        out = sc.tick(now, ev, n - orph - sc.carried, level=level)
        assert len(out["assign"]) == n and np.bincount(out["assign"]).max() == level + 1
    return sc.done()


def _edge_forms(cap, knobs=None):
    form = "xplan" if cap == 32 and (knobs or {}).get("xplan", 1) else "recount"
    return [[form]] * 3


@pytest.mark.parametrize("world", [2, 4, 16])
@pytest.mark.parametrize("cap", [32, 40, 100])
@pytest.mark.parametrize("Q", EDGE_Q)
def test_large_queue_edges(Q, cap, world):
    """xplan (cap 32) and the large-queue recount (cap 40, 100: R = 64, 128) with ~2 000
    mixed messages a tick, expired workers and orphans, at queue lengths that leave one
    position in the last block, an odd block count (half a k_emit_shard_xp workgroup empty)
    and a whole or a barely started last k_xscan chunk."""
    _run_forms(_edge(Q, cap), world, forms=_edge_forms(cap))


# ------------------------------------------------------------------------------ 3. knobs
@pytest.fixture
def knobs(request, monkeypatch):
    """fb_set_path values for every context made in the test (every rank: the exchange
    layouts agree)."""
    for k, v in request.param.items():
        monkeypatch.setitem(TEST_PATHS, k, v)
    return request.param


@pytest.mark.parametrize("knobs", KNOBS, ids=KNOB_IDS, indirect=True)
def test_form_ladder_knobs(knobs):
    """(xplan = 0: the xplan ticks re-count in a phase-2 k_scan, the recount form's launches.)"""
    forms = LADDER_FORMS
    if knobs.get("xplan") == 0:
        forms = [["recount" if f == "xplan" else f for f in m] for m in forms]
    _run_forms(_ladder(), 2, forms=forms)


@pytest.mark.parametrize("knobs", KNOBS, ids=KNOB_IDS, indirect=True)
def test_large_queue_edge_knobs(knobs):
    """65 792 positions at world 2: xcfirst is on by default there, so xcfirst = 0 is the
    other order (tests/test_plan.py::test_xcfirst_defaults_on_at_the_knob_shapes asks
    plan_tick, for this scenario and the ladder's xplan ticks)."""
    _run_forms(_edge(65_792, 32), 2, forms=_edge_forms(32, knobs))


@pytest.mark.parametrize("seed", range(6))
def test_sharded_random_multitick_wfirst0(monkeypatch, seed):
    monkeypatch.setitem(TEST_PATHS, "wfirst", 0)
    tgs.test_sharded_random_multitick(seed)


# ------------------------------------------------------------------------------ 4. calls around the tick
@functools.lru_cache(maxsize=2)
def _small(Q):
    """One recorded tick state of Q queued workers (4 096: the rows form; 65 792: xplan)."""
    rng = np.random.default_rng(Q)
    st = _edge_state(rng, Q, 32)
    return st, len(st["log"]) + 40_000


def _fresh(st, cap):
    o = Oracle(len(st["reg"]), cap)
    o.load(st["reg"], st["free"], st["hb"], st["epoch"], st["queue"], st["log"])
    return o


def _group_of(st, cap, world):
    sc = _Scenario(st, cap)
    return _bals(sc, world), sc.o


@pytest.mark.parametrize("Q", [4096, 65_792])
def test_uncommitted_relaunch(Q):
    """Three launches of one tick without a commit give the same outputs (every phase 2
    flipped the records' parity); a fourth with other messages, committed, equals the
    oracle that never saw the first three -- and so does the tick after it."""
    st, cap = _small(Q)
    rng = np.random.default_rng(Q + 1)
    bals, o = _group_of(st, cap, 3)
    try:
        ev1 = _mixed(rng, st, 500).events(rng, 1000.0)
        ev2 = _mixed(rng, st, 700).events(rng, 1000.0)
        want = _fresh(st, cap).tick(1000.0, TTE, *ev1, 3000)
        for _ in range(3):
            a, _r = _group_tick(bals, 1000.0, TTE, *ev1, 3000, commit=False)
            _cmp_outputs(a, want, 0)
        args = (1000.0, TTE, *ev2, 2500)
        a, _r = _group_tick(bals, *args)
        _cmp(bals, o, a, o.tick(*args), 0)
        # an idle launch (no memset of the records), abandoned, then a tick with work
        _group_tick(bals, 1000.5, TTE, [], [], [], [], [], 0, commit=False)
        ev3 = _mixed(rng, o.export(), 400).events(rng, 1000.5)
        args = (1000.5, TTE, *ev3, 2000)
        a, _r = _group_tick(bals, *args)
        _cmp(bals, o, a, o.tick(*args), 1)
    finally:
        _close(bals)


def test_abandoned_launch_results_leave_log_entries_in_flight():
    """Regression: a sharded launch clears the log entries its results complete in place (the
    same tick's log scan reads them), so an abandoned launch left them completed: the next
    tick, without those results, no longer equalled the oracle's log (79 entries at this
    shape), and a later death of their workers would not have redistributed them.  The next
    launch now names the entries again (k_log_undo) unless the tick was committed."""
    st, cap = _small(4096)
    rng = np.random.default_rng(7)
    bals, o = _group_of(st, cap, 2)
    try:
        live = rng.choice(np.nonzero(o.export()["log"] >= 0)[0], 300, replace=False)
        b = _Batch()
        b.add(RESULT, o.export()["log"][live], seq=live)
        _group_tick(bals, 1000.0, TTE, *b.events(rng, 1000.0), 100, commit=False)
        for t in range(2):  # (the second tick: the abandoned launch's notes are not applied twice)
            args = (1000.0 + 0.5 * t, TTE, [], [], [], [], [], 1000)
            a, _r = _group_tick(bals, *args)
            _cmp(bals, o, a, o.tick(*args), t)
    finally:
        _close(bals)


def test_abandoned_launch_then_load_keeps_the_loaded_log():
    """Regression: fb_load_shard replaces the log, so the notes of a launch abandoned before
    it must be dropped with it -- else the next launch writes the old owners at the old local
    indices into the loaded log."""
    st, cap = _small(4096)
    rng = np.random.default_rng(8)
    bals, o = _group_of(st, cap, 2)
    try:
        live = rng.choice(np.nonzero(o.export()["log"] >= 0)[0], 2000, replace=False)
        b = _Batch()
        b.add(RESULT, o.export()["log"][live], seq=live)
        _group_tick(bals, 1000.0, TTE, *b.events(rng, 1000.0), 100, commit=False)
        st2 = _edge_state(np.random.default_rng(9), 4096, 32)  # other workers own the log's entries
        o = _fresh(st2, cap)
        for x in bals:
            x.load(st2)
        for t in range(2):
            ev = _mixed(rng, o.export(), 300).events(rng, 1000.0 + 0.5 * t)
            args = (1000.0 + 0.5 * t, TTE, *ev, 1000)
            a, _r = _group_tick(bals, *args)
            _cmp(bals, o, a, o.tick(*args), t)
    finally:
        _close(bals)


def test_group_dispatcher_enospc_rerun_with_results():
    """The drop-in on a shard group: a tick that carries results overflows the in-flight log
    (FB_ENOSPC, not committed), the dispatcher compacts on the host -- state read, log
    renumbered, loaded again on every rank -- and reruns the tick.  One finished entry ahead
    of the results' entries, ten unfinished ones behind them: the compaction moves live
    entries of another worker to the indices the failed launch noted.  Afterwards the device
    log holds exactly the dispatcher's in-flight table, and every message sent equals a run
    whose log never fills."""
    import torch  # noqa: F401
    from faasbal import codec
    from faasbal.dispatcher import GpuPushDispatcher
    from faasbal.sharded import LocalShardGroup
    from test_dispatcher import FakeEnv, wid

    def msg(w, typ, data, now):
        return (wid(w), codec.serialize({"type": typ, "data": data}).encode(), now)

    runs, comp = [], []
    for cap in (1 << 12, 73):
        env = FakeEnv()
        grp = LocalShardGroup(2, 8, cap, max_events=128)
        try:
            d = GpuPushDispatcher("127.0.0.1", 0, 10, max_workers=8, max_events=128, max_inflight=cap,
                                  redis_client=env, subscriber=env, socket=env, poller=env, clock=env.clock,
                                  balancer=grp)
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
                    # worker 0 answers at once, worker 1 one tick late: at tick 2 both results arrive,
                    # worker 0's naming an entry behind the finished one and amid worker 2's
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
                st = grp.read_state()
                want = np.full(d.head, -1, np.int32)
                for q, (_tid, s) in d.inflight.items():
                    want[q] = s
                np.testing.assert_array_equal(st["log"], want, err_msg="cap %d tick %d" % (cap, t))
            runs.append(sent)
            comp.append(d.compactions)
        finally:
            grp.close()
    assert comp == [0, 1], comp
    assert runs[0] == runs[1]
    assert sum(m["type"] == "task" for _, m in runs[1][2]) == 61


def _cmp_merged(sg, so, what):
    m = so["reg"].astype(bool)
    np.testing.assert_array_equal(sg["reg"], so["reg"], err_msg=what + " reg")
    for k in ("free", "hb", "epoch"):
        np.testing.assert_array_equal(sg[k][m], so[k][m], err_msg=what + " " + k)
    np.testing.assert_array_equal(sg["queue"], so["queue"], err_msg=what + " queue")
    np.testing.assert_array_equal(sg["log"], so["log"], err_msg=what + " log")


@pytest.mark.parametrize("Q", [4096, 65_792])
def test_group_purge(Q):
    """LocalShardGroup.purge: the expired workers' tasks reported, none dispatched; then
    a tick with work."""
    import torch  # noqa: F401
    from faasbal.sharded import LocalShardGroup

    st, cap = _small(Q)
    rng = np.random.default_rng(Q + 2)
    o = _fresh(st, cap)
    grp = LocalShardGroup(3, len(st["reg"]), cap, max_events=4096)
    try:
        grp.load(st)
        a = grp.purge(1000.0, TTE)
        b = o.tick(1000.0, TTE, [], [], [], [], np.zeros(0, np.int64), 0, dispatch_limit=0)
        assert len(b["orphans"]) > 50 and len(b["evicted"]) > 50 and a["result"]["n_assigned"] == 0
        np.testing.assert_array_equal(a["orphans"], b["orphans"])
        np.testing.assert_array_equal(a["evicted"], b["evicted"])
        _cmp_merged(grp.read_state(), o.export(), "purge")
        ev = _mixed(rng, o.export(), 600).events(rng, 1000.5)
        a, b = grp.tick(1000.5, TTE, *ev, 3000), o.tick(1000.5, TTE, *ev, 3000)
        _cmp_outputs(a, b, 1)
        _cmp_merged(grp.read_state(), o.export(), "tick")
    finally:
        grp.close()


@pytest.mark.parametrize("Q", [4096, 65_792])
def test_full_assign_equals_union(Q):
    """fb_set_full_assign on rank 0: its assignments() is the union of every rank's
    local_assignments() (and the oracle's), three ticks."""
    st, cap = _small(Q)
    rng = np.random.default_rng(Q + 3)
    bals, o = _group_of(st, cap, 3)
    try:
        bals[0].set_full_assign(True)
        for t in range(3):
            now = 1000.0 + 0.5 * t
            ev = _mixed(rng, o.export(), 600).events(rng, now)
            args = (now, TTE, *ev, 3000)
            a, r = _group_tick(bals, *args, commit=False)
            full = bals[0].assignments().copy()
            for b in bals:
                b.commit()
            assert len(full) == r["n_assigned"] > 0
            np.testing.assert_array_equal(full, a["assign"], err_msg="tick %d" % t)
            _cmp(bals, o, a, o.tick(*args), t)
    finally:
        _close(bals)
