"""The life of a tick on the GPU: tests/life_cases.py (what the library did when ten context
flags and one ladder per entry point kept the rules) held against the library itself, through
the C ABI only.

Each case brings a small context into one state by clean means -- the flags of life_cases
follow every call -- and then makes every entry point's call once, from that state again each
time (a rejected fb_tick_stage drops a staged batch, a load drops everything else).  The
call's return code is the table's: FB_ESTATE with the table's message, or no refusal of the
gate; and the duties are the table's, as fb_timing_read counts the launches labelled
"commit", "log_undo" and "settle".

The last test is the one place the library differs from that table on purpose: a rejected
load leaves the stale-entries fact alone.  On the library before faasbal_life.h every other
case passes unchanged and that one fails at its last tick: slot 0's two orphans come out as
entries [0, 1], redistributed once already, where the oracle has its new entries [10, 74].
"""
import ctypes as C

import numpy as np
import pytest

import abandoned
import life_cases as lc
from faasbal import GpuBalancer, _lib, synth
from faasbal.sharded import ShardedBalancer

pytestmark = pytest.mark.gpu

W, CAP, E_CAP = 64, 64, 32
NOW, TTE = 1000.0, 10.0
RES = synth.EV_RESULT


def small_state():
    """64 registered slots with 2 free processes each, all queued; entries 0 .. 7 in flight on
    slots 0 .. 7."""
    return dict(reg=np.ones(W, np.uint8), free=np.full(W, 2, np.int32), hb=np.full(W, NOW - 1.0),
                epoch=np.zeros(W, np.uint32), queue=np.arange(W, dtype=np.int32), log=np.arange(8, dtype=np.int32))


def messages(n=3):
    """n messages of slots 1 .. n: results that complete their senders' entries."""
    s = np.arange(1, n + 1)
    return (np.full(n, RES, np.uint8), s.astype(np.int32), np.zeros(n, np.int32), np.full(n, NOW), s.astype(np.int64))


class Ctx:
    """A context, and the flags the old library would hold for it (life_cases.Raw)."""

    def __init__(self, kind, g, st, window=False, eager=False):
        self.kind, self.g, self.st, self.window, self.eager = kind, g, st, window, eager
        self.lib, self.h = g.lib, g.h
        self.raw = lc.CREATED
        self.now = NOW
        self.win_launch = False  # the next launch with messages is a window tick (the case knows)
        self.msgs, self.pending, self.base_now = messages(), 0, NOW  # a tick with messages: theirs, its tasks, its clock
        g.timing_enable(True)

    def did(self, act):
        self.raw = lc.apply(self.kind, self.raw, act)[2]

    # -- clean means
    def reset(self):
        assert self.lib.fb_log_compact_shard_cancel(self.h) == 0  # (a mark the last call left)
        bad = (np.zeros(1, np.uint8), np.full(1, 1 << 20, np.int32), np.zeros(1, np.int32), np.full(1, NOW))
        assert self.lib.fb_tick_stage(self.h, NOW, 1, *(a.ctypes.data_as(C.c_void_p) for a in bad), None) == _lib.FB_EINVAL
        self.g.load(self.st)
        self.raw, self.now = lc.CREATED, self.base_now
        self.g.timing_read()

    def stage(self, ev=None, pinned=False):
        ev = ev or ((), (), (), (), None)
        if pinned:
            ev = self.keep = self.g.pin_events(*ev)
        self.g.stage(self.now, *ev)
        self.E = len(ev[0])
        self.did(("stage", 1))

    def launch(self, n_pending=0):
        win = self.win_launch and self.E > 0
        assert self.lib.fb_tick_launch_staged(self.h, TTE, n_pending) == 0, self.lib.fb_last_error(self.h)
        self.did(("launch", self.E, int(win), int(win and self.eager)))
        if self.kind == "shard":
            self.g._E = self.E

    def cont(self):
        self.g.cont()
        self.did(("continue",))

    def wait(self, want=0):
        r = _lib.TickResult()
        rc = self.lib.fb_tick_wait(self.h, C.byref(r))
        assert rc == want, (rc, self.lib.fb_last_error(self.h))
        self.last, self.wait_rc = r, rc
        assert rc or r.reruns == 0
        self.did(("wait", {0: "ok", _lib.FB_ENOSPC: "log_full", _lib.FB_EHIP: "lengths_rejected",
                           _lib.FB_EINVAL: "invalid_message"}[rc]))

    def commit(self):
        deferred = self.kind in lc.LISTS and not self.raw.l_win and not self.raw.l_eager
        self.g.commit()
        self.did(("commit", int(deferred), int(self.kind in lc.LISTS and self.last.n_orphans > 0)))

    def tick(self, ev=None, n_pending=0):
        self.stage(ev)
        self.launch(n_pending)
        if self.kind == "shard":
            self.cont()
        self.wait()
        self.commit()

    # -- every entry point's call, with arguments that are valid in every state
    def call(self, name):
        lib, h, n64, buf = self.lib, self.h, C.c_int64(), np.zeros(self.g.max_log + 64, np.int32)
        p = buf.ctypes.data_as(C.c_void_p)
        if name == "load_state":
            return lib.fb_load_state(h, 0, None, None, None, None, None, 0, None, 0)
        if name == "load_shard":
            return lib.fb_load_shard(h, 0, 0, None, None, None, None, None, 0, None, None, 0, 0)
        if name == "read_state":
            return lib.fb_read_state(h, None, None, None, None, None, C.byref(n64), p, C.byref(C.c_int64()))
        if name == "read_inflight":
            return lib.fb_read_inflight(h, np.zeros(max(self.g.n_workers, 1) + 8, np.uint32).ctypes.data_as(C.c_void_p))
        if name == "read_shard_log":
            return lib.fb_read_shard_log(h, p, C.byref(n64), C.byref(C.c_int64()))
        if name == "device_view":
            return lib.fb_device_view_get(h, C.byref(_lib.DeviceView()))
        if name == "log_compact":
            return lib.fb_log_compact(h, -1, None, 0, C.byref(n64))
        if name == "pool_stats":
            return lib.fb_pool_stats(h, NOW, TTE, None, 0, C.byref(_lib.PoolSummary()))
        if name == "pool_stats_shard":
            return lib.fb_pool_stats_shard(h, NOW, TTE, None, 0, C.byref(_lib.PoolSummary()), C.byref(n64))
        if name in ("log_reclaim", "log_reclaim_shard"):  # (an empty prefix: behind the gate nothing is launched)
            return getattr(lib, "fb_" + name)(h, 0, None, None, None, 0, C.byref(n64))
        if name == "log_compact_shard_mark":  # (a sharded context checks the bitmap's size ahead of the gate)
            if self.kind != "shard":
                return lib.fb_log_compact_shard_mark(h, None, 0, None)
            view = self.g.compact_exchange()
            return lib.fb_log_compact_shard_mark(h, C.c_void_p(self.g._cbuf.data_ptr()), view.numel(), None)
        if name == "log_compact_shard_apply":
            return lib.fb_log_compact_shard_apply(h, 0, None, 0, None)
        if name == "log_compact_shard_cancel":
            return lib.fb_log_compact_shard_cancel(h)
        if name == "exchange_bytes":
            return lib.fb_exchange_bytes(h, 0, C.byref(n64))
        if name == "stage":
            return lib.fb_tick_stage(h, self.now, 0, None, None, None, None, None)
        if name == "launch":
            return lib.fb_tick_launch_staged(h, TTE, 0)
        if name == "tick_continue":
            return lib.fb_tick_continue(h)
        if name == "wait":
            return lib.fb_tick_wait(h, None)
        if name == "commit":
            return lib.fb_tick_commit(h)
        if name == "get_local_assignments":
            return lib.fb_get_local_assignments(h, 0, 0, None, None)
        if name == "get_assignments":
            return lib.fb_get_assignments(h, 0, 0, p)
        if name == "get_orphans":
            return lib.fb_get_orphans(h, 0, p)
        if name == "get_evicted":
            return lib.fb_get_evicted(h, 0, p)
        if name == "get_outputs":
            return lib.fb_get_outputs(h, None, None, None)
        if name == "get_outputs_compact":
            return lib.fb_get_outputs_compact(h, None, None, 0, C.byref(n64), None, None)
        if name == "expand_compact":
            return lib.fb_expand_compact(h, None, None, 0, p)
        if name == "get_event_status":
            return lib.fb_get_event_status(h, 0, p)
        if name == "set_window":
            return lib.fb_set_window(h, 1 if self.window else -1)
        if name == "set_eager_commit":
            return lib.fb_set_eager_commit(h, int(self.eager))
        if name == "set_compact_out":
            return lib.fb_set_compact_out(h, None, None, 0, None, 0, None, 0)
        if name == "set_full_assign":
            return lib.fb_set_full_assign(h, 0)
        if name == "set_round_hint":
            return lib.fb_set_round_hint(h, 2)
        if name == "set_path":
            return lib.fb_set_path(h, b"lazy", 1)
        if name == "debug_read":
            return lib.fb_debug_read(h, None, 0, C.byref(n64))
        if name == "sync":
            return lib.fb_sync(h)
        raise KeyError(name)


# checks of a call's own, behind the gate, that a valid-everywhere argument list cannot avoid
BEHIND_THE_GATE = {"get_outputs_compact": _lib.FB_ESTATE,   # "the tick was launched without fb_set_compact"
                   "get_assignments": _lib.FB_ESTATE,       # sharded: "use fb_get_local_assignments"
                   "expand_compact": _lib.FB_EINVAL,        # no compact form given
                   }


# -- the states: name -> how to reach it from a reset context
def s_created(c):
    pass


def s_staged(c):
    c.stage(c.msgs)


def s_launched(c):
    c.stage(c.msgs)
    c.launch(c.pending)


def s_launched_idle(c):
    c.stage()
    c.launch()


def s_phase2(c):
    s_launched(c)
    c.cont()


def s_waited(c):
    s_launched(c)
    if c.kind == "shard":
        c.cont()
    c.wait()


def s_log_full(c):
    """FB_ENOSPC: 128 free processes, 56 free log entries; the results complete entries."""
    c.stage(c.msgs)
    c.launch(1000)
    if c.kind == "shard":
        c.cont()
    c.wait(_lib.FB_ENOSPC)


def s_dropped_lengths(c):
    c.g.set_path("fault_qlen", 1 << 28)
    s_launched(c)
    if c.kind == "shard":
        c.cont()
    c.wait(_lib.FB_EHIP)


def s_dropped_message(c):
    """A pinned batch (checked on the device) with a slot out of range."""
    k, s, v, t, q = c.msgs
    s = s.copy()
    s[1] = 1 << 20
    c.stage((k, s, v, t, q), pinned=True)
    c.launch()
    c.wait(_lib.FB_EINVAL)


def s_commit_pending(c):
    c.tick(c.msgs, c.pending)
    c.now += 1.0


def s_stale(c):
    """Everybody expires with entries in flight: the commit leaves them in the log."""
    c.now += 100.0
    c.tick()
    assert c.last.n_orphans > 0


def s_stale_staged(c):
    s_stale(c)
    c.stage()


STATES = {
    "hb": (s_created, s_staged, s_launched, s_launched_idle, s_waited, s_log_full, s_dropped_lengths,
           s_dropped_message, s_commit_pending, s_stale, s_stale_staged),
    "deque": (s_created, s_staged, s_launched, s_waited, s_log_full),  # (no device length it rejects can be injected)
    "shard": (s_created, s_staged, s_launched, s_phase2, s_waited, s_log_full, s_dropped_lengths),
    "hb_window": (s_created, s_launched, s_waited, s_commit_pending),
    "hb_eager": (s_launched, s_waited),
    "hb_large": (s_created, s_launched, s_waited, s_dropped_message),
}


def _window_state():
    """tests/test_gpu_pool_stats.py's stream: 300 slots, 16 tasks and results a tick -- its
    first tick with messages runs as a window tick under fb_set_window(1)."""
    st = synth.zipf_state(W=300, seed=3, dead_frac=0.0)
    tk = synth.stream_ticks(st, n_ticks=1, seed=11, tasks_per_tick=16, results_per_tick=16, dt=0.3, hb_frac=0.01,
                            join_frac=0.0)[0]
    return st, tk


@pytest.fixture(scope="module")
def contexts():
    made = {}

    def get(name):
        if name in made:
            return made[name]
        if name in ("hb", "deque"):
            g = GpuBalancer(W, CAP, max_events=E_CAP, mode="heartbeat" if name == "hb" else "deque")
            c = Ctx(name, g, small_state())
        elif name == "shard":
            c = Ctx("shard", ShardedBalancer(0, 1, W, CAP, max_events=E_CAP), small_state())
        elif name in ("hb_window", "hb_eager"):
            st, tk = _window_state()
            g = GpuBalancer(300, 3 * len(st["log"]) + 4096, max_events=max(len(tk["ev_kind"]), 1))
            g.set_window(1)
            g.set_eager_commit(name == "hb_eager")
            c = Ctx("hb", g, st, window=True, eager=name == "hb_eager")
            c.msgs = (tk["ev_kind"], tk["ev_slot"], tk["ev_val"], tk["ev_ts"], tk["ev_seq"])
            c.pending, c.base_now = tk["n_new"], tk["now"]
        else:
            st = synth.zipf_state(W=abandoned.H_LARGE_W, seed=4, dead_frac=0.05)
            g = GpuBalancer(abandoned.H_LARGE_W, len(st["log"]) + 50000, max_events=E_CAP)
            c = Ctx("hb_large", g, st)
        made[name] = c
        return c

    yield get
    for c in made.values():
        c.g.close()


def _is_window_tick(c):
    """Whether a launch of the context's messages on the reset context commits as a window tick."""
    c.reset()
    w0 = c.g.window_stats()
    c.win_launch = False
    c.tick(c.msgs, c.pending)
    w1 = c.g.window_stats()
    assert w1[1] == w0[1], "the tick fell back: its launch is not told from a general one"
    return w1[0] == w0[0] + 1


def _know_window(c, ctx):
    """Whether the context's tick with messages launches as a window tick (once per context)."""
    if ctx in ("hb_window", "hb_eager", "hb_large") and not hasattr(c, "is_win"):
        c.is_win = _is_window_tick(c)
        assert c.is_win or ctx == "hb_large", "the stream's tick is no window tick"
    c.win_launch = getattr(c, "is_win", False)


CASES = [(k, s.__name__[2:]) for k, ss in STATES.items() for s in ss]


@pytest.mark.parametrize("ctx,state", CASES)
def test_every_call_in_state(contexts, ctx, state):
    c = contexts(ctx)
    reach = dict((s.__name__[2:], s) for s in STATES[ctx])[state]
    _know_window(c, ctx)
    seen = set()
    for call in lc.CALLS:
        c.reset()
        reach(c)
        seen.add(lc.canon(c.kind, c.raw))
        assert lc.canon(c.kind, c.raw) in lc.STATES[c.kind]
        variant = "log" if call in ("read_state", "device_view") else "ok"
        refuse, duties = lc.gate(c.kind, c.raw, call)
        settle = refuse is None and variant == "log" and c.raw.stale_any
        c.g.timing_read()
        rc = c.call(call)
        msg = (c.lib.fb_last_error(c.h) or b"").decode()
        what = (ctx, state, call, rc, msg)
        if refuse is not None:
            assert rc == _lib.FB_ESTATE and msg == refuse, what
        elif call == "wait" and c.raw.l_failed:
            assert rc == c.wait_rc, what  # what failed fails again
        elif rc != 0:
            assert rc == BEHIND_THE_GATE.get(call) and msg not in _refusals(c.kind, call), what
        got = {k: v[1] for k, v in c.g.timing_read().items()}
        if call not in ("launch", "commit"):  # (their own launches carry the label too)
            assert got.get("commit", 0) == int("flush" in duties), what + (got,)
        assert got.get("log_undo", 0) == int("undo" in duties), what + (got,)
        assert got.get("settle", 0) == int(settle), what + (got,)
    assert len(seen) == 1


def _refusals(kind, call):
    out = set()
    for r in lc.closure(kind):
        m = lc.gate(kind, r, call)[0]
        if m:
            out.add(m)
    return out


def test_states_reached_cover_the_positions(contexts):
    """The cases above reach every position of a tick's life, every qualifier and every debt."""
    seen = set()
    for ctx, ss in STATES.items():
        c = contexts(ctx)
        _know_window(c, ctx)
        for s in ss:
            c.reset()
            s(c)
            seen.add((c.kind,) + tuple(lc.canon(c.kind, c.raw).split(",")))
    pos = {s[2] for s in seen}
    assert pos == {"none", "phase1", "launched", "waited", "failed", "dropped"}, pos
    assert any(s[5] == "1" for s in seen) and any(s[6] == "1" for s in seen) and any(s[8] == "1" for s in seen)
    assert any(s[2] == "failed" and s[7] != "0" for s in seen), "FB_ENOSPC with clears owed"
    assert any(s[3] == "1" and s[4] == "0" for s in seen) and any(s[4] == "1" for s in seen), "window, eager"
    assert any(s[0] == "hb_large" and s[2] == "dropped" for s in seen), "a dropped launch that owes clears"


# ------------------------------------------------------------------ the deliberate correction
def test_rejected_load_keeps_stale_entries_dead():
    """life_cases.restale_scenario: slot 0 dies with entries in flight and the tick commits, so
    they stay in the log, stale.  A load with a bad queue entry is rejected.  Slot 0 registers
    again, receives tasks, dies again: only its new entries are orphans -- every tick's outputs
    and the final state are the oracle's."""
    st, steps, final = lc.restale_scenario()
    g = GpuBalancer(len(st["reg"]), lc.RESTALE_CAP, max_events=2 * len(st["reg"]))
    g.load(st)
    got = []
    for args, want in steps:
        if want is None:  # the rejected load
            reg, free, hb, epoch, bad_q = (np.ascontiguousarray(a) for a in args)
            rc = g.lib.fb_load_state(g.h, len(reg), *(a.ctypes.data_as(C.c_void_p) for a in (reg, free, hb, epoch, bad_q)),
                                     len(bad_q), None, 0)
            assert rc == _lib.FB_EINVAL, g.lib.fb_last_error(g.h)
            continue
        a = g.tick(*args)
        print("tick at %.1f: device orphans %s, oracle %s" % (args[0], a["orphans"].tolist(), want["orphans"].tolist()))
        got.append((a, want))
    for t, (a, b) in enumerate(got):
        for k in ("reconnect", "assign", "orphans", "evicted"):
            np.testing.assert_array_equal(a[k], b[k], err_msg="tick %d: %s" % (t, k))
    sg = g.read_state()
    for k in ("reg", "queue", "log"):
        np.testing.assert_array_equal(sg[k], final[k], err_msg=k)
    g.close()
