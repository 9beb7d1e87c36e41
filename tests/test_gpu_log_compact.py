"""fb_log_compact on the GPU: the in-flight log renumbered on the device.

Against the numpy model of the rule (tests/lc_model.py), against a twin balancer that took
the host path (read_state -> searchsorted -> load_state), and -- ticking on after
compactions -- against the oracle, which never compacts: the tests keep the map between the
two numberings, translate result sequences going in and orphans coming out.
"""
import ctypes as C

import numpy as np
import pytest

from faasbal import FaasbalError, GpuBalancer, _lib, synth
from lc_model import compact_model, host_compact
from oracle import Oracle

pytestmark = pytest.mark.gpu

STATE_KEYS = ("reg", "free", "hb", "epoch", "queue", "log")


def _same_state(a, b, what, keys=STATE_KEYS):
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg="%s: %s" % (what, k))
    assert a["head"] == b["head"], what


# ------------------------------------------------------------------ 1. shapes vs the model
HEADS = (0, 1, 63, 64, 65, 2047, 2048, 2049, 3 * 2048 + 5, 40000)
PATTERNS = ("all", "none", "alternating", "random30", "first", "last")
W_SHAPES = 300


def _pattern(name, head, rng):
    q = np.arange(head)
    if name == "all":
        return np.ones(head, bool)
    if name == "none":
        return np.zeros(head, bool)
    if name == "alternating":
        return q % 2 == 0
    if name == "random30":
        return rng.random(head) < 0.3
    return q == (0 if name == "first" else head - 1)


def _shape_state(head, live, rng):
    """W = 300 slots: 0..99 registered with epoch 0 (they own the live entries), 100..149
    registered with epochs anywhere in [0, head] -- inside dead runs, on live entries --
    and entries of their own where the epoch allows, 150..199 registered with epoch ==
    head, 200..299 without a record, epochs up to past the head."""
    W = W_SHAPES
    reg = (np.arange(W) < 200).astype(np.uint8)
    epoch = np.zeros(W, np.uint32)
    epoch[100:150] = rng.integers(0, head + 1, 50)
    epoch[150:200] = head
    epoch[200:] = rng.integers(0, head + 6, 100)
    log = np.full(head, -1, np.int32)
    idx = np.flatnonzero(live)
    s = rng.integers(0, 150, len(idx))
    s = np.where(idx >= epoch[s].astype(np.int64), s, idx % 100)
    log[idx] = s
    free = np.where(reg, rng.integers(0, 4, W), 0).astype(np.int32)
    hb = np.where(reg, 1000.0 - 0.25 * rng.integers(0, 8, W), 0.0)
    queue = rng.permutation(np.flatnonzero(reg & (free > 0))).astype(np.int32)[:40]
    return dict(reg=reg, free=free, hb=hb, epoch=epoch, queue=queue, log=log)


@pytest.mark.parametrize("head", HEADS)
def test_shapes_against_the_model(head):
    rng = np.random.default_rng(head)
    g = GpuBalancer(W_SHAPES, 40000 + 64, max_events=64)
    for name in PATTERNS:
        live = _pattern(name, head, rng)
        st = _shape_state(head, live, rng)
        g.load(st)
        before, infl = g.read_state(), g.inflight()
        want, kept = compact_model(before)
        np.testing.assert_array_equal(kept, np.flatnonzero(live))  # (the pattern survived the load)
        out = g.compact_log()
        what = "head %d %s" % (head, name)
        assert out["n_kept"] == len(kept), what
        np.testing.assert_array_equal(out["kept"], kept, err_msg=what + ": kept")
        _same_state(g.read_state(), want, what)
        np.testing.assert_array_equal(g.inflight(), infl, err_msg=what + ": inflight")
        # the same without the kept list, and with the count stated
        g.load(st)
        assert g.compact_log(expect=len(kept), want_kept=False) == {"n_kept": len(kept), "kept": None}
        _same_state(g.read_state(), want, what + " (no kept list)")
        np.testing.assert_array_equal(g.inflight(), infl, err_msg=what + ": inflight (no kept list)")
        # compacting a compacted log keeps everything
        again = g.compact_log()
        np.testing.assert_array_equal(again["kept"], np.arange(len(kept)), err_msg=what + ": twice")
        _same_state(g.read_state(), want, what + " (twice)")
    g.close()


# ------------------------------------------------------------------ helpers: ticks vs the oracle
def _state_of(scen):
    return dict(reg=scen["init_reg"], free=scen["init_free"], hb=scen["init_hb"], epoch=scen["init_epoch"],
                queue=scen["init_queue"], log=scen["init_log"])


def _resolve_own(log, tk):
    """A result names an in-flight entry of its own slot (or none): sequences of `log`."""
    seq = np.full(len(tk["ev_kind"]), -1, np.int64)
    for i in np.nonzero(tk["ev_kind"] == synth.EV_RESULT)[0]:
        mine = np.nonzero(log == tk["ev_slot"][i])[0]
        if len(mine) and tk["ev_pick"][i] % 5 != 4:
            seq[i] = mine[tk["ev_pick"][i] % len(mine)]
    return seq


class SeqMap:
    """old <-> new: g2o[q] is the oracle's sequence of the GPU balancer's entry q (ascending)."""

    def __init__(self, head):
        self.g2o = np.arange(head, dtype=np.int64)

    def to_gpu(self, seq):
        out = np.full(len(seq), -1, np.int64)
        i = np.searchsorted(self.g2o, seq)
        ok = (seq >= 0) & (i < len(self.g2o))
        ok[ok] = self.g2o[i[ok]] == seq[ok]
        out[ok] = i[ok]  # (an entry the compaction dropped was dead: no sequence names it)
        return out

    def to_oracle(self, seq):
        return self.g2o[np.asarray(seq, np.int64)]

    def dispatched(self, o_head_before, n):
        self.g2o = np.concatenate([self.g2o, o_head_before + np.arange(n, dtype=np.int64)])

    def compacted(self, kept):
        self.g2o = self.g2o[kept]


def _tick_pair(g, o, m, tk, tte, n, t, seq_o=None):
    """One tick on both, sequences translated; outputs compared.  Returns the oracle's."""
    so = o.export()
    if seq_o is None:
        seq_o = _resolve_own(so["log"], tk)
    seq_g = m.to_gpu(seq_o)
    a = g.tick(tk["now"], tte, tk["ev_kind"], tk["ev_slot"], tk["ev_val"], tk["ev_ts"], seq_g, n)
    b = o.tick(tk["now"], tte, tk["ev_kind"], tk["ev_slot"], tk["ev_val"], tk["ev_ts"], seq_o, n)
    for k in ("reconnect", "assign", "evicted"):
        np.testing.assert_array_equal(a[k], b[k], err_msg="tick %d: %s" % (t, k))
    np.testing.assert_array_equal(m.to_oracle(a["orphans"]), b["orphans"], err_msg="tick %d: orphans" % t)
    m.dispatched(so["head"], len(b["assign"]))
    assert a["result"]["log_head"] == len(m.g2o), "tick %d: log head" % t
    return b


def _compact(g, m, o=None):
    out = g.compact_log()
    m.compacted(out["kept"])
    if o is not None:  # the survivors are exactly the oracle's live entries
        live = np.flatnonzero(o.export()["log"] >= 0)
        np.testing.assert_array_equal(m.g2o, live, err_msg="kept entries")
    return out


def _final(g, o, m):
    sg, so = g.read_state(), o.export()
    np.testing.assert_array_equal(sg["reg"], so["reg"], err_msg="final reg")
    reg = so["reg"].astype(bool)
    np.testing.assert_array_equal(sg["free"][reg], so["free"][reg], err_msg="final free")
    np.testing.assert_array_equal(sg["queue"], so["queue"], err_msg="final queue")
    np.testing.assert_array_equal(sg["log"], so["log"][m.g2o], err_msg="final log")


# ------------------------------------------------------------------ 2. stale entries present
def _run_without_log_reads(g, scen):
    carried, n_orph = 0, 0
    for tk in scen["ticks"]:
        n = carried + tk["n_new"]
        seq = np.full(len(tk["ev_kind"]), -1, np.int64)
        a = g.tick(tk["now"], scen["tte"], tk["ev_kind"], tk["ev_slot"], tk["ev_val"], tk["ev_ts"], seq, n)
        n_orph += len(a["orphans"])
        carried = n + len(a["orphans"]) - len(a["assign"])
        g.read_state(with_log=False)  # (never the log: the lazily kept entries stay)
    return n_orph


@pytest.mark.parametrize("lazy", [1, 0])
@pytest.mark.parametrize("seed", range(4))
def test_stale_entries_against_the_host_path(seed, lazy):
    """Ticks in which workers with in-flight tasks expire leave their redistributed entries
    in the log (lazy clears); the compaction tests liveness itself and ends where a twin
    that took the host path (which settles the log first) ends."""
    W = [48, 300][seed % 2]
    scen = synth.random_scenario(4200 + seed, W=W, n_ticks=6, max_events=[30, 200][seed % 2], max_new=[60, 300][seed % 2])
    st = _state_of(scen)
    twins = []
    for _ in range(2):
        g = GpuBalancer(W, len(st["log"]) + 20000, max_events=256)
        g.set_path("lazy", lazy)
        g.load(st)
        g.timing_enable(True)
        twins.append(g)
    n_orph = [_run_without_log_reads(g, scen) for g in twins]
    assert n_orph[0] == n_orph[1] and n_orph[0] > 0, "no worker with in-flight tasks expired"
    dev, host = twins
    for g in twins:
        g.timing_read()  # (the ticks' launches)
    out = dev.compact_log()
    kept = host_compact(host)
    np.testing.assert_array_equal(out["kept"], kept, err_msg="kept")
    names = dev.timing_read()
    assert "lc_flag" in names and "lc_scan" in names and "lc_move" in names, names
    assert "settle" not in names, names  # liveness tested in the flag pass, no k_log_normalize
    if lazy:
        assert "settle" in host.timing_read()  # the host path had stale entries to clear
    _same_state(dev.read_state(), host.read_state(), "seed %d" % seed)
    np.testing.assert_array_equal(dev.inflight(), host.inflight())
    # and they go on alike
    tk = synth.empty_tick(scen["ticks"][-1]["now"] + 1.0)
    a = dev.tick(tk["now"], scen["tte"], n_pending=25)
    b = host.tick(tk["now"], scen["tte"], n_pending=25)
    for k in ("assign", "orphans", "evicted"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    _same_state(dev.read_state(), host.read_state(), "seed %d after a tick" % seed)
    for g in twins:
        g.close()


# ------------------------------------------------------------------ 3. continue vs the oracle
def _continue_vs_oracle(seed, setup):
    scen = synth.random_scenario(7300 + seed, W=48, n_ticks=6 + seed % 3, max_events=40, max_new=70)
    st = _state_of(scen)
    cap = len(st["log"]) + 4000
    g = GpuBalancer(48, cap, max_events=64)
    setup(g)
    g.load(st)
    o = Oracle(48, cap)
    o.load(st["reg"], st["free"], st["hb"], st["epoch"], st["queue"], st["log"])
    m = SeqMap(len(st["log"]))
    rng = np.random.default_rng(seed)
    carried, compactions = 0, 0
    for t, tk in enumerate(scen["ticks"]):
        n = carried + tk["n_new"]
        b = _tick_pair(g, o, m, tk, scen["tte"], n, t)
        carried = n + len(b["orphans"]) - len(b["assign"])
        if rng.random() < 0.6 or t == 1:
            if rng.random() < 0.5:
                g.read_state(with_log=False)
            _compact(g, m, o)
            compactions += 1
    assert compactions >= 1
    _final(g, o, m)
    g.close()


@pytest.mark.parametrize("seed", range(20))
def test_continue_after_compaction_vs_oracle(seed):
    _continue_vs_oracle(seed, lambda g: None)


@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("path", ["plan", "logscan", "window"])
def test_continue_after_compaction_other_paths(path, seed):
    _continue_vs_oracle(100 + seed, (lambda g: g.set_window(1)) if path == "window" else (lambda g: g.set_path(path, 1)))


def _ev(kind, slot, val, ts):
    return dict(ev_kind=np.asarray(kind, np.uint8), ev_slot=np.asarray(slot, np.int32),
                ev_val=np.asarray(val, np.int32), ev_ts=np.asarray(ts, np.float64),
                ev_pick=np.zeros(len(kind), np.uint32))


def test_slot_dies_reregisters_and_dies_again_across_compactions():
    """Slot 3 holds in-flight tasks and expires (orphans), the log is compacted, it
    registers again and gets tasks (a new epoch, in the new numbering), the log is
    compacted again, and it expires again: both deaths redistribute exactly its tasks."""
    W = 8
    reg = np.ones(W, np.uint8)
    st = dict(reg=reg, free=np.full(W, 2, np.int32), hb=np.full(W, 1000.0), epoch=np.zeros(W, np.uint32),
              queue=np.arange(W, dtype=np.int32), log=np.asarray([3, -1, 3, 5, -1, 3, 1, -1], np.int32))
    g = GpuBalancer(W, 512, max_events=64)
    g.load(st)
    o = Oracle(W, 512)
    o.load(st["reg"], st["free"], st["hb"], st["epoch"], st["queue"], st["log"])
    m = SeqMap(8)
    others = [s for s in range(W) if s != 3]
    n_orph = []

    def beat(now, extra=None):  # everyone but slot 3 stays alive
        tk = _ev([synth.EV_HEARTBEAT] * len(others), others, [0] * len(others), [now] * len(others))
        if extra is not None:
            for k in extra:
                tk[k] = np.concatenate([tk[k], extra[k]])
        return dict(tk, now=now)

    carried = 0
    steps = [(beat(1005.0), 4), (beat(1011.0), 0),                                  # slot 3 expires at 1011
             (beat(1012.0, _ev([synth.EV_REGISTER], [3], [3], [1012.0])), 9),       # back, with tasks
             (beat(1018.0), 0), (beat(1023.0), 2)]                                  # expires again at 1023
    for t, (tk, n_new) in enumerate(steps):
        n = carried + n_new
        b = _tick_pair(g, o, m, tk, 10.0, n, t)
        carried = n + len(b["orphans"]) - len(b["assign"])
        n_orph.append(len(b["orphans"]))
        _compact(g, m, o)
    assert n_orph[1] >= 3 and n_orph[4] >= 1, n_orph
    _final(g, o, m)
    g.close()


# ------------------------------------------------------------------ 4. the pipeline survives
def test_window_pipeline_survives_a_compaction():
    """Level-0 ticks under set_window(1) run as window ticks; after a device compaction the
    window (its offset, tombstones and positions) is where it was, and the next tick
    commits as a window tick with no fallback."""
    st = synth.zipf_state(W=300, seed=3, dead_frac=0.0)
    ticks = synth.stream_ticks(st, n_ticks=6, seed=11, tasks_per_tick=16, results_per_tick=16, dt=0.3,
                               hb_frac=0.01, join_frac=0.0)
    E = max(len(t["ev_kind"]) for t in ticks)
    cap = 3 * len(st["log"]) + 1024
    o = Oracle(300, cap, purge_mode=2)
    o.load(st["reg"], st["free"], st["hb"], st["epoch"], st["queue"], st["log"])
    g = GpuBalancer(300, cap, max_events=max(E, 1))
    g.set_window(1)
    g.load(st)
    m = SeqMap(len(st["log"]))
    carried = 0
    for t, tk in enumerate(ticks):
        n = carried + tk["n_new"]
        b = _tick_pair(g, o, m, tk, 10.0, n, t, seq_o=tk["ev_seq"])
        assert g.last["fill_level"] == 0, "tick %d" % t
        carried = n + len(b["orphans"]) - len(b["assign"])
        if t == 3:
            wt, fb = g.window_stats()
            assert wt >= 2, "window ticks before the compaction: %d (fallbacks %d)" % (wt, fb)
            q_before = g.read_state(with_log=False)["queue"]
            _compact(g, m, o)
            np.testing.assert_array_equal(g.read_state(with_log=False)["queue"], q_before)
        if t == 4:
            assert g.window_stats() == (wt + 1, fb), "the tick after the compaction left the window path"
    _final(g, o, m)
    g.close()


# ------------------------------------------------------------------ 5. deque contexts
@pytest.mark.parametrize("seed", range(3))
def test_deque_twins_device_and_host_path(seed):
    scen = synth.random_deque_scenario(600 + seed, W=40, n_ticks=10, max_events=40, max_new=50)
    st = _state_of(scen)
    twins = []
    for _ in range(2):
        g = GpuBalancer(40, len(st["log"]) + 4000, max_events=64, mode="deque")
        g.load(st)
        twins.append(g)
    dev, host = twins
    carried = 0
    for t, tk in enumerate(scen["ticks"]):
        log = dev.read_state()["log"]
        seq = _resolve_own(log, tk)
        n = carried + tk["n_new"]
        outs = [g.tick(tk["now"], 0.0, tk["ev_kind"], tk["ev_slot"], tk["ev_val"], tk["ev_ts"], seq, n) for g in twins]
        for k in ("reconnect", "assign"):
            np.testing.assert_array_equal(outs[0][k], outs[1][k], err_msg="tick %d: %s" % (t, k))
        carried = n - len(outs[0]["assign"])
        if t % 3 == 2:
            before = dev.read_state()
            out = dev.compact_log()
            np.testing.assert_array_equal(out["kept"], host_compact(host, deque=True), err_msg="tick %d kept" % t)
            want, kept = compact_model(before, deque=True)
            np.testing.assert_array_equal(out["kept"], kept)
        _same_state(dev.read_state(), host.read_state(), "tick %d" % t, keys=("reg", "free", "hb", "queue", "log"))
    for g in twins:
        g.close()


# ------------------------------------------------------------------ 6. refusals change nothing
def _loaded(seed=5, W=48, cap_extra=4000):
    scen = synth.random_scenario(8800 + seed, W=W, n_ticks=2, max_events=30, max_new=40)
    st = _state_of(scen)
    g = GpuBalancer(W, len(st["log"]) + cap_extra, max_events=64)
    g.load(st)
    return g, scen, st


def test_refused_while_a_tick_is_launched():
    g, scen, st = _loaded()
    o = Oracle(48, len(st["log"]) + 4000)
    o.load(st["reg"], st["free"], st["hb"], st["epoch"], st["queue"], st["log"])
    tk = scen["ticks"][0]
    seq = _resolve_own(o.export()["log"], tk)
    g.launch(tk["now"], scen["tte"], tk["ev_kind"], tk["ev_slot"], tk["ev_val"], tk["ev_ts"], seq, 30)
    with pytest.raises(FaasbalError) as e:
        g.compact_log()
    assert e.value.code == _lib.FB_ESTATE
    g.wait()  # the tick then waits and commits as usual
    with pytest.raises(FaasbalError) as e:  # waited, not committed: still refused
        g.compact_log()
    assert e.value.code == _lib.FB_ESTATE
    a = dict(reconnect=g.event_status(), assign=g.assignments(), orphans=g.orphans(), evicted=g.evicted())
    g.commit()
    b = o.tick(tk["now"], scen["tte"], tk["ev_kind"], tk["ev_slot"], tk["ev_val"], tk["ev_ts"], seq, 30)
    for k in ("reconnect", "assign", "orphans", "evicted"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    np.testing.assert_array_equal(g.read_state()["log"], o.export()["log"])
    # staged events pending
    g.stage(tk["now"] + 1.0)
    with pytest.raises(FaasbalError) as e:
        g.compact_log()
    assert e.value.code == _lib.FB_ESTATE
    g.launch_staged(scen["tte"], 0)
    g.wait()
    g.commit()
    e0 = synth.empty_tick(tk["now"] + 1.0)
    o.tick(e0["now"], scen["tte"], e0["ev_kind"], e0["ev_slot"], e0["ev_val"], e0["ev_ts"], e0["ev_seq"], 0)
    assert g.compact_log()["n_kept"] == int((o.export()["log"] >= 0).sum())
    g.close()


def test_refusals_leave_the_state_alone():
    g, scen, st = _loaded(seed=6)
    # some ticks first, so the refused calls meet a deferred commit and lazily kept entries
    carried = 0
    for tk in scen["ticks"]:
        n = carried + tk["n_new"]
        a = g.tick(tk["now"], scen["tte"], tk["ev_kind"], tk["ev_slot"], tk["ev_val"], tk["ev_ts"],
                   np.full(len(tk["ev_kind"]), -1, np.int64), n)
        carried = n + len(a["orphans"]) - len(a["assign"])
    before, infl = g.read_state(), g.inflight()
    live = int((before["log"] >= 0).sum())
    assert live >= 2
    kept = np.full(live, -7, np.int64)
    n = C.c_int64(-7)
    rc = g.lib.fb_log_compact(g.h, -1, kept.ctypes.data_as(C.c_void_p), live - 1, C.byref(n))  # cap too small
    assert rc == _lib.FB_EINVAL and n.value == -7 and (kept == -7).all()
    _same_state(g.read_state(), before, "cap too small")
    for wrong in (live + 1, live - 1, 0):
        with pytest.raises(FaasbalError) as e:
            g.compact_log(expect=wrong)
        assert e.value.code == _lib.FB_ESTATE
        _same_state(g.read_state(), before, "expect %d" % wrong)
    np.testing.assert_array_equal(g.inflight(), infl)
    assert g.compact_log(expect=live)["n_kept"] == live
    g.close()


def test_sharded_context_is_refused():
    from faasbal.sharded import ShardedBalancer
    assert ShardedBalancer.compact_log is None
    try:
        sb = ShardedBalancer(0, 1, 16, 64, max_events=16)
    except FaasbalError as e:
        pytest.skip("a world of one rank does not construct on one GPU: %s" % e)
    n = C.c_int64(-7)
    assert sb.lib.fb_log_compact(sb.h, -1, None, 0, C.byref(n)) == _lib.FB_ESTATE
    assert n.value == -7
    sb.close()


# ------------------------------------------------------------------ 7. FB_ENOSPC at balancer level
def test_enospc_then_compact_then_rerun():
    """A tick whose dispatches overflow the log fails its wait with FB_ENOSPC and commits
    nothing; fb_log_compact discards it, and the same tick with its result sequences
    remapped succeeds and equals the oracle's (whose log is large enough)."""
    W = 8
    log = np.full(60, -1, np.int32)
    log[[5, 17, 30, 31, 59]] = [1, 2, 1, 4, 2]
    st = dict(reg=np.ones(W, np.uint8), free=np.full(W, 3, np.int32), hb=np.full(W, 1000.0),
              epoch=np.zeros(W, np.uint32), queue=np.arange(W, dtype=np.int32), log=log)
    g = GpuBalancer(W, 64, max_events=16)
    g.load(st)
    o = Oracle(W, 4096)
    o.load(st["reg"], st["free"], st["hb"], st["epoch"], st["queue"], st["log"])
    m = SeqMap(60)
    tk = dict(_ev([synth.EV_RESULT, synth.EV_RESULT, synth.EV_HEARTBEAT], [1, 2, 3], [0, 0, 0], [1001.0] * 3), now=1001.0)
    seq_o = np.asarray([30, 59, -1], np.int64)
    before = g.read_state()
    with pytest.raises(FaasbalError) as e:
        g.tick(tk["now"], 10.0, tk["ev_kind"], tk["ev_slot"], tk["ev_val"], tk["ev_ts"], m.to_gpu(seq_o), 20)
    assert e.value.code == _lib.FB_ENOSPC
    out = _compact(g, m, o)
    np.testing.assert_array_equal(out["kept"], [5, 17, 30, 31, 59])
    want, _ = compact_model(before)
    _same_state(g.read_state(), want, "after the compaction")
    np.testing.assert_array_equal(m.to_gpu(seq_o), [2, 4, -1])
    b = _tick_pair(g, o, m, tk, 10.0, 20, 0, seq_o=seq_o)
    assert len(b["assign"]) == 20
    _final(g, o, m)
    g.close()
