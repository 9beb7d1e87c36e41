"""A shard group's log compaction on the GPU: fb_log_compact_shard_mark / _apply behind
LocalShardGroup.compact_log (every rank's context on one device, the bitmaps summed there).

The reference of every comparison is tests/lc_model.compact_model applied to the merged state
read before the compaction, split per rank again (the helpers of
tests/test_log_compact_shard_host.py, which run the same checks over model ranks).
"""
import ctypes as C

import numpy as np
import pytest

from faasbal import FaasbalError, GpuBalancer, _lib, synth
from faasbal._lib import FB_EINVAL, FB_ENOSPC, FB_ESTATE
from faasbal.sharded import LocalShardGroup, shard_range
from lc_model import compact_model
from test_log_compact_shard_host import (HEADS, MARKED, _run_ticks, _scenario_state, check_group_compaction,
                                         random_state)

pytestmark = pytest.mark.gpu

KERNELS = ("lcs_flag", "lcs_mark", "lcs_count", "lcs_move")


def _rank_states(g):
    return [b.read_state() for b in g.bals]


def _same(a, b, what, keys=("reg", "free", "hb", "epoch", "queue", "log", "head")):
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg="%s: %s" % (what, k))


# ------------------------------------------------------------------ 1. against the model
@pytest.mark.parametrize("world", (1, 2, 3, 4))
def test_ticked_states_against_the_model(world):
    """States reached by ticks that carry results, evictions and re-registrations."""
    for seed, W in ((7311, 37), (7312, 300)):
        scen, st = _scenario_state(seed, W)
        g = LocalShardGroup(world, W, len(st["log"]) + 4096, max_events=256)
        g.load(st)
        for b in g.bals:
            b.timing_enable(True)
        ref, carried = _run_ticks(g, scen, scen["ticks"][:3], g.read_state())
        assert (ref["log"] < 0).any() and (ref["log"] >= 0).any() and ref["head"] > 20
        for b in g.bals:
            b.timing_read()
        post = check_group_compaction(g, lambda: _rank_states(g), world, W)
        assert 0 < post["head"] < ref["head"]
        for b in g.bals:  # the library's own kernels ran, on every rank
            names = b.timing_read()
            assert all(k in names for k in KERNELS) and "lc_scan" in names, names
        # on: the next tick's results name the new sequences, then a compaction without a list
        ref, carried = _run_ticks(g, scen, scen["ticks"][3:], post, carried)
        want, kept = compact_model(ref)
        assert g.compact_log(expect=len(kept), want_kept=False) == {"n_kept": len(kept), "kept": None}
        _same(g.read_state(), dict(want, head=len(kept)), "W %d, second compaction" % W)
        # compacting a compacted log keeps everything
        again = g.compact_log()
        np.testing.assert_array_equal(again["kept"], np.arange(len(kept)))
        _same(g.read_state(), dict(want, head=len(kept)), "W %d, twice" % W)
        g.close()


@pytest.mark.parametrize("world,W", ((1, 41), (2, 41), (3, 300), (4, 5)))
def test_loaded_heads_against_the_model(world, W):
    """Directly loaded states at the heads where a tile or a word ends; W = 5 over four ranks
    leaves the last without a slot; the folded log leaves all ranks but the first an empty shard."""
    rng = np.random.default_rng(5100 + world)
    g = LocalShardGroup(world, W, 3 * 2048 + 64, max_events=64)
    if (world, W) == (4, 5):
        assert shard_range(W, world, 3)[1] == 0
    for head in HEADS:
        for variant in ("random", "far epochs", "all", "none", "first rank"):
            st = random_state(rng, W, head, epoch_hi=head + 70 if variant == "far epochs" else None,
                              p_done=0.0 if variant == "all" else 1.0 if variant == "none" else 0.3,
                              p_reg=1.0 if variant == "all" else 0.8)
            if variant == "all":
                st["epoch"][:] = 0
            if variant == "first rank":
                n0 = max(shard_range(W, world, 0)[1], 1)
                st["log"] = np.where(st["log"] >= 0, st["log"] % n0, -1).astype(np.int32)
            g.load(st)
            post = check_group_compaction(g, lambda: _rank_states(g), world, W)
            what = "world %d head %d %s" % (world, head, variant)
            if variant == "all":
                assert post["head"] == head, what
            if variant == "none":
                assert post["head"] == 0, what
            if variant == "first rank" and world > 1 and head > 64:
                assert post["head"] > 0 and all(s["log_len"] == 0 for s in _rank_states(g)[1:]), what
    g.close()


def test_world_1_is_fb_log_compact():
    """A group of one rank ends where fb_log_compact ends on a one-GPU context of the same state."""
    scen, st = _scenario_state(7313, 48)
    g = LocalShardGroup(1, 48, len(st["log"]) + 4096, max_events=256)
    o = GpuBalancer(48, len(st["log"]) + 4096, max_events=256)
    g.load(st)
    o.load(st)
    ref = g.read_state()
    for tk in scen["ticks"][:3]:
        seq = np.full(len(tk["ev_kind"]), -1, np.int64)
        for i in np.nonzero(tk["ev_kind"] == synth.EV_RESULT)[0]:
            mine = np.nonzero(ref["log"] == tk["ev_slot"][i])[0]
            if len(mine):
                seq[i] = mine[tk["ev_pick"][i] % len(mine)]
        a = g.tick(tk["now"], scen["tte"], tk["ev_kind"], tk["ev_slot"], tk["ev_val"], tk["ev_ts"], seq, tk["n_new"])
        b = o.tick(tk["now"], scen["tte"], tk["ev_kind"], tk["ev_slot"], tk["ev_val"], tk["ev_ts"], seq, tk["n_new"])
        np.testing.assert_array_equal(a["assign"], b["assign"])
        ref = g.read_state()
    x, y = g.compact_log(), o.compact_log()
    assert x["n_kept"] == y["n_kept"] > 0
    np.testing.assert_array_equal(x["kept"], y["kept"])
    _same(g.read_state(), o.read_state(), "world 1")
    g.close()
    o.close()


# ------------------------------------------------------------------ 2. the pipeline survives
@pytest.mark.parametrize("world", (2, 3))
def test_tick_after_compaction_is_the_twins(world):
    """A tick after a compaction gives the assignments, orphans and evicted slots of the same
    tick on a twin that never compacted, modulo the renumbering, with no more reruns."""
    scen, st = _scenario_state(7314, 300)
    twins = []
    for _ in range(2):
        g = LocalShardGroup(world, 300, len(st["log"]) + 8192, max_events=256)
        g.load(st)
        twins.append(g)
    g, h = twins
    g2h = np.arange(len(st["log"]), dtype=np.int64)  # h's sequence of g's entry q
    carried, compactions, orphans = 0, 0, 0
    for t, tk in enumerate(scen["ticks"] + [synth.empty_tick(scen["ticks"][-1]["now"] + 0.5, 20)]):
        hlog = h.read_state()["log"]
        seq_h = np.full(len(tk["ev_kind"]), -1, np.int64)
        for i in np.nonzero(tk["ev_kind"] == synth.EV_RESULT)[0]:
            mine = np.nonzero(hlog == tk["ev_slot"][i])[0]
            if len(mine) and tk["ev_pick"][i] % 5 != 4:
                seq_h[i] = mine[tk["ev_pick"][i] % len(mine)]
        j = np.searchsorted(g2h, seq_h)
        seq_g = np.where(seq_h >= 0, j, -1)
        assert (g2h[j[seq_h >= 0]] == seq_h[seq_h >= 0]).all()  # (a live entry was kept)
        n = carried + tk["n_new"]
        args = (tk["now"], scen["tte"], tk["ev_kind"], tk["ev_slot"], tk["ev_val"], tk["ev_ts"])
        a, b = g.tick(*args, seq_g, n), h.tick(*args, seq_h, n)
        for k in ("assign", "evicted", "reconnect"):
            np.testing.assert_array_equal(a[k], b[k], err_msg="tick %d: %s" % (t, k))
        np.testing.assert_array_equal(g2h[a["orphans"]], b["orphans"], err_msg="tick %d: orphans" % t)
        for k in ("n_assigned", "fill_level", "max_free", "queue_len"):
            assert a["result"][k] == b["result"][k], (t, k)
        # fb_load_shard's reset (a narrow round table, a relaunch) did not happen
        assert a["result"]["reruns"] <= b["result"]["reruns"], (t, a["result"], b["result"])
        orphans += len(b["orphans"])
        g2h = np.concatenate([g2h, b["result"]["log_head"] - len(b["assign"]) + np.arange(len(b["assign"]), dtype=np.int64)])
        carried = n + len(b["orphans"]) - len(b["assign"])
        if t >= 1:
            out = g.compact_log()
            g2h = g2h[out["kept"]]
            compactions += 1
            np.testing.assert_array_equal(g2h, np.flatnonzero(h.read_state()["log"] >= 0))
    assert compactions >= 3 and orphans > 0
    sg, sh = g.read_state(), h.read_state()
    _same(sg, sh, "final", keys=("reg", "free", "hb", "queue"))
    np.testing.assert_array_equal(sg["log"], sh["log"][g2h])
    for g in twins:
        g.close()


# ------------------------------------------------------------------ 3. refusals change nothing
def _raises(code, f, *a, needle=None):
    with pytest.raises(FaasbalError) as e:
        f(*a)
    assert e.value.code == code, e.value
    if needle is not None:
        assert needle in str(e.value), e.value


def _sum_exchange(g, views):
    import torch
    torch.cuda.synchronize()
    total = views[0].clone()
    for x in views[1:]:
        total += x
    for x in views:
        x.copy_(total)
    torch.cuda.synchronize()


def _finish_tick(g):
    """The rest of a tick whose phase 1 every rank has enqueued (LocalShardGroup's steps)."""
    for b in g.bals:
        n = C.c_int64()
        b._chk(b.lib.fb_exchange_bytes(b.h, b._E, C.byref(n)))
        b._xbytes = n.value
    _sum_exchange(g, [b.exchange() for b in g.bals])
    for b in g.bals:
        b.cont()
    for b in g.bals:
        b.wait()
    for b in g.bals:
        b.commit()


def test_refusals_change_nothing():
    scen, st = _scenario_state(7315, 37)
    g = LocalShardGroup(2, 37, len(st["log"]) + 4096, max_events=256)
    g.load(st)
    _run_ticks(g, scen, scen["ticks"][:2], g.read_state())
    b0, b1 = g.bals
    before = _rank_states(g)

    def unchanged(what):
        for r, (x, y) in enumerate(zip(_rank_states(g), before)):
            _same(x, y, "%s, rank %d" % (what, r))
            np.testing.assert_array_equal(x["log_seq"], y["log_seq"], err_msg=what)
            assert x["log_len"] == y["log_len"], what

    # a one-GPU context
    o = GpuBalancer(37, len(st["log"]) + 64, max_events=64)
    o.load(st)
    so = o.read_state()
    n = C.c_int64()
    for rc in (o.lib.fb_log_compact_shard_bytes(o.h, C.byref(n)), o.lib.fb_log_compact_shard_mark(o.h, None, 0, C.byref(n)),
               o.lib.fb_log_compact_shard_apply(o.h, 0, None, 0, C.byref(n))):
        assert rc == FB_ESTATE
    assert "one-GPU context" in o.lib.fb_last_error(o.h).decode()
    assert o.lib.fb_log_compact_shard_cancel(o.h) == _lib.FB_OK
    _same(o.read_state(), so, "one-GPU context")
    o.close()
    # a buffer too small or misaligned
    view = b0.compact_exchange()
    assert view.numel() == b0.compact_bytes() > 0
    for ptr, nbytes in ((b0._cbuf.data_ptr(), view.numel() - 1), (b0._cbuf.data_ptr() + 4, view.numel()), (0, view.numel())):
        assert b0.lib.fb_log_compact_shard_mark(b0.h, C.c_void_p(ptr), nbytes, C.byref(n)) == FB_EINVAL
    unchanged("bad buffer")
    # staged events
    for b in g.bals:
        b.stage(scen["ticks"][2]["now"])
    _raises(FB_ESTATE, b0.compact_mark, needle="staged events")
    with pytest.raises(FaasbalError):
        g.compact_log()
    # a tick in flight: phase 1 enqueued, then phase 2 enqueued and not waited for
    for b in g.bals:
        b.launch_staged(scen["tte"], 0)
    _raises(FB_ESTATE, b0.compact_mark, needle="tick in flight")
    for b in g.bals:
        n = C.c_int64()
        b._chk(b.lib.fb_exchange_bytes(b.h, b._E, C.byref(n)))
        b._xbytes = n.value
    _sum_exchange(g, [b.exchange() for b in g.bals])
    for b in g.bals:
        b.cont()
    _raises(FB_ESTATE, b1.compact_mark, needle="tick in flight")
    for b in g.bals:
        b.wait()
    for b in g.bals:
        b.commit()
    before = _rank_states(g)  # (an idle tick: the heartbeat clock moved nothing, the queue may have)
    # apply without a mark
    _raises(FB_ESTATE, b0.compact_apply, 5, needle="without fb_log_compact_shard_mark")
    unchanged("apply without a mark")
    # apply with a wrong total: nothing changes and the mark is dropped
    live = [b.compact_mark() for b in g.bals]
    _sum_exchange(g, [b.compact_exchange() for b in g.bals])
    for b in g.bals:
        _raises(FB_ESTATE, b.compact_apply, sum(live) + 1, needle="the group agreed on")
        _raises(FB_ESTATE, b.compact_apply, sum(live), needle="without fb_log_compact_shard_mark")
    unchanged("wrong total")
    # cap too small: FB_EINVAL, nothing changes; the mark stays
    live = [b.compact_mark() for b in g.bals]
    _sum_exchange(g, [b.compact_exchange() for b in g.bals])
    kept = np.zeros(sum(live), np.int64)
    assert b0.lib.fb_log_compact_shard_apply(b0.h, sum(live), kept.ctypes.data_as(C.c_void_p), sum(live) - 1,
                                             C.byref(n)) == FB_EINVAL
    # marked: the log is not read, no tick is launched, no second mark
    _raises(FB_ESTATE, b0.read_state, needle=MARKED)
    _raises(FB_ESTATE, b0.compact_mark, needle=MARKED)
    _raises(FB_ESTATE, b0.launch, 2000.0, scen["tte"], needle=MARKED)
    _raises(FB_ESTATE, b0.pool_stats_part, 2000.0, scen["tte"], needle=MARKED)
    assert b0.compact_bytes() == view.numel()
    # cancel restores normal service
    for b in g.bals:
        b.compact_cancel()
        b.compact_cancel()
    unchanged("cap too small, marked, cancelled")
    g.tick(scen["ticks"][2]["now"] + 0.25, scen["tte"], n_pending=9)
    check_group_compaction(g, lambda: _rank_states(g), 2, 37)
    g.close()


# ------------------------------------------------------------------ 4. one rank's shard is full
def _results(log, picks):
    """A result message per picked live entry: (kind, slot, val, seq)."""
    q = np.asarray(picks, np.int64)
    return (np.full(len(q), synth.EV_RESULT, np.uint8), log[q].astype(np.int32), np.zeros(len(q), np.int32), q)


def test_full_shard_on_one_rank_compacts_and_reruns():
    """Rank 0's shard is full (FB_ENOSPC) while rank 1 waited and did not commit; the group
    compacts, and the discarded tick -- launched again with remapped result sequences -- gives
    the outputs of a twin whose log never filled."""
    W, tte = 8, 100.0
    st = dict(reg=np.ones(W, np.uint8), free=np.asarray([20] * 4 + [2] * 4, np.int32), hb=np.full(W, 1000.0),
              epoch=np.zeros(W, np.uint32), queue=np.arange(W, dtype=np.int32), log=np.zeros(0, np.int32))
    g = LocalShardGroup(2, W, 64, max_events=128)
    h = LocalShardGroup(2, W, 4096, max_events=128)
    for x in (g, h):
        x.load(st)
        a = x.tick(1001.0, tte, n_pending=60)
        assert len(a["assign"]) == 60
    log = g.read_state()["log"]
    r0, r1 = np.flatnonzero(log < 4), np.flatnonzero(log >= 4)
    # (room for the 30 results below, a full shard at the third tick, room again once compacted)
    assert 45 <= len(r0) <= 54 and len(r1) >= 6 and len(r0) + len(r1) == 60
    k, s, v, q = _results(log, np.sort(np.concatenate([r0[:30], r1[:4]])))
    for x in (g, h):
        x.tick(1002.0, tte, k, s, v, np.full(len(k), 1002.0), q, 0)
    # the tick that overflows rank 0's shard: 5 + 2 results, 40 tasks
    k, s, v, q = _results(log, np.sort(np.concatenate([r0[30:35], r1[4:6]])))
    ts = np.full(len(k), 1003.0)
    pre, pre_all = _rank_states(g), g.read_state()
    with pytest.raises(FaasbalError) as e:
        g.tick(1003.0, tte, k, s, v, ts, q, 40)
    assert e.value.code == FB_ENOSPC and "log full" in str(e.value)
    # (the discarded tick's results completed nothing: its clears are taken back on both ranks)
    want, kept = compact_model(pre_all)
    assert len(kept) == 60 - 34
    out = g.compact_log(expect=len(kept))
    np.testing.assert_array_equal(out["kept"], kept)
    post = g.read_state()
    np.testing.assert_array_equal(post["log"], want["log"])
    np.testing.assert_array_equal(post["epoch"], want["epoch"])
    for r, (x, y) in enumerate(zip(_rank_states(g), pre)):
        _same(x, y, "rank %d" % r, keys=("reg", "free", "hb", "queue"))
    a = g.tick(1003.0, tte, k, s, v, ts, np.searchsorted(kept, q), 40)
    b = h.tick(1003.0, tte, k, s, v, ts, q, 40)
    assert len(b["assign"]) > 30
    for key in ("assign", "evicted", "reconnect", "orphans"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    g2h = np.concatenate([kept, 60 + np.arange(len(b["assign"]), dtype=np.int64)])
    sg, sh = g.read_state(), h.read_state()
    _same(sg, sh, "after the rerun", keys=("reg", "free", "hb", "queue"))
    np.testing.assert_array_equal(sg["log"], sh["log"][g2h])
    g.close()
    h.close()


# ------------------------------------------------------------------ 5. the drop-in
@pytest.mark.parametrize("world", (2, 3))
@pytest.mark.parametrize("name", ("small_log", "enospc"))
def test_dispatcher_compacts_a_group_on_the_device(name, world):
    """GpuPushDispatcher over a LocalShardGroup with a small per-rank log: the messages of a
    run whose log never fills, every compaction on the device, and after every tick the merged
    device log is the dispatcher's in-flight table."""
    from faasbal.dispatcher import GpuPushDispatcher
    from test_log_compact_host import SCENARIOS
    run, cap = SCENARIOS[name]

    def make(host, port, tte, **kw):
        group = LocalShardGroup(world, kw["max_workers"], kw["max_inflight"], max_events=kw["max_events"])
        d = GpuPushDispatcher(host, port, tte, balancer=group, **kw)
        group.reads = reads = []
        read = group.read_state
        tick = d.tick

        def checked_tick(*a, **k):
            out = tick(*a, **k)
            log = read()["log"]
            assert d.head == len(log), (d.head, len(log))
            assert {q: s for q, (_, s) in d.inflight.items()} == {int(q): int(log[q]) for q in np.flatnonzero(log >= 0)}
            return out
        d.tick = checked_tick
        group.read_state = lambda *a, **k: (reads.append(k), read(*a, **k))[1]
        return d

    big, d0 = run(make, 1 << 14)
    small, d = run(make, cap)
    assert d0.compactions == 0 and small == big and sum(len(x) for x in big) > 50
    assert d.device_compactions == d.compactions > 0
    assert not d.balancer.reads  # the dispatcher itself never read the state
    d0.balancer.close()
    d.balancer.close()


# ------------------------------------------------------------------ 6. across processes
def _dist_main(rank, port, errq):
    """Two processes on one GPU over gloo, library contexts on both: the bitmap travels through
    torch.distributed.all_reduce on the balancer's stream, the headers through all_gather."""
    from test_gpu_shard_dist import _setup
    dist = _setup(rank, port)
    from faasbal.sharded import DistShardGroup, ShardedBalancer, serve_shard
    try:
        scen, st = _scenario_state(7316, 300)
        bal = ShardedBalancer(rank, 2, 300, len(st["log"]) + 8192, max_events=256, device=0)
        if rank != 0:
            serve_shard(bal)
            bal.read_state()  # (no mark is left standing: the context still answers)
            return
        g = DistShardGroup(bal, 300)
        assert callable(g.compact_log)
        g.load(st)
        ref, carried = _run_ticks(g, scen, scen["ticks"][:3], g.read_state())
        want, kept = compact_model(ref)
        assert 0 < len(kept) < ref["head"]
        # a wrong expect: FB_ESTATE, every rank cancelled, every shard as it was
        with pytest.raises(FaasbalError) as e:
            g.compact_log(expect=len(kept) + 1)
        assert e.value.code == FB_ESTATE
        _same(g.read_state(), ref, "wrong expect")
        out = g.compact_log(expect=len(kept))
        np.testing.assert_array_equal(out["kept"], kept)
        post = g.read_state()
        _same(post, dict(want, head=len(kept)), "over gloo")
        # the group goes on: results name the new sequences
        ref, carried = _run_ticks(g, scen, scen["ticks"][3:], post, carried)
        want, kept = compact_model(ref)
        assert g.compact_log(want_kept=False) == {"n_kept": len(kept), "kept": None}
        _same(g.read_state(), dict(want, head=len(kept)), "over gloo, no kept list")
        g.close()
    except Exception as e:  # report to the parent, keep the peer from hanging
        errq.put("rank %d: %r" % (rank, e))
        raise
    finally:
        dist.destroy_process_group()


def test_dist_group_compacts_over_gloo_on_one_gpu():
    from test_gpu_shard_dist import _spawn
    _spawn(_dist_main, ())
