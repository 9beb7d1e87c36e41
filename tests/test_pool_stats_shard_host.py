"""A shard group's pool summary without a GPU: the parts and their merge.

1. merge_summaries over pool_stats_part_model of every rank's split_state equals
   pool_stats_model of the whole state, for worlds with empty ranks too; the merge's refusals.
2. fb_pool_merge (host arithmetic: the library loads without a GPU) equals merge_summaries,
   refusals included.
3. fb_pool_stats_shard's gate (life_gate's Call::pool_stats_shard, asked of tests/life_probe.cpp):
   on the sharded kind fb_pool_stats' refusals and duties with the sharded refusal set aside, on
   the one-GPU kinds a refusal.  (tests/test_life.py runs the probe under the sanitizers.)
4. DistShardGroup's "stats" message over gloo, two processes, model ranks.
5. GpuPushDispatcher.pool_stats takes a group's summary where the group has one and reads
   the state where it has none.
"""
import ctypes as C
import os
import socket

import numpy as np
import pytest

import life_cases as lc
from faasbal import _lib, synth
from faasbal.poolstats import (MAX_EDGES, diff_summary, merge_summaries, pool_stats_model,
                               pool_stats_part_model)
from faasbal.sharded import split_state
from shard_model_balancer import ModelRankBalancer
from test_gpu_pool_stats import _shape_state
from test_life import _asker, _build, _gate

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
NOW, TTE = 1000.0, 10.0
EDGES15 = tuple(float(i) for i in range(1, 16))
WORLDS = (1, 2, 3, 8)


def _hand_states():
    """Small states written out: an empty table's neighbour (one slot), a table whose live
    slots all sit in one rank's range, and one whose only heartbeats are NaN."""
    one = dict(reg=np.ones(1, np.uint8), free=np.asarray([3], np.int32), hb=np.asarray([NOW - 1.0]),
               epoch=np.zeros(1, np.uint32), queue=np.asarray([0], np.int32), log=np.asarray([0, -1, 0], np.int32))
    W = 9
    reg = np.asarray([0, 0, 0, 0, 0, 0, 1, 1, 1], np.uint8)
    left = dict(reg=reg, free=np.asarray([0] * 6 + [2, 0, 5], np.int32),
                hb=np.asarray([0.0] * 6 + [NOW - 2.0, NOW - 11.0, NOW - 3.5]), epoch=np.asarray([0] * 6 + [0, 1, 2], np.uint32),
                queue=np.asarray([8, 7, 6], np.int32), log=np.asarray([7, 7, 8, 6, -1, 8], np.int32))
    nan = dict(left, hb=np.where(reg != 0, np.nan, 0.0))
    assert W == len(reg)
    return [("one", one), ("one_rank_owns_all", left), ("nan_heartbeats", nan)]


def _states():
    out = _hand_states()
    for i, (W, head, Q) in enumerate(((5, 7, 3), (257, 2049, 257), (1025, 300, 64))):
        out.append(("shape_w%d" % W, _shape_state(W, head, Q, np.random.default_rng(900 + i))))
    return out


def _parts(st, world, now, tte, edges):
    got = [pool_stats_part_model(split_state(st, world, r), now, tte, edges) for r in range(world)]
    return [p for p, _ in got], [q for _, q in got]


# ------------------------------------------------------------------ 1. the merge model
@pytest.mark.parametrize("world", WORLDS)
def test_merged_parts_are_the_whole(world):
    for name, st in _states():
        for now, tte, edges in ((NOW, TTE, ()), (NOW, TTE, EDGES15), (NOW + 100.0, TTE, (1.0, 2.0)), (NOW, 1e300, (10.0,))):
            parts, qlens = _parts(st, world, now, tte, edges)
            want = pool_stats_model(st, now, tte, edges, inflight_counts=False)
            d = diff_summary(merge_summaries(parts, qlens), want)
            assert not d, (name, world, now, tte, d)
            assert all(q == len(st["queue"]) for q in qlens)
            assert [p["n_slots"] for p in parts] == [split_state(st, world, r)["n"] for r in range(world)]
            if name == "shape_w257" and edges == EDGES15:  # the state has what the test is about
                assert 0 < want["n_expired"] < want["n_registered"] and want["inflight"] > 0 < want["inflight_expired"]
                assert want["n_queued"] > 0 < want["n_queued_expired"] and (want["age_hist"] > 0).all()
                assert want["log_head"] - want["inflight"] - want["inflight_expired"] > 0
                if world > 1:
                    assert sum(p["n_queued"] > 0 for p in parts) >= 2
                if world > 2:  # (the live entries sit on the first 128 slots: one rank's at world 2)
                    assert sum(p["inflight"] > 0 for p in parts) >= 2
    if world == 8:  # ranks without a slot exist, and hold nothing
        parts, _ = _parts(dict(_states())["shape_w5"], 8, NOW, TTE, ())
        assert [p["n_slots"] for p in parts] == [1] * 5 + [0] * 3
        assert all(p["n_registered"] == p["inflight"] == p["n_queued"] == 0 for p in parts[5:])


def test_merge_skips_parts_without_a_heartbeat():
    sts = dict(_hand_states())
    # one part NaN: rank 0 of 2 owns slots 0 .. 4, none registered
    parts, qlens = _parts(sts["one_rank_owns_all"], 2, NOW, TTE, ())
    assert np.isnan(parts[0]["oldest_hb"]) and not np.isnan(parts[1]["oldest_hb"])
    m = merge_summaries(parts, qlens)
    assert (m["oldest_hb"], m["newest_hb"]) == (NOW - 3.5, NOW - 2.0)  # (slot 7 is expired)
    # every part NaN
    parts, qlens = _parts(sts["nan_heartbeats"], 3, NOW, TTE, ())
    m = merge_summaries(parts, qlens)
    assert np.isnan(m["oldest_hb"]) and np.isnan(m["newest_hb"])
    # inflight_max: -1 as soon as one part keeps no counts, else the maximum
    a, b = dict(parts[0], inflight_max=4), dict(parts[1], inflight_max=9)
    assert merge_summaries([a, b, parts[2]], qlens)["inflight_max"] == -1
    assert merge_summaries([a, b, dict(parts[2], inflight_max=0)], qlens)["inflight_max"] == 9


def _bad_merges():
    """(what, parts, queue_lens) the merge refuses, from a good three-rank set."""
    st = dict(_states())["shape_w257"]
    parts, qlens = _parts(st, 3, NOW, TTE, (10.0,))
    merge_summaries(parts, qlens)
    return [("log_head", [parts[0], dict(parts[1], log_head=parts[1]["log_head"] + 1), parts[2]], qlens),
            ("queue_len", parts, [qlens[0], qlens[1] + 1, qlens[2]]),
            ("queue sum short", [parts[0], dict(parts[1], n_queued=parts[1]["n_queued"] - 1), parts[2]], qlens),
            ("queue sum long", parts, [q + 1 for q in qlens]),
            ("no parts", [], [])]


def test_merge_refusals():
    for what, parts, qlens in _bad_merges():
        with pytest.raises(ValueError):
            merge_summaries(parts, qlens)
            pytest.fail(what)


# ------------------------------------------------------------------ 2. fb_pool_merge
def _c_summary(d):
    s = _lib.PoolSummary()
    for k, _ in s._fields_[:-2]:
        setattr(s, k, d[k])
    for k in ("free_hist", "age_hist"):
        for i, v in enumerate(d[k]):
            getattr(s, k)[i] = int(v)
    return s


def _c_merge(lib, parts, qlens, out=None):
    arr = (_lib.PoolSummary * max(len(parts), 1))(*[_c_summary(p) for p in parts])
    q = (C.c_int64 * max(len(qlens), 1))(*qlens)
    out = _lib.PoolSummary() if out is None else out
    rc = lib.fb_pool_merge(None, arr, q, len(parts), C.byref(out))
    d = {k: getattr(out, k) for k, _ in out._fields_[:-2]}
    d["free_hist"], d["age_hist"] = np.array(out.free_hist, np.int64), np.array(out.age_hist, np.int64)
    return rc, d


def test_fb_pool_merge_is_the_model():
    lib = _lib.load()
    for name, st in _states():
        for world in WORLDS:
            for now, tte, edges in ((NOW, TTE, EDGES15), (NOW + 100.0, TTE, ())):
                parts, qlens = _parts(st, world, now, tte, edges)
                rc, got = _c_merge(lib, parts, qlens)
                assert rc == _lib.FB_OK, (name, world)
                d = diff_summary(got, merge_summaries(parts, qlens))
                assert not d, (name, world, d)
    parts, qlens = _parts(dict(_hand_states())["nan_heartbeats"], 3, NOW, TTE, ())
    rc, got = _c_merge(lib, [dict(p, inflight_max=i) for i, p in enumerate(parts)], qlens)
    assert rc == _lib.FB_OK and got["inflight_max"] == 2 and np.isnan(got["oldest_hb"]) and np.isnan(got["newest_hb"])


def test_fb_pool_merge_refusals():
    lib = _lib.load()
    for what, parts, qlens in _bad_merges():
        out = _lib.PoolSummary()
        out.n_slots = -7
        rc, _ = _c_merge(lib, parts, qlens, out)
        assert rc == _lib.FB_EINVAL and out.n_slots == -7, what
    parts, qlens = _parts(dict(_states())["shape_w5"], 2, NOW, TTE, ())
    arr = (_lib.PoolSummary * 2)(*[_c_summary(p) for p in parts])
    q = (C.c_int64 * 2)(*qlens)
    out = _lib.PoolSummary()
    assert lib.fb_pool_merge(None, arr, q, 2, C.byref(out)) == _lib.FB_OK
    assert lib.fb_pool_merge(None, None, q, 2, C.byref(out)) == _lib.FB_EINVAL
    assert lib.fb_pool_merge(None, arr, None, 2, C.byref(out)) == _lib.FB_EINVAL
    assert lib.fb_pool_merge(None, arr, q, 2, None) == _lib.FB_EINVAL
    assert lib.fb_pool_merge(None, arr, q, 0, C.byref(out)) == _lib.FB_EINVAL
    assert lib.fb_pool_merge(None, arr, q, -1, C.byref(out)) == _lib.FB_EINVAL


# ------------------------------------------------------------------ 3. the gate
ONE_GPU_REFUSAL = "fb_pool_stats_shard on a one-GPU context: use fb_pool_stats"
SHARDED_REFUSAL = "fb_pool_stats on a sharded context: the pool is the group's, a summary needs a collective"


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return _asker(_build(tmp_path_factory.mktemp("life_ps_shard"), "life_probe"))


def test_gate_is_pool_stats_gate_without_the_sharded_refusal(probe):
    def ask(kind, states):
        return [_gate(a)[:2] for a in probe(["gate %s %s pool_stats_shard" % (kind, s) for s in states])]

    # the sharded kind: every Life the table reaches, every flag state that stands for it
    by_life = {}
    for r in lc.closure("shard"):
        by_life.setdefault(lc.canon("shard", r), []).append(r)
    states = sorted(by_life)
    assert states == sorted(lc.STATES["shard"])
    seen = set()
    for s, (refuse, duties) in zip(states, ask("shard", states)):
        for r in by_life[s]:
            if r.marked:  # between a compaction's mark and its apply both wait
                assert lc.gate("shard", r, "pool_stats") == (lc.MARKED, []) == (refuse, duties), s
                continue
            assert lc.gate("shard", r, "pool_stats") == (SHARDED_REFUSAL, [])
            # ... set aside: the ladder of a one-GPU kind with in-place clears, the same flags
            assert lc.gate("deque", r, "pool_stats") == (refuse, duties), (s, r, refuse, duties)
        seen.add((refuse, tuple(duties)))
    # the table has what the test is about: each refusal, a pass, and the undo of a dropped launch
    assert {m for m, _ in seen} == {None, lc.MARKED,
                                    "fb_pool_stats with staged events pending: launch and commit their tick first",
                                    "fb_pool_stats between a tick's wait and its commit: fb_tick_commit first",
                                    "fb_pool_stats with a tick launched: fb_tick_wait and fb_tick_commit first"}
    assert (None, ("undo",)) in seen and (None, ()) in seen
    # one-GPU kinds: refused, whatever the state; at most the flush
    for kind in ("hb", "hb_large", "deque"):
        states = lc.STATES[kind]
        for s, (refuse, duties) in zip(states, ask(kind, states)):
            assert refuse == ONE_GPU_REFUSAL, (kind, s, refuse)
            assert duties == (["flush"] if s.split(",")[5] == "1" else []), (kind, s, duties)


def test_entry_point_goes_through_the_gate():
    api = open(os.path.join(REPO, "distributed-faas_amd", "csrc", "faasbal_api.hip")).read()
    body = api[api.index("static int pool_stats_run(fb_ctx *c, bool shard"):]
    body = body[:body.index("\n}\n")]
    assert "enter(c, shard ? Call::pool_stats_shard : Call::pool_stats)" in body
    assert body.index("enter(c, ") < body.index("launch_ps_slots") and "hipMemcpy" not in body[:body.index("enter(c, ")]
    assert "X(pool_stats_shard)" in open(os.path.join(REPO, "distributed-faas_amd", "csrc", "faasbal_life.h")).read()


# ------------------------------------------------------------------ 4. the wire format over gloo
class PartRank(ModelRankBalancer):
    """The model rank with a part of the summary: the part model on its shard."""
    fail_next = False

    def pool_stats_part(self, now, tte, age_edges=()):
        if self.fail_next:
            self.fail_next = False
            raise _lib.FaasbalError(_lib.FB_EHIP, "summary failed (injected)")
        return pool_stats_part_model(self.read_state(), now, tte, age_edges)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _gloo_rank(rank, world, port, errq):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    from faasbal.sharded import DistShardGroup, serve_shard
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        scen = synth.random_scenario(7301, W=37, n_ticks=3, max_events=20, max_new=50)
        st = dict(reg=scen["init_reg"], free=scen["init_free"], hb=scen["init_hb"], epoch=scen["init_epoch"],
                  queue=scen["init_queue"], log=scen["init_log"])
        bal = PartRank(rank, world, 37)
        bal.fail_next = False
        if rank != 0:
            # this rank's second 15-edge summary fails (the sixth it serves)
            served = [0]
            part = bal.pool_stats_part

            def counted(now, tte, age_edges=()):
                served[0] += 1
                bal.fail_next = served[0] == 6
                return part(now, tte, age_edges)
            bal.pool_stats_part = counted
            serve_shard(bal)
            return
        g = DistShardGroup(bal, 37)
        assert callable(g.pool_stats)
        g.load(st)
        tte, carried, n_checked = scen["tte"], 0, 0

        def check(now):
            nonlocal n_checked
            ref = g.read_state()
            for edges in ((), EDGES15):
                d = diff_summary(g.pool_stats(now, tte, edges), pool_stats_model(ref, now, tte, edges, inflight_counts=False))
                assert not d, (now, len(edges), d)
                n_checked += 1
            return ref

        ref = check(scen["ticks"][0]["now"])
        for t, tk in enumerate(scen["ticks"]):
            seq = np.full(len(tk["ev_kind"]), -1, np.int64)
            for i in np.nonzero(tk["ev_kind"] == synth.EV_RESULT)[0]:
                mine = np.nonzero(ref["log"] == tk["ev_slot"][i])[0]
                if len(mine) and tk["ev_pick"][i] % 5 != 4:
                    seq[i] = mine[tk["ev_pick"][i] % len(mine)]
            n = carried + tk["n_new"]
            out = g.tick(tk["now"], tte, tk["ev_kind"], tk["ev_slot"], tk["ev_val"], tk["ev_ts"], seq, n)
            carried = n + len(out["orphans"]) - len(out["assign"])
            if t == 1:
                # rank 1 fails this summary: rank 0 raises its error, and the group keeps serving
                ref = g.read_state()
                assert not diff_summary(g.pool_stats(tk["now"], tte),
                                        pool_stats_model(ref, tk["now"], tte, (), inflight_counts=False))
                try:
                    g.pool_stats(tk["now"], tte, EDGES15)
                    raise AssertionError("the failing rank's error did not reach rank 0")
                except _lib.FaasbalError as e:
                    assert e.code == _lib.FB_EHIP and "injected" in str(e), e
            ref = check(tk["now"]) if t != 1 else g.read_state()
        assert n_checked == 6 and ref["head"] > len(st["log"])
        g.close()
    except Exception as e:  # report to the parent, keep the peer from hanging
        errq.put("rank %d: %r" % (rank, e))
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_dist_shard_group_stats_over_gloo():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    errq = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_rank, args=(r, 2, port, errq)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
    for p in procs:
        if p.is_alive():
            p.kill()
    errs = []
    while not errq.empty():
        errs.append(errq.get())
    assert not errs, errs
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]


def test_stats_record_round_trip():
    from faasbal.sharded import _PS_REC, _pack_summary, _unpack_summary
    part, qn = pool_stats_part_model(split_state(dict(_states())["shape_w257"], 2, 1), NOW, TTE, EDGES15)
    rec = _pack_summary(part, qn)
    assert rec.dtype == np.int64 and len(rec) == _PS_REC == 3 + C.sizeof(_lib.PoolSummary) // 8
    back, q2 = _unpack_summary(rec)
    assert q2 == qn and not diff_summary(back, part)
    nan, _ = pool_stats_part_model(split_state(dict(_hand_states())["nan_heartbeats"], 3, 0), NOW, TTE)
    back, _ = _unpack_summary(_pack_summary(nan, 3))
    assert np.isnan(back["oldest_hb"]) and np.isnan(back["newest_hb"])


# ------------------------------------------------------------------ 5. the dispatcher
def _dispatcher(rank_cls, world, W, st):
    from faasbal.dispatcher import GpuPushDispatcher
    from faasbal.sharded import LocalShardGroup
    group = LocalShardGroup(world, W, 1 << 16, rank_factory=lambda r: rank_cls(r, world, W))
    io = object()
    d = GpuPushDispatcher("127.0.0.1", 0, TTE, max_workers=W, max_inflight=1 << 16, max_events=64, redis_client=io,
                          subscriber=io, socket=io, poller=io, clock=lambda: NOW, balancer=group)
    group.load(st)
    reads = []
    read_state = group.read_state
    group.read_state = lambda *a, **k: (reads.append(k), read_state(*a, **k))[1]
    return d, reads


def test_dispatcher_takes_the_groups_summary():
    st = _shape_state(257, 2049, 257, np.random.default_rng(77))
    d, reads = _dispatcher(PartRank, 3, 257, st)
    assert callable(d.balancer.pool_stats)
    dev = d.pool_stats()
    assert not reads, reads
    h, hreads = _dispatcher(ModelRankBalancer, 3, 257, st)
    assert h.balancer.pool_stats is None
    host = h.pool_stats()
    assert len(hreads) == 1
    assert dev["inflight_max"] == -1 and host["inflight_max"] >= 0
    d2 = diff_summary(dev, host)
    assert set(d2) == {"inflight_max"}, d2
    for k in ("now", "pending", "inflight_host", "ticks", "compactions", "log_garbage"):
        assert dev[k] == host[k], k
    # the default edges: a quarter, half, three quarters and the whole of time_to_expire
    want = pool_stats_model(st, NOW, TTE, (2.5, 5.0, 7.5, 10.0), inflight_counts=False)
    assert not diff_summary(dev, want) and 0 < want["n_expired"] < want["n_registered"] and want["inflight_expired"] > 0
    assert (want["age_hist"][:5] > 0).all() and not want["age_hist"][5:].any() and MAX_EDGES == 15
