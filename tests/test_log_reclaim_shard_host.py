"""A shard group's reclaim (fb_log_reclaim_shard, ShardGroup.reclaim) without a GPU.

1. The per-rank numpy model (tests/lrs_model.py), merged over the ranks, is
   tests/reclaim_model.reclaim_model on the global state: lists and log.
2. lrs_plan (csrc/faasbal_layout.h), walked on the CPU by tests/lrs_probe.cpp and compared
   with the plan recomputed here.
3. life_gate's Call::log_reclaim_shard (csrc/faasbal_life.h), asked of tests/life_probe.cpp
   over every point of a tick's life, every context kind and a marked compaction (the probe
   runs under the sanitizers in tests/test_life.py); csrc/faasbal_api.hip enters through it;
   the library declares, exports and binds the symbol.
4. ShardGroup.reclaim over model ranks, in process and over gloo (world 2): the model's
   result, a rank that refuses in the count step, a group of ranks without the part.
5. GpuPushDispatcher's deadline and restart scenarios over a group of reclaiming model ranks
   send what they send over the one-table oracle double.
"""
import os
import shutil
import socket
import subprocess

import numpy as np
import pytest

import lcs_model as lm
import lrs_model as lr
from faasbal import _lib
from faasbal._lib import FB_EINVAL, FB_ESTATE, FaasbalError
from faasbal.sharded import shard_range, split_state
from life_cases import KINDS
from reclaim_model import reclaim_model, slots_mask
from shard_model_balancer import ModelRankBalancer
from test_life import _asker, _gate
from test_life import _build as _build_life

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "distributed-faas_amd", "csrc")


# --------------------------------------------------------------------------- 1. the model
def _random_state(rng, W, head):
    reg = (rng.random(W) < 0.7).astype(np.uint8)
    epoch = np.where(rng.random(W) < 0.5, 0, rng.integers(0, head + 2, W)).astype(np.uint32)
    log = rng.integers(0, W, head).astype(np.int32)
    log[rng.random(head) < 0.3] = -1
    q = rng.permutation(np.flatnonzero(reg)).astype(np.int32)
    return dict(reg=reg, free=rng.integers(0, 4, W).astype(np.int32), hb=rng.random(W) + 1000.0, epoch=epoch,
                queue=q[: len(q) // 2], log=log)


def check_group_model(st, world, below, slots, what):
    """The ranks' models merged against reclaim_model on the global state; returns the lists."""
    W = len(st["reg"])
    want, seq, slot, _ = reclaim_model(st, below, None if slots is None else slots_mask(W, slots))
    shards = [split_state(st, world, r) for r in range(world)]
    outs, gseq, gslot = lr.group_reclaim_model(shards, below, slots)
    assert gseq.tolist() == seq.tolist() and gslot.tolist() == slot.tolist(), what
    assert gseq.dtype == np.int64 and gslot.dtype == np.int32, what
    log = np.asarray(st["log"], np.int32).copy()
    for r, (o, pre) in enumerate(zip(outs, shards)):
        for k in pre:  # nothing but log_slot changes, and the input is left alone
            if k != "log_slot":
                assert o[k] is pre[k], (what, r, k)
        taken = np.asarray(o["log_slot"]) != np.asarray(pre["log_slot"])
        assert (np.asarray(o["log_slot"])[taken] == -1).all(), (what, r)
        log[np.asarray(pre["log_seq"], np.int64)] = o["log_slot"]
    # (entries of slots without a record or older than their registration stay as they were)
    assert log.tolist() == want["log"].tolist(), what
    return seq


@pytest.mark.parametrize("world", (1, 2, 3, 4))
def test_ranks_merged_are_the_global_model(world):
    rng = np.random.default_rng(8100 + world)
    taken = 0
    for W, head in ((5, 300), (37, 0), (37, 1), (41, 2049), (300, 700)):
        st = _random_state(rng, W, head)
        for below in (None, 0, 1, head // 2, head, head + 7):
            for slots in (None, [], [W // 2], np.flatnonzero(rng.random(W) < 0.5).tolist()):
                taken += len(check_group_model(st, world, below, slots, "W %d head %d below %s slots %s"
                                               % (W, head, below, slots)))
    assert taken > 0
    with pytest.raises(ValueError):
        lr.reclaim_part_model(split_state(st, world, 0), -1)


def test_model_special_cases():
    rng = np.random.default_rng(8200)
    # a rank that owns no slot: W = 5 over 4 ranks is 2 + 2 + 1 + 0
    assert [shard_range(5, 4, r)[1] for r in range(4)] == [2, 2, 1, 0]
    st = _random_state(rng, 5, 500)
    assert len(check_group_model(st, 4, None, None, "zero-slot rank")) > 0
    assert lr.reclaim_part_model(split_state(st, 4, 3), None, lr.local_mask(split_state(st, 4, 3), [4]))[1].tolist() == []
    # a rank with an empty shard
    st = _random_state(rng, 40, 300)
    st["log"] = np.where(st["log"] >= 0, st["log"] % 10, -1).astype(np.int32)
    assert len(check_group_model(st, 4, 200, None, "empty shards")) > 0
    assert all(len(split_state(st, 4, r)["log_slot"]) == 0 for r in (1, 2, 3))
    # a rank's prefix is not the bound: the sequences are interleaved across the ranks
    st = dict(reg=np.ones(4, np.uint8), free=np.ones(4, np.int32), hb=np.zeros(4), epoch=np.zeros(4, np.uint32),
              queue=np.zeros(0, np.int32), log=np.asarray([0, 2, 1, 3, 0, 2, 1, 3], np.int32))
    outs, seq, slot = lr.group_reclaim_model([split_state(st, 2, r) for r in range(2)], 5)
    assert seq.tolist() == [0, 1, 2, 3, 4] and slot.tolist() == [0, 2, 1, 3, 0]
    assert outs[0]["log_slot"].tolist() == [-1, -1, -1, 1] and outs[1]["log_slot"].tolist() == [-1, -1, 2, 3]
    # the mask is the rank's own bytes: global slots of other ranks name nothing here
    rs = split_state(st, 2, 1)
    assert lr.local_mask(rs, [0, 1, 3]).tolist() == [0, 1] and lr.local_mask(rs, None) is None


# --------------------------------------------------------------------------- 2. the plan
def _build(tmp, src, name, extra=()):
    if shutil.which("hipcc") is None:
        pytest.fail("hipcc not found: %s cannot be compiled" % src)
    exe = str(tmp / name)
    subprocess.run(["hipcc", "-std=c++17", "-O1", *extra, "-I" + CSRC, "-I" + os.path.join(REPO, "include"),
                    os.path.join(HERE, src), "-o", exe], check=True)
    return exe


SEAMS = (0, 1, 63, 64, 65, 2047, 2048, 2049, 3 * 2048 + 5)


def _r256(b):
    return (b + 255) & ~255


def test_plan_is_the_one_recomputed_here(tmp_path):
    exe = _build(tmp_path, "lrs_probe.cpp", "lrs_probe")
    cases = [(hl, W) for hl in SEAMS for W in (0, 1, 300)]
    cases.append((1 << 23, 1 << 17))
    text = "".join("%d %d\n" % c for c in cases)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
    rows = [{k: int(v) for k, v in (kv.split("=") for kv in line.split())} for line in out.splitlines()]
    assert len(rows) == len(cases)
    for (hl, W), r in zip(cases, rows):
        what = "head_local %d W %d" % (hl, W)
        nt = -(-hl // 2048)
        assert (r["tile"], r["words_per_tile"]) == (2048, 32), what
        assert (r["lists"], r["nt"], r["nw"]) == (hl, nt, 32 * nt), what
        assert r["flag_grid"] == r["take_grid"] == -(-nt // 4) and r["scan_grid"] == 1, what
        # the grids cover the local tiles once; the regions do not overlap
        assert r["flag.cover"] == r["take.cover"] == r["words.cover"] == r["regions.ok"] == 1, what
        # the scratch recomputed: the table, the W mask bytes, the two lists at head_local entries each
        at, o = {}, 0
        for key, nbytes in (("bitmap", 8 * 32 * nt), ("wrel", 4 * 32 * nt), ("tcnt", 4 * nt), ("tpre", 4 * (nt + 1)),
                            ("mask", W), ("seq", 8 * hl), ("slot", 4 * hl)):
            at[key] = o
            o += _r256(nbytes)
        assert {k: r[k] for k in at} == at and r["bytes"] == o, what


# --------------------------------------------------------------------------- 3. the gate
IN_TICK = ("phase1", "launched", "waited", "failed")
MARKED = "a log compaction is marked: apply or cancel first"


POS = ("none", "phase1", "launched", "waited", "failed", "dropped")


def test_gate_refusals_and_duties(tmp_path):
    """Every Pos x staged x kind x cm_pending x undo_E (0, 3) x marked, table states or not, with
    fb_pool_stats_shard's gate at the same point beside it (ps_*).  (That the gate never makes
    a transition needs no row: life_gate takes a const Life &.)"""
    ask = _asker(_build_life(tmp_path, "life_probe"))
    rows = [dict(kind=k, staged=st, pos=pos, cm=cm, undo_E=ue, marked=m) for k in KINDS for st in "01" for pos in POS
            for cm in "01" for ue in "03" for m in "01"]
    at = ["%(kind)s %(staged)s,%(pos)s,0,0,0,%(cm)s,%(undo_E)s,0,%(marked)s" % r for r in rows]
    for r, mine, ps in zip(rows, ask(["gate %s log_reclaim_shard" % x for x in at]),
                           ask(["gate %s pool_stats_shard" % x for x in at])):
        refuse, duties, _ = _gate(mine)
        ps_refuse, ps_duties, _ = _gate(ps)
        r.update(refuse=refuse, duties=",".join(duties) or "-", ps_duties=",".join(ps_duties) or "-",
                 ps_refused=str(int(ps_refuse is not None)))
    assert len(rows) == 4 * 2 * 6 * 2 * 2 * 2
    assert len({(r["kind"], r["staged"], r["pos"], r["cm"], r["undo_E"], r["marked"]) for r in rows}) == len(rows)
    seen = set()
    for r in rows:
        what = str(r)
        duties = set() if r["duties"] == "-" else set(r["duties"].split(","))
        # refused exactly where fb_pool_stats_shard is, with the same duties
        assert (r["refuse"] is not None) == (r["ps_refused"] == "1"), what
        assert r["duties"] == r["ps_duties"], what
        if r["kind"] != "shard":  # one-GPU and deque kinds
            assert r["refuse"] == "fb_log_reclaim_shard on a one-GPU context: use fb_log_reclaim", what
            assert duties == ({"flush"} if r["cm"] == "1" else set()), what
        elif r["marked"] == "1":
            assert r["refuse"] == MARKED and duties == set(), what
        elif r["staged"] == "1" or r["pos"] in IN_TICK:
            # under its own name
            assert r["refuse"].startswith("fb_log_reclaim_shard ") and "fb_pool_stats" not in r["refuse"], what
            assert duties <= {"flush"}, what
            word = "staged" if r["staged"] == "1" else "wait and its commit" if r["pos"] == "waited" else "launched"
            assert word in r["refuse"], what
        else:  # between ticks (none; dropped: a launch the wait dropped, its in-place clears owed)
            assert r["refuse"] is None, what
            want = set()
            if r["cm"] == "1":
                want.add("flush")
            if r["pos"] == "dropped" and r["undo_E"] != "0":
                want.add("undo")  # taken back first: the entries its results named count as live
            assert duties == want, what
            seen.add((r["pos"], tuple(sorted(duties))))
    assert ("dropped", ("undo",)) in seen and ("dropped", ("flush", "undo")) in seen and ("none", ()) in seen


def test_api_enters_through_the_gate_and_the_binding_knows_the_symbol():
    api = open(os.path.join(CSRC, "faasbal_api.hip")).read()
    wrapper = api[api.index("int fb_log_reclaim_shard(fb_ctx *c"):]
    assert "return log_reclaim_run(c, true, " in wrapper[:wrapper.index("\n}\n")]
    body = api[api.index("static int log_reclaim_run(fb_ctx *c, bool shard"):]
    body = body[:body.index("\n}\n")]
    assert "enter(c, shard ? Call::log_reclaim_shard : Call::log_reclaim)" in body
    # ... ahead of every launch and every write; the count check before the take
    assert body.index("enter(c, ") < body.index("launch_lr_flag") < body.index("launch_lc_scan") \
        < body.index("cap < (int64_t)n") < body.index("launch_lr_take")
    assert "lrs_plan(c->head_local, c->W)" in body and "lr_plan(c->head, below_seq, c->W)" in body
    assert "hipMemcpy" not in body[:body.index("enter(c, ")]
    # the one-GPU call keeps refusing sharded contexts, and says where to go
    life = open(os.path.join(CSRC, "faasbal_life.h")).read()
    assert "use fb_log_reclaim_shard" in life and life.count('"%s"' % MARKED) == 1
    header = open(os.path.join(REPO, "include", "faasbal.h")).read()
    assert "int fb_log_reclaim_shard(fb_ctx *ctx, int64_t below_seq, const uint8_t *slot_mask" in header
    assert "fb_log_reclaim_shard" in _lib.EXPORTS
    assert callable(_lib.load().fb_log_reclaim_shard)
    from faasbal.sharded import ShardedBalancer, ShardGroup
    assert callable(ShardedBalancer.reclaim_part) and ShardedBalancer.reclaim is None and callable(ShardGroup.reclaim)


# --------------------------------------------------------------------------- 4. the group over model ranks
def _group(world, W, rank_cls=lr.ReclaimRank):
    return lm.ModelGroup(world, W, rank_cls)


def _loaded(g, seed, W, head):
    """A loaded group and the state as the ranks hold it (dead entries dropped at the load)."""
    g.load(_random_state(np.random.default_rng(seed), W, head))
    return g.read_state()


def check_group_reclaim(g, ranks_read, world, below, slots, what):
    """ShardGroup.reclaim against reclaim_model of the merged state read before it, on the
    group's lists and on every rank's shard; returns the result."""
    pre, ranks_pre = g.read_state(), ranks_read()
    W = len(pre["reg"])
    want, seq, slot, _ = reclaim_model(pre, below, None if slots is None else slots_mask(W, slots))
    out = g.reclaim(below, slots)
    assert out["n"] == len(seq), what
    np.testing.assert_array_equal(out["seq"], seq, err_msg=what + ": seq")
    np.testing.assert_array_equal(out["slot"], slot, err_msg=what + ": slot")
    assert out["seq"].dtype == np.int64 and out["slot"].dtype == np.int32, what
    post = g.read_state()
    np.testing.assert_array_equal(post["log"], want["log"], err_msg=what + ": log")
    assert post["head"] == pre["head"], what
    for k in ("reg", "free", "hb", "epoch", "queue"):
        np.testing.assert_array_equal(post[k], pre[k], err_msg=what + ": " + k)
    for r, (rs, p) in enumerate(zip(ranks_read(), ranks_pre)):
        w = split_state(want, world, r)
        # (the shard keeps its length and its sequences: the taken entries stay in place, at -1)
        np.testing.assert_array_equal(rs["log_seq"], p["log_seq"], err_msg="%s: rank %d log_seq" % (what, r))
        for k in ("reg", "free", "hb", "epoch", "queue"):
            np.testing.assert_array_equal(rs[k], p[k], err_msg="%s: rank %d %s" % (what, r, k))
        assert rs["head"] == p["head"] and len(rs["log"]) == len(p["log"]), (what, r)
        got = np.full(pre["head"], -1, np.int32)
        got[np.asarray(rs["log_seq"], np.int64)] = rs["log"]
        own = (want["log"] >= w["base"]) & (want["log"] < w["base"] + w["n"])
        np.testing.assert_array_equal(got[own], want["log"][own], err_msg="%s: rank %d log" % (what, r))
        assert (got[~own] == -1).all(), (what, r)
    return out


@pytest.mark.parametrize("world", (1, 2, 3))
def test_local_group_reclaims_as_the_model(world):
    W = 37
    g = _group(world, W)
    assert callable(g.reclaim)
    pre = _loaded(g, 8300, W, 600)
    taken = 0
    for below, slots in ((200, None), (None, [3, 20, 36]), (450, np.flatnonzero(np.arange(W) % 2 == 0)), (0, None),
                         (None, []), (None, None)):
        taken += check_group_reclaim(g, lambda: [b.read_state() for b in g.bals], world, below, slots,
                                     "world %d below %s" % (world, below))["n"]
    assert taken == int((pre["log"] >= 0).sum()) > 100
    with pytest.raises(ValueError):
        g.reclaim(slots=[W])
    with pytest.raises(ValueError):
        g.reclaim(slots=[-1])
    with pytest.raises(FaasbalError) as e:
        g.reclaim(below_seq=-1)
    assert e.value.code == FB_EINVAL


@pytest.mark.parametrize("world", (2, 3))
def test_a_rank_that_refuses_leaves_every_shard_as_it_was(world):
    W = 37
    g = _group(world, W)
    _loaded(g, 8301, W, 400)
    before = [b.read_state() for b in g.bals]
    g.bals[-1].refuse_count = True
    with pytest.raises(FaasbalError) as e:
        g.reclaim(300)
    assert e.value.code == FB_ESTATE and "injected" in str(e.value)
    for b, pre in zip(g.bals, before):
        now = b.read_state()
        assert all(np.array_equal(now[k], pre[k]) for k in pre if k != "base"), b.rank
        assert all(c[2] for c in b.reclaim_calls), "no rank took anything"
    # the next call works
    assert check_group_reclaim(g, lambda: [b.read_state() for b in g.bals], world, 300, None, "after a refusal")["n"] > 0


def test_group_of_old_doubles_has_no_reclaim():
    g = _group(2, 8, ModelRankBalancer)
    assert g.reclaim is None
    g = _group(2, 8, lm.CompactRank)  # (the parts of a compaction, no part of a reclaim)
    assert g.reclaim is None and callable(g.compact_log)
    from faasbal.dispatcher import GpuPushDispatcher
    from test_dispatcher import FakeEnv, wid
    env = FakeEnv()
    args = dict(redis_client=env, subscriber=env, socket=env, poller=env, clock=env.clock, max_workers=8, max_events=8,
                max_inflight=64)
    with pytest.raises(FaasbalError) as e:
        GpuPushDispatcher("127.0.0.1", 0, 10, balancer=_group(2, 8, ModelRankBalancer), task_timeout=1.0, **args)
    assert e.value.code == FB_ESTATE and "reclaim_part" in str(e.value)
    d = GpuPushDispatcher("127.0.0.1", 0, 10, balancer=_group(2, 8, ModelRankBalancer), **args)
    with pytest.raises(FaasbalError) as e:
        d.reclaim([wid(0)])
    assert e.value.code == FB_ESTATE and "reclaim_part" in str(e.value)


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
        W = 37
        bal = lr.ReclaimRank(rank, world, W)
        if rank != 0:
            # this rank's third count step refuses
            part = bal.reclaim_part

            def counted(below_seq=None, slots=None, count_only=False):
                if count_only:
                    bal.refuse_count = sum(1 for c in bal.reclaim_calls if c[2]) == 2
                return part(below_seq, slots, count_only)
            bal.reclaim_part = counted
            serve_shard(bal)  # (it keeps serving after the refused reclaim)
            assert [c[2] for c in bal.reclaim_calls] == [True, False, True, False, True, True, False, True, False], \
                bal.reclaim_calls
            return
        g = DistShardGroup(bal, W)
        assert callable(g.reclaim)
        g.load(_random_state(np.random.default_rng(8302), W, 700))
        shards = lambda: g._each("read", with_log=True)  # noqa: E731 -- every rank's shard, through the group
        # 1, 2: the model's result, with a bound, then with a mask (the slots travel as a tensor)
        n1 = check_group_reclaim(g, shards, world, 300, None, "gloo, a bound")["n"]
        n2 = check_group_reclaim(g, shards, world, None, [1, 5, 20, 30, 36], "gloo, a mask")["n"]
        assert n1 > 0 and n2 > 0
        # 3: rank 1 refuses in the count step: rank 0 raises the code, every shard is as it was
        before = g.read_state()
        try:
            g.reclaim(600)
            raise AssertionError("the refusing rank's error did not reach rank 0")
        except FaasbalError as e:
            assert e.code == FB_ESTATE and "injected" in str(e), e
        after = g.read_state()
        assert all(np.array_equal(after[k], before[k]) for k in ("reg", "free", "hb", "epoch", "queue", "log"))
        assert all(c[2] for c in bal.reclaim_calls[4:]), "rank 0 took nothing"
        # 4: the next call still works; 5: an empty result (only rank 0 has anything: no gather)
        assert check_group_reclaim(g, shards, world, 600, None, "gloo, after a refusal")["n"] > 0
        assert check_group_reclaim(g, shards, world, 600, None, "gloo, nothing left")["n"] == 0
        g.close()
    except Exception as e:  # report to the parent, keep the peer from hanging
        errq.put("rank %d: %r" % (rank, e))
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_dist_shard_group_reclaims_over_gloo():
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


# --------------------------------------------------------------------------- 5. the dispatcher
def _scripted(make):
    """The deadline and restart scenarios of tests/test_reclaim_dispatcher.py as one script;
    returns, per step, the task messages sent, the Redis writes and the host's counters."""
    from test_dispatcher import FakeEnv, wid
    from test_reclaim_dispatcher import _beats, _make, _msg, _result, _tick
    trace = []

    def step(d, env, *a, **k):
        env.hsets.clear()
        sent = _tick(d, env, *a, **k)
        trace.append((sent, list(env.hsets), d.reclaimed, d.timed_out_failed, dict(d.attempts), sorted(d.task_seq.items()),
                      list(d.pending)))
        return sent

    reg = lambda w, n=1: (wid(w), _msg("register", {"num_processes": n}))  # noqa: E731
    # a hung task goes to another worker at the deadline, not before; late and own results
    env = FakeEnv()
    d = _make(make, env, task_timeout=5.0)
    assert step(d, env, 1000.0, [reg(0)], ["hang"]) == [(wid(0), "hang")]
    step(d, env, 1002.0, _beats([0], reg(1)))
    assert step(d, env, 1004.9, _beats([0, 1])) == [] and d.reclaimed == 0
    assert step(d, env, 1005.0, _beats([0, 1])) == [(wid(1), "hang")] and d.reclaimed == 1
    assert step(d, env, 1006.0, _beats([1], (wid(0), _result("hang"))), ["next"]) == [(wid(0), "next")]
    step(d, env, 1007.0, _beats([0], (wid(1), _result("hang"))))
    assert "hang" not in d.task_seq
    dispatchers = [d]
    # max_attempts ends in FAILED
    env = FakeEnv()
    d = _make(make, env, task_timeout=5.0, max_attempts=2)
    step(d, env, 1000.0, [reg(0)], ["doom"])
    step(d, env, 1001.0, _beats([0], reg(1)))
    assert step(d, env, 1005.0, _beats([0, 1])) == [(wid(1), "doom")]
    step(d, env, 1009.0, _beats([0, 1]))
    step(d, env, 1010.0, _beats([0, 1]))
    assert [(t, m["status"]) for t, m in trace[-1][1]] == [("doom", "FAILED")]
    assert d.reclaimed == 2 and d.timed_out_failed == 1
    step(d, env, 1020.0, _beats([0, 1]))
    dispatchers.append(d)
    # a worker restarted under its identity: reclaim() by identity, a mask of one slot
    env = FakeEnv()
    d = _make(make, env)
    sent = step(d, env, 1000.0, [reg(0, 2), reg(1, 2)], ["a", "b", "c", "d"])
    on0 = [t for dst, t in sent if dst == wid(0)]
    step(d, env, 1001.0, [reg(0, 2)])
    back = d.reclaim([wid(0), b"nobody"])
    assert back == on0 and list(d.pending) == on0
    trace.append(("reclaim", back))
    assert step(d, env, 1002.0, _beats([0, 1])) == [(wid(0), t) for t in on0]
    assert d.reclaim([b"nobody"]) == []
    dispatchers.append(d)
    return trace, dispatchers


@pytest.mark.parametrize("world", (2, 3))
def test_dispatcher_deadlines_over_a_group_of_model_ranks(world, monkeypatch):
    import faasbal.dispatcher as D
    from test_reclaim_dispatcher import ReclaimingOracleBalancer
    monkeypatch.setattr(D, "GpuBalancer", ReclaimingOracleBalancer)
    one, d1 = _scripted(D.GpuPushDispatcher)

    def over_group(*a, **kw):
        return D.GpuPushDispatcher(*a, balancer=_group(world, kw["max_workers"]), **kw)
    grp, dn = _scripted(over_group)
    assert grp == one and len(one) > 12
    # the same reclaims reached the device: every rank counted, then every rank took
    for a, b in zip(d1, dn):
        want = a.balancer.reclaim_calls
        for r in b.balancer.bals:
            assert [c[:2] for c in r.reclaim_calls if not c[2]] == [(1 << 62 if q is None else q, s) for q, s in want]
            assert [c[2] for c in r.reclaim_calls] == [True, False] * len(want)
        # the group's merged log is the dispatcher's in-flight table
        log = b.balancer.read_state()["log"]
        assert b.head == len(log) and all(log[q] == s for q, (_, s) in b.inflight.items())
        assert int((log >= 0).sum()) == len(b.inflight)
