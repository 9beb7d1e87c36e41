"""The group layer's wire format and its two transports, characterised (faasbal/sharded.py).

One script of thirteen group calls -- every operation, with and without its optional payload,
accepted and refused -- runs

1. on a DistShardGroup over gloo (world 2) with six torch.distributed functions wrapped, so
   that every collective is recorded as name, dtype and element count: both ranks' sequences
   are tests/group_wire_trace.py's table, recorded once from this project's own output and
   kept as a literal (it is not derived from the code under test);
2. on an in-process group of the same rank doubles: every returned value, every raised error
   and every rank's state after every step are the distributed run's -- the two transports
   carry one protocol.

Then the structure the group layer keeps: one function per protocol, one guard, one header
gather, the operations as keys of one table.
"""
import copy
import inspect
import os
import re
import socket

import numpy as np
import pytest

import lcs_model as lm
import lrs_model as lr
from faasbal import synth
from faasbal._lib import FaasbalError
from faasbal.poolstats import pool_stats_part_model
from group_wire_trace import STEPS, TRACE

W, WORLD = 37, 2
WIRE = ("broadcast", "all_gather", "all_reduce", "gather", "all_gather_object", "broadcast_object_list")
PREFIX = "failed on a rank: "


class FullRank(lr.ReclaimRank):
    """TEST DOUBLE: the model rank with every part (a compaction's, a reclaim's, the summary's)."""

    def pool_stats_part(self, now, tte, age_edges=()):
        return pool_stats_part_model(self.read_state(), now, tte, age_edges)


def scenario():
    scen = synth.random_scenario(7301, W=W, n_ticks=3, max_events=20, max_new=50)
    st = dict(reg=scen["init_reg"], free=scen["init_free"], hb=scen["init_hb"], epoch=scen["init_epoch"],
              queue=scen["init_queue"], log=scen["init_log"])
    return scen, st


def _attempt(f, *a, **k):
    try:
        return ("ok", f(*a, **k))
    except (FaasbalError, RuntimeError) as e:
        return ("error", getattr(e, "code", None), str(e).split(PREFIX, 1)[-1])


def run_script(g, after_step):
    """The thirteen steps on a group, ``after_step(name)`` called after each; returns the
    list of (name, ("ok", value) | ("error", code, text after the prefix))."""
    scen, st = scenario()
    tte, tk = scen["tte"], scen["ticks"][0]
    out = []

    def step(name, f, *a, **k):
        out.append((name, _attempt(f, *a, **k)))
        after_step(name)
        return out[-1][1][1]

    step("load", g.load, st)
    ref = step("read", g.read_state)
    seq = np.full(len(tk["ev_kind"]), -1, np.int64)
    for i in np.nonzero(tk["ev_kind"] == synth.EV_RESULT)[0]:
        mine = np.nonzero(ref["log"] == tk["ev_slot"][i])[0]
        if len(mine) and tk["ev_pick"][i] % 5 != 4:
            seq[i] = mine[tk["ev_pick"][i] % len(mine)]
    step("tick", g.tick, tk["now"], tte, tk["ev_kind"], tk["ev_slot"], tk["ev_val"], tk["ev_ts"], seq, tk["n_new"])
    step("tick_no_events", g.tick, tk["now"] + 1.0, tte, n_pending=5)
    step("purge", g.purge, tk["now"] + 1.0, tte)
    step("stats", g.pool_stats, tk["now"] + 1.0, tte)
    step("stats_two_edges", g.pool_stats, tk["now"] + 1.0, tte, (1.0, 5.0))
    kept = step("compact", g.compact_log)
    step("compact_wrong_expect", g.compact_log, expect=kept["n_kept"] + 1)
    step("reclaim_all", g.reclaim)
    step("reclaim_slots", g.reclaim, slots=[1, 30])
    step("reclaim_refused", g.reclaim, below_seq=-1)
    step("close", g.close)
    assert tuple(n for n, _ in out) == STEPS
    return out


# --------------------------------------------------------------------------- the distributed run
def _describe(name, a):
    shape = lambda t: "%s[%d]" % (str(t.dtype).replace("torch.", ""), t.numel())  # noqa: E731
    if name in ("broadcast", "all_reduce", "gather"):
        return "%s %s" % (name, shape(a[0]))
    if name == "all_gather":
        return "%s %d x %s" % (name, len(a[0]), shape(a[1]))
    return name


def _wrap(dist, seen):
    for name in WIRE:
        def wrapped(*a, _name=name, _real=getattr(dist, name), **k):
            seen(_describe(_name, a))
            return _real(*a, **k)
        setattr(dist, name, wrapped)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _gloo_rank(rank, world, port, errq, resq):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    from faasbal.sharded import DistShardGroup, serve_shard
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        bal = FullRank(rank, world, W)
        trace, states = [], []  # per step: the collectives; this rank's state after it
        if rank == 0:
            g = DistShardGroup(bal, W)
            trace.append([])
            _wrap(dist, lambda what: trace[-1].append(what))

            def after_step(name):
                states.append(copy.deepcopy(bal.read_state()))
                trace.append([])
            results = run_script(g, after_step)
            trace.pop()
        else:
            # a call begins with its header, the one int64[8] that is broadcast: what this rank
            # holds then is its state after the step before
            def seen(what):
                if what == "broadcast int64[8]":
                    if trace:
                        states.append(copy.deepcopy(bal.read_state()))
                    trace.append([])
                trace[-1].append(what)
            _wrap(dist, seen)
            serve_shard(bal)
            states.append(copy.deepcopy(bal.read_state()))
            results = None
        resq.put((rank, trace, states, results))
    except Exception as e:  # report to the parent, keep the peer from hanging
        errq.put("rank %d: %r" % (rank, e))
        raise
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def dist_run():
    """{rank: (trace per step, state after each step, results or None)} of the script over gloo."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    errq, resq = ctx.Queue(), ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_rank, args=(r, WORLD, port, errq, resq)) for r in range(WORLD)]
    for p in procs:
        p.start()
    got = {}
    try:
        for _ in procs:
            r = resq.get(timeout=240)
            got[r[0]] = r[1:]
    except Exception:  # noqa: BLE001 -- a rank died: its report is in errq
        pass
    for p in procs:
        p.join(60)
    for p in procs:
        if p.is_alive():
            p.kill()
    errs = []
    while not errq.empty():
        errs.append(errq.get())
    assert not errs, errs
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    return got


@pytest.mark.timeout(300)
def test_wire_trace_is_the_recorded_one(dist_run):
    for rank in range(WORLD):
        trace = dist_run[rank][0]
        assert len(trace) == len(STEPS)
        for name, got in zip(STEPS, trace):
            assert got == list(TRACE[name]), (rank, name, got)
    assert dist_run[1][0] == dist_run[0][0]
    assert sum(len(t) for t in dist_run[0][0]) == 41


# --------------------------------------------------------------------------- the two transports
def same_value(a, b, what):
    if isinstance(a, dict):
        assert isinstance(b, dict) and sorted(a) == sorted(b), what
        for k in a:
            same_value(a[k], b[k], "%s[%r]" % (what, k))
    elif isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        np.testing.assert_array_equal(a, b, err_msg=what)
        assert np.asarray(a).dtype == np.asarray(b).dtype, what
    else:
        assert a == b or (a != a and b != b), (what, a, b)


def model_run():
    """The script on an in-process group of the doubles: (results, per step every rank's state)."""
    g = lm.ModelGroup(WORLD, W, FullRank)
    states = []
    results = run_script(g, lambda name: states.append([copy.deepcopy(b.read_state()) for b in g.bals]))
    return results, states


@pytest.mark.timeout(300)
def test_local_and_distributed_carry_one_protocol(dist_run):
    results, states = model_run()
    want = dist_run[0][2]
    assert [n for n, _ in results] == [n for n, _ in want] == list(STEPS)
    for (name, got), (_, exp) in zip(results, want):
        assert got[0] == exp[0], (name, got, exp)
        if got[0] == "error":
            assert got[1:] == exp[1:], name
        else:
            same_value(got[1], exp[1], name)
    refused = {n: r for n, r in results if r[0] == "error"}
    assert sorted(refused) == ["compact_wrong_expect", "reclaim_refused"]
    for i, name in enumerate(STEPS):
        for rank in range(WORLD):
            same_value(states[i][rank], dist_run[rank][1][i], "%s: rank %d's state" % (name, rank))


# --------------------------------------------------------------------------- the structure
def test_each_protocol_is_stated_once():
    import faasbal.sharded as S
    src = inspect.getsource(S)
    layer = src[src.index("class ShardGroup"):]  # the groups, the protocols, the wire format, the transports
    # one function holds each protocol: the ranks' parts are called there and nowhere else
    for fn, calls in ((S._compact, ("b.compact_mark", "b.compact_exchange", "b.compact_apply", "b.compact_cancel")),
                      (S._reclaim, ("b.reclaim_part",)), (S._tick, ("b.commit()",)),
                      (S.run_phases, ("launch(b)", "b.cont()", "b.wait()"))):
        for call in calls:
            assert inspect.getsource(fn).count(call) == src.count(call) >= 1, (fn.__name__, call)
    assert inspect.getsource(S._reclaim).count("b.reclaim_part") == 2  # the count, then the take
    # the groups differ in their transport and in who holds which ranks
    # (and in _collective_once, the seam LocalShardGroup keeps for rank doubles: it holds no step of its own)
    assert set(vars(S.DistShardGroup)) <= {"__module__", "__doc__", "__init__", "close"}, vars(S.DistShardGroup).keys()
    assert set(vars(S.LocalShardGroup)) <= {"__module__", "__doc__", "__init__", "close", "_each", "_collective_once"}
    for m in ("_each", "_collective_once"):
        assert "super()._each(op, **kw)" in inspect.getsource(getattr(S.LocalShardGroup, m))
    assert {m for m in vars(S.InProcess) if not m.startswith("_")} == {m for m in vars(S.Distributed) if not m.startswith("_")} \
        == {"announce", "agree", "reduce", "collect", "phases"}
    # the operations are the keys of one table (serve_shard's loop ends at "stop"): no ladders
    assert sorted(S._OPS) == ["compact", "load", "purge", "read", "reclaim", "stats", "stop", "tick"]
    assert sorted(spec.code for spec in S._OPS.values()) == list(range(1, 9))
    assert re.findall(r"\bop (?:==|!=|in|not in) \S+", src) == ['op == "stop":']
    for op in S._OPS:  # named as a key and by its ShardGroup method ("stop": the key, close() and serve_shard)
        assert len(re.findall(r'"%s"' % op, layer)) == (3 if op == "stop" else 1 + len(re.findall(r'_each\("%s"' % op, layer))), op
    # one guard, one header gather, one gather of lists; the pickled forms: whole values, messages
    assert src.count("except Exception") == 1 and "except Exception" in inspect.getsource(S._guarded)
    assert src.count(".all_gather(") == 1 and src.count(".gather(") == 1 and src.count(".all_gather_object(") == 2
    assert src.count(".broadcast(") == 4 and src.count(".broadcast_object_list(") == 2  # a sender's and a receiver's each
    # the exchange's size is asked once per launch, and no group reaches into a rank
    assert src.count("fb_exchange_bytes") == 2 and "fb_exchange_bytes" in inspect.getsource(S.ShardedBalancer._launched)
    assert not re.search(r"\._E\b|\._chk\b|\.lib\.|\._xbytes\b|\.h\b", layer)
    # shorter than what it replaced, and the doubles' group no longer than it was
    assert len(src.splitlines()) < 1055
    assert len(inspect.getsource(lm).splitlines()) <= 162


def test_collective_once_is_a_seam_for_rank_doubles():
    """A group may put its own tick in LocalShardGroup._collective_once (serve_op per rank,
    committed): world 1, where the exchange has one contributor, gives the model group's tick."""
    from faasbal.sharded import LocalShardGroup, serve_op

    class OwnTick(LocalShardGroup):
        def _collective_once(self, op, kw):
            return [serve_op(b, op, kw, allreduce=lambda x: None) for b in self.bals]

    scen, st = scenario()
    groups = [OwnTick(1, W, 0, rank_factory=lambda r: FullRank(r, 1, W)), lm.ModelGroup(1, W, FullRank)]
    outs = []
    for g in groups:
        g.load(st)
        outs.append([g.tick(scen["ticks"][0]["now"], scen["tte"], n_pending=7), g.purge(scen["ticks"][0]["now"] + 1.0, scen["tte"]),
                     g.read_state()])
    assert len(outs[0][0]["assign"]) > 0
    for a, b in zip(outs[0], outs[1]):
        same_value(a, b, "own tick")
