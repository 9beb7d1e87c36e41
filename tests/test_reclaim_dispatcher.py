"""Task deadlines and restarted workers in GpuPushDispatcher, without a GPU.

The balancer is the oracle double (tests/oracle_balancer.py) with a ``reclaim`` that goes
oracle export -> the numpy model of fb_log_reclaim's rule (tests/reclaim_model.py) -> oracle
load; sockets, pub/sub, Redis and the clock are tests/test_dispatcher.py's fakes.
"""
import numpy as np
import pytest

from faasbal import codec
from faasbal._lib import FB_ESTATE, FaasbalError
from oracle_balancer import OracleBalancer
from reclaim_model import reclaim_model, slots_mask
from test_dispatcher import GOLDEN, FakeEnv, replay_golden, wid


class ReclaimingOracleBalancer(OracleBalancer):
    """The oracle double with fb_log_reclaim's rule applied to its own state."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.reclaim_calls = []

    def reclaim(self, below_seq=None, slots=None):
        st = self.o.export()
        mask = None if slots is None else slots_mask(len(st["reg"]), slots)
        self.reclaim_calls.append((below_seq, None if slots is None else sorted(int(s) for s in slots)))
        new, seq, slot, _ = reclaim_model(st, below_seq, mask)
        self.o.load(new["reg"], new["free"], new["hb"], new["epoch"], new["queue"], new["log"])
        return {"n": len(seq), "seq": seq, "slot": slot}

    def compact_log(self, expect=None, want_kept=True):
        from lc_model import compact_model
        st, kept = compact_model(self.o.export())
        if expect is not None and int(expect) != len(kept):
            raise FaasbalError(FB_ESTATE, "the log holds %d live entries, the caller expected %d" % (len(kept), expect))
        self.o.load(st["reg"], st["free"], st["hb"], st["epoch"], st["queue"], st["log"])
        return {"n_kept": len(kept), "kept": kept if want_kept else None}


@pytest.fixture
def dispatcher_cls(monkeypatch):
    import faasbal.dispatcher as D
    monkeypatch.setattr(D, "GpuBalancer", ReclaimingOracleBalancer)
    return D.GpuPushDispatcher


def _msg(typ, data=None):
    m = {"type": typ}
    if data is not None:
        m["data"] = data
    return codec.serialize(m).encode()


def _result(tid):
    return _msg("result", {"task_id": tid, "status": "COMPLETED", "result": 1})


def _make(cls, env, **kw):
    return cls("127.0.0.1", 0, 10, redis_client=env, subscriber=env, socket=env, poller=env, clock=env.clock,
               max_workers=8, max_events=64, max_inflight=kw.pop("max_inflight", 1 << 12), **kw)


def _tick(d, env, now, inbound=(), tasks=()):
    """One tick at clock ``now``; returns the task messages it sent as (identity, task id)."""
    env.now = now
    for w, frame in inbound:
        env.inbound.append((w, frame, now))
    env.tasks.extend(tasks)
    env.sent.clear()
    d.tick()
    return [(dst, m["data"]["task_id"]) for dst, m in env.sent if m["type"] == "task"]


def _beats(ws, *extra):
    return [(wid(w), _msg("heartbeat")) for w in ws] + list(extra)


def _mirror_ok(d):
    log = d.balancer.o.export()["log"]
    assert d.head == len(log)
    assert all(log[q] == s for q, (_, s) in d.inflight.items())
    assert {tid: q for q, (tid, _) in d.inflight.items()} == d.task_seq
    assert int((log >= 0).sum()) == len(d.inflight)  # (no worker died here: every entry >= 0 is live)


def test_hung_task_goes_to_another_worker_after_the_timeout_and_not_before(dispatcher_cls):
    env = FakeEnv()
    d = _make(dispatcher_cls, env, task_timeout=5.0)
    sent = _tick(d, env, 1000.0, [(wid(0), _msg("register", {"num_processes": 1}))], ["hang"])
    assert sent == [(wid(0), "hang")]
    # worker 1 arrives with room; worker 0 heartbeats on and never answers
    sent = _tick(d, env, 1002.0, _beats([0], (wid(1), _msg("register", {"num_processes": 1}))))
    assert sent == [] and d.reclaimed == 0
    sent = _tick(d, env, 1004.9, _beats([0, 1]))  # 4.9 s after the dispatch: not yet
    assert sent == [] and d.reclaimed == 0 and d.balancer.reclaim_calls == []
    sent = _tick(d, env, 1005.0, _beats([0, 1]))  # the deadline: taken back and sent on in the same tick
    assert sent == [(wid(1), "hang")]
    assert d.reclaimed == 1 and d.timed_out_failed == 0 and d.attempts == {"hang": 1}
    assert d.balancer.reclaim_calls == [(1, None)]
    _mirror_ok(d)
    # the first worker's late result: recorded, frees that worker, the second dispatch stays
    env.hsets.clear()
    sent = _tick(d, env, 1006.0, _beats([1], (wid(0), _result("hang"))), ["next"])
    assert ("hang", {"status": "COMPLETED", "result": 1}) in env.hsets
    assert sent == [(wid(0), "next")]  # worker 0 has a free process again
    assert d.task_seq["hang"] == 1 and d.inflight[1] == ("hang", d.slot_of[wid(1)])
    _mirror_ok(d)
    # ... and the second worker's own result completes it
    _tick(d, env, 1007.0, _beats([0], (wid(1), _result("hang"))))
    assert "hang" not in d.task_seq and "hang" not in d.attempts
    _mirror_ok(d)


def test_max_attempts_ends_in_failed(dispatcher_cls):
    env = FakeEnv()
    d = _make(dispatcher_cls, env, task_timeout=5.0, max_attempts=2)
    regs = [(wid(w), _msg("register", {"num_processes": 1})) for w in (0, 1)]
    assert _tick(d, env, 1000.0, regs[:1], ["doom"]) == [(wid(0), "doom")]
    assert _tick(d, env, 1001.0, _beats([0], regs[1])) == []
    assert _tick(d, env, 1005.0, _beats([0, 1])) == [(wid(1), "doom")]  # attempt 1 taken back, sent again
    assert _tick(d, env, 1009.0, _beats([0, 1])) == []
    env.hsets.clear()
    assert _tick(d, env, 1010.0, _beats([0, 1])) == []  # attempt 2 taken back: that was the last
    assert env.hsets == [("doom", {"status": "FAILED", "result": codec.serialize(None)})]
    assert codec.deserialize(env.hsets[0][1]["result"]) is None
    assert list(d.pending) == [] and d.inflight == {} and d.task_seq == {} and d.attempts == {}
    assert d.reclaimed == 2 and d.timed_out_failed == 1
    _mirror_ok(d)
    assert _tick(d, env, 1020.0, _beats([0, 1])) == []  # and it stays gone


def test_reclaim_after_a_register_from_a_live_identity(dispatcher_cls):
    env = FakeEnv()
    d = _make(dispatcher_cls, env)
    regs = [(wid(w), _msg("register", {"num_processes": 2})) for w in (0, 1)]
    sent = _tick(d, env, 1000.0, regs, ["a", "b", "c", "d"])
    on0 = [t for dst, t in sent if dst == wid(0)]
    on1 = [t for dst, t in sent if dst == wid(1)]
    assert len(on0) == 2 and len(on1) == 2
    # worker 0 restarts under its identity: the record stays, and so do its two entries
    sent = _tick(d, env, 1001.0, [(wid(0), _msg("register", {"num_processes": 2}))])
    assert sent == [] and sorted(d.task_seq) == ["a", "b", "c", "d"]
    back = d.reclaim([wid(0), b"nobody"])
    assert back == on0 and list(d.pending) == on0
    assert d.balancer.reclaim_calls == [(None, [d.slot_of[wid(0)]])]
    assert sorted(d.task_seq) == sorted(on1)
    _mirror_ok(d)
    # exactly those go out again, to the restarted worker's two free processes
    sent = _tick(d, env, 1002.0, _beats([0, 1]))
    assert sent == [(wid(0), t) for t in on0]
    _mirror_ok(d)
    assert d.reclaim([b"nobody"]) == []


def test_marks_survive_a_forced_compaction(dispatcher_cls):
    env = FakeEnv()
    d = _make(dispatcher_cls, env, task_timeout=5.0)
    regs = [(wid(w), _msg("register", {"num_processes": 2})) for w in (0, 1)]
    s0 = _tick(d, env, 1000.0, regs, ["a", "b", "c", "d"])          # head 4, mark (4, 1000)
    done = [(dst, _result(t)) for dst, t in s0 if t in ("a", "c")]
    s1 = _tick(d, env, 1002.0, done, ["e", "f"])                     # head 6, mark (6, 1002)
    assert len(s1) == 2 and list(d._marks) == [(4, 1000.0), (6, 1002.0)]
    d.compact_log()                                                  # b, d, e, f -> 0 .. 3
    assert d.device_compactions == 1 and d.head == 4
    assert list(d._marks) == [(2, 1000.0), (4, 1002.0)]
    snap = d.snapshot()
    assert snap["marks"] == [(2, 1000.0), (4, 1002.0)]
    # 1005: only the first tick's survivors (b, d) are due
    s2 = _tick(d, env, 1005.0, _beats([0, 1]))
    assert d.balancer.reclaim_calls == [(2, None)] and d.reclaimed == 2
    assert sorted(t for _, t in s2) == [] and list(d.pending) == ["b", "d"]  # (no free process: they wait)
    assert sorted(d.task_seq) == ["e", "f"]
    _mirror_ok(d)
    # the snapshot restores the marks and the attempt counts
    d2 = _make(dispatcher_cls, FakeEnv(), task_timeout=5.0)
    snap2 = d.snapshot()
    assert snap2["attempts"] == {"b": 1, "d": 1}
    d2.restore(snap2)
    assert list(d2._marks) == list(d._marks) and d2.attempts == d.attempts


def test_task_timeout_needs_a_balancer_with_reclaim():
    import faasbal.dispatcher as D
    from faasbal.sharded import ShardedBalancer
    assert ShardedBalancer.reclaim is None
    env = FakeEnv()
    bal = OracleBalancer(8, 64)  # (as a shard group today: no reclaim)
    with pytest.raises(FaasbalError) as e:
        D.GpuPushDispatcher("127.0.0.1", 0, 10, redis_client=env, subscriber=env, socket=env, poller=env,
                            clock=env.clock, max_workers=8, max_events=8, max_inflight=64, balancer=bal,
                            task_timeout=1.0)
    assert e.value.code == FB_ESTATE
    d = D.GpuPushDispatcher("127.0.0.1", 0, 10, redis_client=env, subscriber=env, socket=env, poller=env,
                            clock=env.clock, max_workers=8, max_events=8, max_inflight=64, balancer=bal)
    with pytest.raises(FaasbalError) as e:
        d.reclaim([wid(0)])
    assert e.value.code == FB_ESTATE


@pytest.mark.parametrize("path", (GOLDEN[0], GOLDEN[-1]), ids=lambda p: p.rsplit("/", 1)[-1][:-4])
def test_defaults_change_nothing(path, dispatcher_cls):
    """With the defaults the balancer's reclaim is never called and the golden replay's
    messages and Redis writes are the ones tests/test_dispatcher.py expects (replay_golden
    asserts them tick by tick)."""
    z = np.load(path)
    d = replay_golden(z, lambda sizes, env: dispatcher_cls(
        "127.0.0.1", 0, float(z["tte"]), **sizes, redis_client=env, subscriber=env, socket=env, poller=env,
        clock=env.clock))
    assert d.balancer.reclaim_calls == [] and d.reclaimed == 0 and len(d._marks) == 0
    snap = d.snapshot()
    assert "marks" not in snap and "attempts" not in snap
