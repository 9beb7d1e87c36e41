"""GpuPushDispatcher and the goodbye message ({"type": "leave"}, evict()) -- CPU.

The dispatcher's host logic over the leave model double (tests/leave_model.py) with the
fake sockets and Redis of tests/test_dispatcher.py; tests/test_gpu_leave.py runs the
same scenarios over the real balancer.
"""
import pytest

from faasbal import codec
from test_dispatcher import FakeEnv, wid


def _msg(env, w, m, ts):
    env.inbound.append((wid(w) if isinstance(w, int) else w, codec.serialize(m).encode(), ts))


def _make(cls, env, **kw):
    return cls("127.0.0.1", 0, 10, max_workers=16, max_events=64, max_inflight=1 << 12,
               redis_client=env, subscriber=env, socket=env, poller=env, clock=env.clock, **kw)


def _four_workers_eight_tasks(cls):
    """four workers with two processes each, eight tasks dispatched: every worker holds two"""
    env = FakeEnv()
    d = _make(cls, env)
    env.now = 1000.0
    for w in range(4):
        _msg(env, w, {"type": "register", "data": {"num_processes": 2}}, 1000.0)
    env.tasks.extend("t%d" % j for j in range(8))
    d.tick()
    first = [(dst, m["data"]["task_id"]) for dst, m in env.sent if m["type"] == "task"]
    assert len(first) == 8
    held = [tid for dst, tid in first if dst == wid(0)]
    assert len(held) == 2
    env.sent.clear()
    env.hsets.clear()
    return env, d, held


def leave_scenario(cls, how):
    """A leave (sent by the worker, or queued by evict()) releases the identity, sends
    nothing, puts the worker's tasks at the front of the pending ones; the next tick sends
    them to other workers; a later message from the identity is answered with reconnect."""
    env, d, held = _four_workers_eight_tasks(cls)
    env.now = 1001.0
    if how == "message":
        _msg(env, 0, {"type": "leave"}, 1001.0)
    else:
        assert d.evict([wid(0), b"nobody"]) == [wid(0)]
    env.tasks.append("late")
    res = d.tick()
    assert env.sent == [] and env.hsets == []                  # a leave gets no reply; nobody has a free process
    assert wid(0) not in d.slot_of and wid(0) not in d.workers and wid(0) not in d.free_workers
    assert b"nobody" not in d.slot_of
    assert res["n_orphans"] == 2 and list(d.pending) == held + ["late"]   # the worker's tasks stand in front
    assert all(d.identity[s] != wid(0) for _, s in d.inflight.values())
    # worker 1 finishes its two tasks: the next tick sends the two orphans to it, ahead of "late"
    env.now = 1002.0
    for tid in [tid for q, (tid, s) in sorted(d.inflight.items()) if d.identity[s] == wid(1)]:
        _msg(env, 1, {"type": "result", "data": {"task_id": tid, "status": "COMPLETED", "result": "r"}}, 1002.0)
    d.tick()
    assert [(dst, m["data"]["task_id"]) for dst, m in env.sent if m["type"] == "task"] == [(wid(1), t) for t in held]
    assert list(d.pending) == ["late"]
    env.sent.clear()
    # the identity speaks again: unknown, so it is asked to reconnect (:356-358)
    env.now = 1003.0
    _msg(env, 0, {"type": "heartbeat"}, 1003.0)
    d.tick()
    assert (wid(0), {"type": "reconnect"}) in env.sent
    assert wid(0) in d.slot_of and d.workers[wid(0)].free_processes == 0
    return d


def unknown_leave_scenario(cls):
    """A leave from an identity that has no slot allocates none and makes no event."""
    env, d, _ = _four_workers_eight_tasks(cls)
    before = (d._next_slot, list(d._free_slots), dict(d.slot_of))
    seen = []
    tick0 = d.balancer.tick

    def spy(now, tte, kind, *a, **kw):
        seen.append(len(kind))
        return tick0(now, tte, kind, *a, **kw)

    d.balancer.tick = spy
    env.now = 1001.0
    _msg(env, b"stranger", {"type": "leave"}, 1001.0)
    _msg(env, 1, {"type": "heartbeat"}, 1001.0)
    d.tick()
    assert seen == [1]                                          # the heartbeat alone
    assert (d._next_slot, list(d._free_slots), dict(d.slot_of)) == before
    assert env.sent == []
    # ... but a leave behind the identity's own register in one batch is an event: the
    # register gives the slot, the leave takes the record, the tick hands the slot back
    seen.clear()
    env.now = 1002.0
    _msg(env, b"brief", {"type": "register", "data": {"num_processes": 1}}, 1002.0)
    _msg(env, b"brief", {"type": "leave"}, 1002.0)
    d.tick()
    assert seen == [2] and b"brief" not in d.slot_of and b"brief" not in d.workers
    assert d._next_slot == before[0] + 1 and d._free_slots == [before[0]]
    return d


def deque_scenario(cls):
    """The loop without heartbeats ignores a leave (start() acts on register and result only)."""
    env = FakeEnv()
    d = _make(cls, env)
    d.use_loop("deque")
    _msg(env, 0, {"type": "register", "data": {"num_processes": 2}}, 0.0)
    _msg(env, 1, {"type": "register", "data": {"num_processes": 1}}, 0.0)
    d.tick()
    _msg(env, 0, {"type": "leave"}, 1.0)
    assert d.evict([wid(1)]) == [wid(1)]
    env.tasks.extend(["a", "b", "c"])
    d.tick()
    assert sorted(d.workers) == [wid(0), wid(1)]
    assert sorted(dst for dst, m in env.sent if m["type"] == "task") == [wid(0), wid(0), wid(1)]
    return d


@pytest.fixture
def model_cls(monkeypatch):
    import faasbal.dispatcher as D
    from leave_model import LeaveModelBalancer
    monkeypatch.setattr(D, "GpuBalancer", LeaveModelBalancer)
    return D.GpuPushDispatcher


@pytest.mark.parametrize("how", ["message", "evict"])
def test_leave_releases_the_worker_and_redistributes(model_cls, how):
    leave_scenario(model_cls, how)


def test_leave_from_unknown_identity_allocates_nothing(model_cls):
    unknown_leave_scenario(model_cls)


def test_evict_counts_against_max_events(model_cls):
    env = FakeEnv()
    d = model_cls("127.0.0.1", 0, 10, max_workers=16, max_events=3, max_inflight=1 << 12,
                  redis_client=env, subscriber=env, socket=env, poller=env, clock=env.clock)
    env.now = 1.0
    for w in range(3):
        _msg(env, w, {"type": "register", "data": {"num_processes": 1}}, 1.0)
    d.tick()
    assert d.evict([wid(0), wid(1)]) == [wid(0), wid(1)]
    for w in (2, 2):
        _msg(env, w, {"type": "heartbeat"}, 2.0)
    env.now = 2.0
    d.tick()                                                    # two leaves + one heartbeat fill the batch
    assert len(env.inbound) == 1 and sorted(d.slot_of) == [wid(2)]


def test_deque_mode_ignores_the_leave(model_cls):
    deque_scenario(model_cls)
