"""GpuPushDispatcher and the planned shutdown ({"type": "drain"} / {"type": "resume"},
drain(), resume(), draining(), evict_drained) -- CPU, and one case on the GPU.

The dispatcher's host logic over the drain model double (tests/drain_model.py) with the
fake sockets and Redis of tests/test_dispatcher.py, as tests/test_leave_dispatcher.py runs
the goodbye; the last test runs the same scenarios over the real balancer.
"""
import pytest

from test_dispatcher import FakeEnv, wid
from test_leave_dispatcher import _four_workers_eight_tasks, _make, _msg


def _tasks_sent(env):
    return [(dst, m["data"]["task_id"]) for dst, m in env.sent if m["type"] == "task"]


def _held_by(d, w):
    return [tid for q, (tid, s) in sorted(d.inflight.items()) if d.identity[s] == wid(w)]


def _result(env, w, tid, ts):
    _msg(env, w, {"type": "result", "data": {"task_id": tid, "status": "COMPLETED", "result": "r"}}, ts)


def drain_scenario(cls, how, end):
    """Worker 0 of four, each holding two tasks, drains (its own message, or drain()): it gets
    no task while its results are still written and draining() counts down; then evict_drained
    lets it go without re-queuing anything, or a resume brings it back first in line."""
    env, d, held = _four_workers_eight_tasks(cls)
    w0 = wid(0)
    # ---- the drain; a drain for an identity without a slot allocates none
    env.now = 1001.0
    before = (d._next_slot, list(d._free_slots))
    if how == "message":
        _msg(env, 0, {"type": "drain"}, 1001.0)
        _msg(env, b"nobody", {"type": "drain"}, 1001.0)
        _msg(env, b"nobody", {"type": "resume"}, 1001.0)
    else:
        assert d.drain([w0, b"nobody"]) == [w0]
        assert d.resume([b"nobody"]) == []
    res = d.tick()
    assert env.sent == [] and env.hsets == []                  # a drain gets no reply
    assert res["n_orphans"] == 0 and not d.pending             # nothing is dispatched a second time
    assert b"nobody" not in d.slot_of and (d._next_slot, list(d._free_slots)) == before
    assert d.draining() == {w0: 2}
    v = d.workers[w0]
    assert v.draining and v.free_processes == 0 and w0 not in d.free_workers
    assert not any(x.draining for w, x in d.workers.items() if w != w0)
    assert _held_by(d, 0) == held                              # its tasks stay in flight, on it
    # ---- its first result: written; a task is pending, it has a free process, it gets nothing
    env.now = 1002.0
    _result(env, 0, held[0], 1002.0)
    env.tasks.append("n0")
    d.tick()
    assert env.hsets == [(held[0], {"status": "COMPLETED", "result": "r"})]
    assert _tasks_sent(env) == [] and list(d.pending) == ["n0"]
    assert d.draining() == {w0: 1}
    v = d.workers[w0]
    assert v.draining and v.free_processes == 1 and v.last_heartbeat == 1002.0 and w0 not in d.free_workers
    # ---- its second result, and one each of workers 2 and 3: "n0" goes to worker 2
    env.now = 1003.0
    _result(env, 0, held[1], 1003.0)
    _result(env, 2, _held_by(d, 2)[0], 1003.0)
    _result(env, 3, _held_by(d, 3)[0], 1003.0)
    d.tick()
    assert _tasks_sent(env) == [(wid(2), "n0")]
    assert d.draining() == {w0: 0} and d.workers[w0].free_processes == 2
    assert d.free_workers == [wid(3)]
    env.sent.clear()
    env.hsets.clear()
    env.now = 1004.0
    if end == "evict":
        # ---- drained dry: the next tick lets it go; nothing was in flight, nothing is re-queued
        d.evict_drained = True
        res = d.tick()
        assert res["n_orphans"] == 0 and not d.pending and env.sent == [] and env.hsets == []
        assert w0 not in d.slot_of and w0 not in d.workers and d.draining() == {}
        assert d.free_workers == [wid(3)]
        # the identity speaks again: unknown, so it is asked to reconnect
        env.now = 1005.0
        _msg(env, 0, {"type": "heartbeat"}, 1005.0)
        d.tick()
        assert (w0, {"type": "reconnect"}) in env.sent and not d.workers[w0].draining
    else:
        # ---- the resume: first in line, ahead of worker 3, which has been queued since the last tick
        if how == "message":
            _msg(env, 0, {"type": "resume"}, 1004.0)
        else:
            assert d.resume([w0]) == [w0]
        env.tasks.extend(["x", "y", "z"])
        d.tick()
        assert _tasks_sent(env) == [(w0, "x"), (wid(3), "y"), (w0, "z")]
        assert d.draining() == {} and not d.workers[w0].draining and d.workers[w0].free_processes == 0
    return d


def snapshot_scenario(cls):
    """snapshot() / restore() keep the draining set: it is rebuilt from the loaded free counts."""
    env, d, held = _four_workers_eight_tasks(cls)
    env.now = 1001.0
    assert d.drain([wid(0), wid(2)]) == [wid(0), wid(2)]
    _result(env, 2, _held_by(d, 2)[0], 1001.0)
    d.tick()
    assert d.draining() == {wid(0): 2, wid(2): 1}
    snap = d.snapshot()
    env2 = FakeEnv()
    d2 = _make(cls, env2)
    d2.restore(snap)
    assert d2.draining() == {wid(0): 2, wid(2): 1}
    assert d2.workers[wid(2)].draining and d2.workers[wid(2)].free_processes == 1
    # the restored dispatcher goes on: worker 1's result queues it, the draining two get nothing
    env2.now = 1002.0
    _result(env2, 1, _held_by(d2, 1)[0], 1002.0)
    _result(env2, 2, _held_by(d2, 2)[0], 1002.0)
    env2.tasks.extend(["p", "q"])
    d2.tick()
    assert _tasks_sent(env2) == [(wid(1), "p")] and list(d2.pending) == ["q"]
    assert d2.draining() == {wid(0): 2, wid(2): 0}
    d.balancer.close()
    return d2


def deque_scenario(cls):
    """The loop without heartbeats ignores both messages (start() acts on register and result only)."""
    env = FakeEnv()
    d = _make(cls, env)
    d.use_loop("deque")
    _msg(env, 0, {"type": "register", "data": {"num_processes": 2}}, 0.0)
    _msg(env, 1, {"type": "register", "data": {"num_processes": 1}}, 0.0)
    d.tick()
    _msg(env, 0, {"type": "drain"}, 1.0)
    _msg(env, 0, {"type": "resume"}, 1.0)
    assert d.drain([wid(1)]) == [wid(1)]
    env.tasks.extend(["a", "b", "c"])
    d.tick()
    assert d.draining() == {}
    assert sorted(d.workers) == [wid(0), wid(1)] and not any(v.draining for v in d.workers.values())
    assert sorted(dst for dst, m in env.sent if m["type"] == "task") == [wid(0), wid(0), wid(1)]
    return d


@pytest.fixture
def model_cls(monkeypatch):
    import faasbal.dispatcher as D
    from drain_model import DrainModelBalancer
    monkeypatch.setattr(D, "GpuBalancer", DrainModelBalancer)
    return D.GpuPushDispatcher


@pytest.mark.parametrize("end", ["evict", "resume"])
@pytest.mark.parametrize("how", ["message", "call"])
def test_drained_worker_gets_no_task_and_finishes_what_it_has(model_cls, how, end):
    drain_scenario(model_cls, how, end)


def test_snapshot_and_restore_keep_the_draining_set(model_cls):
    snapshot_scenario(model_cls)


def test_deque_mode_ignores_drain_and_resume(model_cls):
    deque_scenario(model_cls)


def test_register_and_leave_end_a_drain_in_the_host_mirror(model_cls):
    """A restarted worker is a fresh worker, and a leave deletes the record as ever: its tasks
    are re-queued, the mark goes with the record."""
    env, d, held = _four_workers_eight_tasks(model_cls)
    env.now = 1001.0
    d.drain([wid(0), wid(1)])
    d.tick()
    assert d.draining() == {wid(0): 2, wid(1): 2}
    env.now = 1002.0
    _msg(env, 0, {"type": "register", "data": {"num_processes": 2}}, 1002.0)
    _msg(env, 1, {"type": "leave"}, 1002.0)
    res = d.tick()
    assert d.draining() == {} and not d.workers[wid(0)].draining and wid(1) not in d.slot_of
    assert res["n_orphans"] == 2 and len(_tasks_sent(env)) == 2 and all(dst == wid(0) for dst, _ in _tasks_sent(env))


def test_drains_count_against_max_events(model_cls):
    env = FakeEnv()
    d = model_cls("127.0.0.1", 0, 10, max_workers=16, max_events=3, max_inflight=1 << 12,
                  redis_client=env, subscriber=env, socket=env, poller=env, clock=env.clock)
    env.now = 1.0
    for w in range(3):
        _msg(env, w, {"type": "register", "data": {"num_processes": 1}}, 1.0)
    d.tick()
    d.evict([wid(0)])
    d.drain([wid(1), wid(2)])
    for w in (2, 2):
        _msg(env, w, {"type": "heartbeat"}, 2.0)
    env.now = 2.0
    d.tick()                                                    # the leave and the two drains fill the batch
    assert len(env.inbound) == 2 and sorted(d.slot_of) == [wid(1), wid(2)]
    assert d.draining() == {wid(1): 0, wid(2): 0}


def test_evict_drained_queues_one_leave_behind_a_full_batch(model_cls):
    """A drained-dry identity's goodbye that waits behind a full batch is not queued a second
    time: a copy surfacing later would evict the worker after it had registered again."""
    env = FakeEnv()
    d = model_cls("127.0.0.1", 0, 10, max_workers=16, max_events=2, max_inflight=1 << 12,
                  redis_client=env, subscriber=env, socket=env, poller=env, clock=env.clock, evict_drained=True)
    env.now = 1.0
    for w in range(2):
        _msg(env, w, {"type": "register", "data": {"num_processes": 1}}, 1.0)
    d.tick()
    d.drain([wid(0)])
    d.tick()
    assert d.draining() == {wid(0): 0}
    d.evict([wid(1), b"x"])                                     # two goodbyes ahead of worker 0's fill the batch
    env.now = 2.0
    d.tick()
    assert list(d._leaving) == [wid(0)] and wid(0) in d.slot_of
    d.evict([b"y", b"z"])
    d._leaving.rotate(2)                                        # ... and again
    d.tick()
    assert list(d._leaving) == [wid(0)]
    d.tick()
    assert not d._leaving and wid(0) not in d.slot_of and d.draining() == {}
    env.now = 3.0
    _msg(env, 0, {"type": "register", "data": {"num_processes": 1}}, 3.0)
    d.tick()
    d.tick()
    assert wid(0) in d.workers and d.free_workers == [wid(0)]


def test_mirror_follows_the_free_count_a_register_writes(model_cls):
    """The mark is the free count: a reconnect with a count below FB_DRAIN_BELOW reads as
    draining on the device and in WorkerView, and so it does in draining()."""
    env, d, held = _four_workers_eight_tasks(model_cls)
    env.now = 1001.0
    _msg(env, 0, {"type": "reconnect", "data": {"free_processes": -(1 << 30) + 1}}, 1001.0)
    d.tick()
    assert d.workers[wid(0)].draining and d.workers[wid(0)].free_processes == 1
    assert d.draining() == {wid(0): 2}
    env.now = 1002.0
    _msg(env, 0, {"type": "reconnect", "data": {"free_processes": 0}}, 1002.0)
    d.tick()
    assert d.draining() == {} and not d.workers[wid(0)].draining


@pytest.mark.gpu
@pytest.mark.parametrize("how,end", [("call", "evict"), ("message", "resume")])
def test_dispatcher_drain_over_the_real_balancer(how, end):
    from faasbal.dispatcher import GpuPushDispatcher
    drain_scenario(GpuPushDispatcher, how, end).balancer.close()


@pytest.mark.gpu
def test_dispatcher_snapshot_and_deque_over_the_real_balancer():
    from faasbal.dispatcher import GpuPushDispatcher
    snapshot_scenario(GpuPushDispatcher).balancer.close()
    deque_scenario(GpuPushDispatcher).balancer.close()
