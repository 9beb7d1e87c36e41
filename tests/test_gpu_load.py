"""What a load installs, on the device: the states and the numpy statement of tests/load_cases.py
(the ones tests/test_load_host.py holds csrc/faasbal_load.h to) against what fb_read_state,
fb_read_inflight, fb_read_shard_log and fb_device_view_get show after fb_load_state /
fb_load_shard -- on a one-GPU heartbeat context with in-flight counts, one with window buffers,
a deque, the ranks of a 3-rank group (70 slots each way) and one heartbeat context of
(1 << 17) + 1 slots, the smallest on the in-place / window side of the context kinds.

Then: a rejected load changes nothing (one offending load per class of refusal, the state read
back and one tick against tests/gpu_model.py), also over a stale log; and a load over a
launched, uncommitted tick installs cleanly.
"""
import ctypes as C

import numpy as np
import pytest

import gpu_model
import load_cases as lc
from faasbal import GpuBalancer, _lib, synth
from faasbal.sharded import LocalShardGroup

pytestmark = pytest.mark.gpu

CAP, E_CAP = 256, 256
BIG = (1 << 17) + 1
NOW, TTE = 1045.0, 30.0  # (heartbeats lie in [1000, 1050): some registrations expire)


def make(kind):
    if kind == "shard":
        return LocalShardGroup(lc.WORLD, lc.W, CAP, max_events=E_CAP)
    if kind == "big":
        g = GpuBalancer(BIG, 4096, max_events=E_CAP)
        g.set_window(1)  # (created with window buffers; 1: the first tick after a load may be a window tick)
        return g
    g = GpuBalancer(lc.W, CAP, max_events=E_CAP, mode="deque" if kind == "deque" else "heartbeat")
    if kind == "win":
        g.set_window(1)  # allocates the window buffers: a window-capable context from here on
    return g


@pytest.fixture(scope="module")
def ctxs():
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = make(kind)
        return made[kind]
    yield get
    for g in made.values():
        g.close()


def dev(ptr, shape, typestr):
    """A device array of the library's, on the host."""
    import torch
    if not int(np.prod(shape)):
        return np.zeros(shape, np.dtype(typestr))

    class Dev:
        __cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(int(ptr), False), version=2)
    return torch.as_tensor(Dev(), device="cuda:0").cpu().numpy()


def check_rank(g, f, a, what):
    """One context against the image of the load it was given."""
    want = lc.image(f, a)
    n = a["n"]
    st = g.read_state()
    for k in ("reg", "free", "epoch"):
        np.testing.assert_array_equal(st[k], want[k], err_msg="%s: %s" % (what, k))
    np.testing.assert_array_equal(np.isnan(st["hb"]), want["reg"] == 0, err_msg=what + ": NaN where no record")
    np.testing.assert_array_equal(st["hb"][want["reg"] == 1], want["hb"][want["reg"] == 1], err_msg=what + ": hb")
    np.testing.assert_array_equal(st["queue"], a["queue"], err_msg=what + ": queue")
    np.testing.assert_array_equal(st["log"], want["log"], err_msg=what + ": log")
    if f["sharded"]:
        np.testing.assert_array_equal(st["log_seq"], a["log_seq"], err_msg=what + ": log_seq")
        assert (st["head"], st["log_len"], st["base"]) == (a["log_head"], len(a["log_slot"]), a["base"]), what
    else:
        assert st["head"] == len(a["log_slot"]), what
    if f["inflight"]:
        np.testing.assert_array_equal(g.inflight(), np.where(want["reg"] == 1, want["bud"] - want["free"], 0),
                                      err_msg=what + ": in-flight counts")
    # the device's own arrays: the in-queue flag beside the free count, the NaNs, the queue, the log
    v = g.device_view()
    assert (v.n_workers, v.queue_len, v.log_head) == (n, len(a["queue"]), a["log_head"]), what
    assert (v.free_processes_stride, v.last_heartbeat_stride) == (8, 8)
    fq = dev(v.free_processes, (n, 2), "<i4")
    np.testing.assert_array_equal(fq[:, 0], want["free"], err_msg=what + ": free (device)")
    np.testing.assert_array_equal(fq[:, 1], want["inq"], err_msg=what + ": in-queue flag (device)")
    hb = dev(v.last_heartbeat, (n,), "<f8")
    np.testing.assert_array_equal(np.isnan(hb), want["reg"] == 0, err_msg=what + ": NaN (device)")
    np.testing.assert_array_equal(dev(v.registered, (n,), "|u1"), want["reg"], err_msg=what + ": reg (device)")
    np.testing.assert_array_equal(dev(v.queue, (len(a["queue"]),), "<i4"), a["queue"], err_msg=what + ": queue (device)")
    np.testing.assert_array_equal(dev(v.log_slot, (len(a["log_slot"]),), "<i4"), want["log"], err_msg=what + ": log (device)")


def check_loaded(g, kind, st, what):
    if kind == "shard":
        for r, b in enumerate(g.bals):
            check_rank(b, lc.facts("shard", W_cap=24), lc.local_state(st, "shard", r), "%s rank %d" % (what, r))
    else:
        k = "win" if kind == "big" else kind
        # (70 slots with window buffers: fb_set_window gave them to a context that keeps in-flight counts)
        f = dict(lc.facts(k, W_cap=len(st["reg"])), inflight=int(kind in ("hb", "win")))
        check_rank(g, f, lc.local_state(st, k), what)


def messages(st, deque):
    """A few messages that are valid on every kind: a registration of the slot without a record,
    a result that completes entry 150 of slot 5; on heartbeat contexts also a heartbeat and a
    reconnect."""
    rows = [(synth.EV_REGISTER, 3, 2, -1), (synth.EV_RESULT, 5, 0, 150)]
    if not deque:
        rows += [(synth.EV_HEARTBEAT, 7, 0, -1), (synth.EV_RECONNECT, 11, 3, -1)]
    k, s, v, q = (np.array(c) for c in zip(*rows))
    return k.astype(np.uint8), s.astype(np.int32), v.astype(np.int32), np.full(len(k), NOW - 1.0), q.astype(np.int64)


def model_tick(st, ev, T, deque):
    m = dict(st, epoch=np.zeros(len(st["reg"]), np.uint32) if st.get("epoch") is None else st["epoch"])
    if deque:
        return gpu_model.tick_deque(gpu_model.deque_load(m), *ev, T)[0]
    return gpu_model.tick(m, NOW, TTE, *ev, T)[0]


def check_tick(g, st, what, T=30):
    deque = getattr(g, "mode", "") == "deque"
    ev = messages(st, deque)
    got, want = g.tick(NOW, TTE, *ev, n_pending=T), model_tick(st, ev, T, deque)
    for k in ("reconnect", "assign", "orphans", "evicted"):
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s: the tick's %s" % (what, k))


STATES = {}


def state(kind, seed=1):
    key = (kind, seed)
    if key not in STATES:
        STATES[key] = lc.global_state(seed, deque=kind == "deque", n=BIG if kind == "big" else lc.W)
    return STATES[key]


# --------------------------------------------------------------------------- what the device holds
@pytest.mark.parametrize("kind", lc.KINDS + ("big",))
def test_device_holds_the_image(ctxs, kind):
    g = ctxs(kind)
    variants = [("full", state(kind))]
    if kind != "big":
        variants += [("null_epoch", lc.global_state(2, deque=kind == "deque", null_epoch=True)),
                     ("no_queue_no_log", dict(lc.global_state(3, log=0), queue=np.zeros(0, np.int32)))]
    for name, st in variants:
        g.load(st)
        check_loaded(g, kind, st, "%s/%s" % (kind, name))
    g.load(state(kind))
    check_tick(g, state(kind), kind)  # (win, big: free to run as a window tick, on the positions the load installed)


# --------------------------------------------------------------------------- a rejected load
def raw_load(b, f, a, counts=None):
    """fb_load_state / fb_load_shard through the C ABI, null pointers and miscounts included."""
    def p(x):
        return None if x is None or x is lc.NULL else np.ascontiguousarray(x).ctypes.data_as(C.c_void_p)
    c = dict(qlen=0 if a["queue"] is lc.NULL else len(a["queue"]), llen=0 if a["log_slot"] is lc.NULL else len(a["log_slot"]))
    c.update(counts or {})
    for k, dt in (("reg", np.uint8), ("free", np.int32), ("hb", np.float64), ("queue", np.int32), ("log_slot", np.int32)):
        assert a[k] is lc.NULL or (a[k].dtype == dt and a[k].flags["C_CONTIGUOUS"]), k  # (passed as they are)
    arr = {k: p(a[k]) for k in ("reg", "free", "hb", "epoch", "queue", "log_slot", "log_seq")}
    if f["sharded"]:
        rc = b.lib.fb_load_shard(b.h, a["base"], a["n"], arr["reg"], arr["free"], arr["hb"], arr["epoch"], arr["queue"],
                                 c["qlen"], arr["log_slot"], arr["log_seq"], c["llen"], a["log_head"])
    else:
        rc = b.lib.fb_load_state(b.h, a["n"], arr["reg"], arr["free"], arr["hb"], arr["epoch"], arr["queue"], c["qlen"],
                                 arr["log_slot"], c["llen"])
    return rc, (b.lib.fb_last_error(b.h) or b"").decode()


def offences(f, a):
    """One offending load per class of refusal, made from the accepted load a: (change, counts,
    the condition's words)."""
    base, n = a["base"], a["n"]
    bad_q = a["queue"].copy()
    bad_q[-1] = f["W_cap"] + 9 if f["deque"] else bad_q[0]  # out of range (a deque may repeat); a repeat
    out = [(dict(n=f["W_cap"] + 1), {}, "slot range" if f["sharded"] else "n_workers"),
           (dict(queue=bad_q), {}, "queue[%d] = %d is out of range" % (len(bad_q) - 1, bad_q[-1])),
           (dict(log_slot=np.append(a["log_slot"][:-1], base + n + 1).astype(np.int32)), {}, "log_slot["),
           (dict(reg=lc.NULL), {}, "registered is null")]
    if f["sharded"]:
        out.append((dict(log_seq=a["log_seq"][::-1].copy()), {}, "log_seq must ascend"))
    return out


def reject_all(g, kind, st):
    ranks = g.bals if kind == "shard" else [g]
    n_bad = 0
    for r, b in enumerate(ranks):
        k = "win" if kind == "big" else kind
        f, a = lc.facts(k, W_cap=b.max_workers), lc.local_state(st, k, r)
        for change, counts, words in offences(f, a):
            rc, msg = raw_load(b, f, dict(a, **change), counts)
            assert rc == _lib.FB_EINVAL and words in msg, (kind, r, words, rc, msg)
            n_bad += 1
    return n_bad


@pytest.mark.parametrize("kind", lc.KINDS)
def test_rejected_load_changes_nothing(ctxs, kind):
    g, st = ctxs(kind), state(kind)
    g.load(st)
    assert reject_all(g, kind, st) == (15 if kind == "shard" else 4)
    check_loaded(g, kind, st, kind + " after the rejected loads")
    check_tick(g, st, kind + " after the rejected loads")


def test_rejected_load_over_a_stale_log():
    """A committed tick leaves its orphans in the log (lazy clears); the state is read without
    the log, as ADVICE.md describes, so they stay.  A rejected load must leave them dead: the
    slot registers again, takes tasks and expires again, and only its new entries are orphans."""
    Wn, now, tte = lc.W, 1000.0, 10.0
    st = dict(reg=np.ones(Wn, np.uint8), free=np.full(Wn, 2, np.int32), hb=np.full(Wn, now - 1.0),
              epoch=np.zeros(Wn, np.uint32), queue=np.arange(Wn, dtype=np.int32), log=np.asarray([0, 0, 0, 0, 1, 2], np.int32))
    st["hb"][0] = now - 9.0

    def others(t, reg0=False):
        n = Wn - 1 + int(reg0)
        kind, slot, val = np.full(n, synth.EV_HEARTBEAT, np.uint8), np.arange(1, n + 1, dtype=np.int32), np.zeros(n, np.int32)
        if reg0:
            kind[-1], slot[-1], val[-1] = synth.EV_REGISTER, 0, 2
        return kind, slot, val, np.full(n, t), np.full(n, -1, np.int64)

    g = GpuBalancer(Wn, 1024, max_events=2 * Wn)
    g.load(st)
    carried = 0
    plan = [(now + 2.0, False, 0), None, (now + 3.0, True, 200), (now + 10.0, False, 1), (now + 14.0, False, 0)]
    orphans = []
    for step in plan:
        if step is None:
            seen = g.read_state(with_log=False)
            np.testing.assert_array_equal(seen["queue"], st["queue"])
            f, a = lc.facts("hb"), lc.local_state(st, "hb")
            for change, counts, words in offences(f, a):
                rc, msg = raw_load(g, f, dict(a, **change), counts)
                assert rc == _lib.FB_EINVAL and words in msg, (words, rc, msg)
            continue
        t, reg0, n_new = step
        ev, T = others(t, reg0), carried + n_new
        got = g.tick(t, tte, *ev, n_pending=T)
        want, st = gpu_model.tick(st, t, tte, *ev, T)
        for k in ("reconnect", "assign", "orphans", "evicted"):
            np.testing.assert_array_equal(got[k], want[k], err_msg="tick at %.1f: %s" % (t, k))
        carried = T + len(want["orphans"]) - len(want["assign"])
        orphans.append(want["orphans"].tolist())
    assert orphans[0] == [0, 1, 2, 3] and len(orphans[3]) == 2 and min(orphans[3]) > 5  # (the new entries only)
    g.close()


# --------------------------------------------------------------------------- over a launched tick
@pytest.mark.parametrize("kind", ("hb", "shard"))
def test_load_over_a_launched_uncommitted_tick(ctxs, kind):
    g, st, other = ctxs(kind), state(kind), lc.global_state(7)
    g.load(other)
    ev = messages(other, False)
    for b in (g.bals if kind == "shard" else [g]):
        b.launch(NOW, TTE, *ev, n_pending=20)  # (a rank: phase 1; never waited for, never committed)
    g.load(st)
    check_loaded(g, kind, st, kind + " over a launched tick")
    check_tick(g, st, kind + " over a launched tick")
