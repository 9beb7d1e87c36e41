"""One tick with the goodbye message (FB_EV_LEAVE) -- TEST ONLY.

A plain sequential Python restatement of one tick, in the order of oracle_tick
(oracle/push_oracle.c): per message purge, handle, purge; then the dispatch phase at
`now`, orphans ascending and first.  The C oracle follows the reference, which has no
goodbye, so it cannot say what a leave does; this model can, and tests/test_leave_model.py
pins it to the C oracle wherever the two can be compared.

The rule for one leave at clock ts from slot s (include/faasbal.h):

- Purge first.  The purge at ts runs before it, as before every message.
- s holds a record: the record is deleted exactly as that purge deletes an expired one --
  the record is gone, the slot is out of the LRU queue, and a registration that existed at
  tick start counts as died-at-start: its in-flight entries (sequence >= its epoch) are this
  tick's orphans, dispatched first.
- Later messages of s in the same tick meet an unknown identity: a register opens a new
  registration (epoch = the log head at tick start), anything else creates the free = 0
  record and is answered with a reconnect.
- s holds no record at that point: nothing happens.  No record is created and no reconnect
  is asked for.
- The status is 0 (applied) in both cases; val and seq are ignored.
- The evicted list keeps the kernels' rule: a slot is listed when it held a record at tick
  start or got any message in the tick, and holds no record after the tick.
"""
import numpy as np

from faasbal._lib import FB_ENOSPC, FaasbalError
from oracle import DequeOracle

EV_REGISTER, EV_RECONNECT, EV_HEARTBEAT, EV_RESULT, EV_OTHER, EV_LEAVE = 0, 1, 2, 3, 4, 5


class LeaveModel:
    def __init__(self, W, log_cap):
        self.W, self.cap = int(W), int(log_cap)
        self.load(np.zeros(W, np.uint8), np.zeros(W, np.int32), np.zeros(W), np.zeros(W, np.uint32), (), ())

    def load(self, reg, free, hb, epoch, queue, log):
        W = self.W
        self.reg = np.asarray(reg)[:W].astype(bool)  # (reg and hb as arrays: the purge is one expression)
        self.free = [int(x) for x in np.asarray(free)[:W]]
        self.hb = np.array(np.asarray(hb)[:W], np.float64)
        self.epoch = [int(x) for x in np.asarray(epoch)[:W]]
        self.queue = [int(s) for s in queue]  # LRU order, front first, no duplicates
        if len(set(self.queue)) != len(self.queue) or any(not self.reg[s] for s in self.queue):
            raise ValueError("inconsistent state")
        if len(log) > self.cap:
            raise ValueError("inconsistent state")
        # live entries of current registrations only (oracle_load)
        self.log = [-1 if (s >= 0 and (not self.reg[s] or q < self.epoch[s])) else int(s)
                    for q, s in enumerate(np.asarray(log, np.int64).tolist())]

    def export(self):
        return dict(reg=self.reg.astype(np.uint8), free=np.asarray(self.free, np.int32),
                    hb=self.hb.copy(), epoch=np.asarray(self.epoch, np.uint32),
                    queue=np.asarray(self.queue, np.int32), log=np.asarray(self.log, np.int32).reshape(-1),
                    head=len(self.log))

    # -------------------------------------------------------------- loop pieces
    def _evict(self, s):
        """purge_workers' deletion of one record (evict() in push_oracle.c)"""
        self.reg[s] = False
        if s in self._inq:
            self._inq.discard(s)
            self.queue.remove(s)
        if self._cur_is_start[s]:
            self._died_start[s] = True
            self._cur_is_start[s] = False

    def _purge(self, t, tte):
        # time.time() - last_heartbeat > time_to_expire, fp64 subtract then compare
        for s in np.nonzero(self.reg & ((t - self.hb) > tte))[0]:
            self._evict(int(s))

    def _front(self, s):
        if s in self._inq:
            self.queue.remove(s)
        self.queue.insert(0, s)
        self._inq.add(s)

    def _handle(self, kind, s, val, t, seq, head_in):
        if kind == EV_REGISTER:
            if not self.reg[s]:
                self.reg[s], self.epoch[s] = True, head_in
            self.hb[s], self.free[s] = t, val
            if val > 0:
                self._front(s)
            return 0
        if kind == EV_LEAVE:
            if self.reg[s]:
                self._evict(s)
            return 0
        if not self.reg[s]:
            self.reg[s], self.epoch[s], self.free[s], self.hb[s] = True, head_in, 0, t
            return 1
        if kind == EV_RECONNECT:
            self.hb[s], self.free[s] = t, val
            if val > 0:
                self._front(s)
        elif kind == EV_HEARTBEAT:
            self.hb[s] = t
        elif kind == EV_RESULT:
            self.free[s] += 1
            self.hb[s] = t
            if 0 <= seq < head_in and self.log[seq] == s:
                self.log[seq] = -1
            if self.free[s] == 1 and s not in self._inq:
                self.queue.append(s)
                self._inq.add(s)
        return 0

    def _orphans(self, head_in, start_epoch):
        return [q for q in range(head_in)
                if self.log[q] >= 0 and self._died_start[self.log[q]] and q >= start_epoch[self.log[q]]]

    def tick(self, now, tte, ev_kind, ev_slot, ev_val, ev_ts, ev_seq, n_pending, dispatch_limit=-1):
        W, head_in = self.W, len(self.log)
        E = len(ev_kind)
        reg0 = self.reg.copy()
        self._cur_is_start = [bool(x) for x in self.reg]
        self._died_start = [False] * W
        self._inq = set(self.queue)
        start_epoch = list(self.epoch)
        touched = [False] * W
        status = np.zeros(E, np.uint8)
        for i in range(E):
            s, t = int(ev_slot[i]), float(ev_ts[i])
            self._purge(t, tte)
            touched[s] = True
            status[i] = self._handle(int(ev_kind[i]), s, int(ev_val[i]), t,
                                     int(ev_seq[i]) if ev_seq is not None else -1, head_in)
            self._purge(t, tte)
        orph, assign, N = None, [], -1
        while True:
            self._purge(now, tte)
            if not self.queue:
                break
            if orph is None:
                orph = self._orphans(head_in, start_epoch)
                N = len(orph) + int(n_pending)
            if len(assign) >= N or (0 <= dispatch_limit <= len(assign)):
                break
            if head_in + len(assign) >= self.cap:
                raise RuntimeError("oracle log overflow")
            w = self.queue.pop(0)
            self._inq.discard(w)
            self.log.append(w)
            assign.append(w)
            self.free[w] -= 1
            if self.free[w] > 0:
                self.queue.append(w)
                self._inq.add(w)
        if orph is None:
            orph = self._orphans(head_in, start_epoch)
        for q in orph:
            self.log[q] = -1
        evicted = [s for s in range(W) if (reg0[s] or touched[s]) and not self.reg[s]]
        return dict(reconnect=status, assign=np.asarray(assign, np.int32).reshape(-1),
                    orphans=np.asarray(orph, np.int64).reshape(-1), evicted=np.asarray(evicted, np.int32).reshape(-1))


class LeaveModelBalancer:
    """TEST DOUBLE with OracleBalancer's call shape (tests/oracle_balancer.py), over the
    model above; deque contexts, which know no leave, over the C deque oracle."""

    def __init__(self, max_workers, max_log, max_events=0, device=0, mode="heartbeat", max_tokens=None):
        self.mode = mode
        self.o = DequeOracle(max_workers, max_log) if mode == "deque" else LeaveModel(max_workers, max_log)

    def close(self):
        pass

    def load_state(self, reg, free, hb, epoch=None, queue=(), log=()):
        epoch = np.zeros(len(reg), np.uint32) if epoch is None else epoch
        self.o.load(reg, free, hb, epoch, queue, log)

    def read_state(self, with_log=True):
        return self.o.export()

    def tick(self, now, tte, ev_kind=(), ev_slot=(), ev_val=(), ev_ts=(), ev_seq=None, n_pending=0, pinned=False,
             compact=False):
        if ev_seq is None:
            ev_seq = np.full(len(ev_kind), -1, np.int64)
        if self.mode == "deque" and np.any(np.asarray(ev_kind) == EV_LEAVE):
            raise FaasbalError(-1, "event %d: leave on a deque context"
                               % int(np.nonzero(np.asarray(ev_kind) == EV_LEAVE)[0][0]))
        snap = self.o.export() if self.mode != "deque" else None
        try:
            out = self.o.tick(now, tte, ev_kind, ev_slot, ev_val, ev_ts, ev_seq, n_pending)
        except RuntimeError as e:
            if snap is None or "overflow" not in str(e):
                raise
            self.o.load(snap["reg"], snap["free"], snap["hb"], snap["epoch"], snap["queue"], snap["log"])
            raise FaasbalError(FB_ENOSPC, "in-flight log full (model double)")
        out["result"] = dict(n_assigned=len(out["assign"]), n_orphans=len(out["orphans"]),
                             log_head=self.o.export()["head"])
        return out

    def purge(self, now, tte):
        out = self.o.tick(now, tte, [], [], [], [], np.zeros(0, np.int64), 0, dispatch_limit=0)
        out["result"] = dict(n_assigned=0, n_orphans=len(out["orphans"]), log_head=self.o.export()["head"])
        return out
