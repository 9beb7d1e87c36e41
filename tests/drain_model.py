"""One tick with the planned-shutdown message (FB_EV_DRAIN) -- TEST ONLY.

The leave model (tests/leave_model.py) with one more branch in its message handling.  The C
oracle follows the reference, which knows no drain; tests/test_drain_model.py pins this
model to it wherever the two can be compared.

The rule for one drain at clock ts from slot s (include/faasbal.h); val != 0
drains, val == 0 resumes, seq is ignored:

- Purge first.  The purge at ts runs before it, as before every message.
- s holds no record at that point: nothing happens.  No record is created and no reconnect
  is asked for; the evicted list keeps its rule (a touched slot without a record is listed).
- s holds a record that is not draining, val != 0: free = min(free, 2^29 - 1) - 2^30 and the
  slot is out of the LRU queue.  The record, heartbeat, epoch and in-flight entries stay; it
  is not a death and orphans nothing.
- s already draining, val != 0: nothing.
- val == 0 on a draining record: free += 2^30; if that is > 0 the slot goes to the LRU front
  as a reconnect(n > 0) puts it there.  On a record that is not draining: nothing.
- The status is 0 (applied) in every case.
- Nothing else knows the mark: a result's free += 1 never reaches 1, register and reconnect
  overwrite free (and so end the drain), expiry and leave delete the record as ever.
"""
import numpy as np

from faasbal._lib import FB_DRAIN_BELOW, FB_DRAIN_BIAS, FaasbalError
from leave_model import LeaveModel, LeaveModelBalancer
from oracle import DequeOracle

EV_DRAIN = 7
CLAMP = (1 << 29) - 1


def is_draining(free):
    return free < FB_DRAIN_BELOW


class DrainModel(LeaveModel):
    def _handle(self, kind, s, val, t, seq, head_in):
        if kind != EV_DRAIN:
            return super()._handle(kind, s, val, t, seq, head_in)
        if not self.reg[s]:
            return 0
        dr = is_draining(self.free[s])
        if val != 0:
            if not dr:
                self.free[s] = min(self.free[s], CLAMP) - FB_DRAIN_BIAS
                if s in self._inq:
                    self._inq.discard(s)
                    self.queue.remove(s)
        elif dr:
            self.free[s] += FB_DRAIN_BIAS
            if self.free[s] > 0:
                self._front(s)
        return 0


class DrainModelBalancer(LeaveModelBalancer):
    """TEST DOUBLE with OracleBalancer's call shape over the model above; deque contexts,
    which know no drain, over the C deque oracle."""

    def __init__(self, max_workers, max_log, max_events=0, device=0, mode="heartbeat", max_tokens=None):
        self.mode = mode
        self.o = DequeOracle(max_workers, max_log) if mode == "deque" else DrainModel(max_workers, max_log)

    def tick(self, now, tte, ev_kind=(), ev_slot=(), ev_val=(), ev_ts=(), ev_seq=None, n_pending=0, pinned=False,
             compact=False):
        k = np.asarray(ev_kind)
        if self.mode == "deque" and np.any(k == EV_DRAIN):
            raise FaasbalError(-1, "event %d: drain on a deque context" % int(np.nonzero(k == EV_DRAIN)[0][0]))
        return super().tick(now, tte, ev_kind, ev_slot, ev_val, ev_ts, ev_seq, n_pending)

    def draining(self):
        st = self.o.export()
        idx = np.nonzero(st["reg"].astype(bool) & (st["free"] < FB_DRAIN_BELOW))[0]
        return {"slot": idx.astype(np.int32), "free": st["free"][idx] + np.int32(FB_DRAIN_BIAS)}
