"""numpy model of fb_log_compact's rule (include/faasbal.h), shared by the CPU and GPU tests.

Entry q survives iff log[q] >= 0 and, on heartbeat contexts, its slot holds a record and
q >= epoch[slot].  Survivors keep their order; every slot's epoch becomes the number of
survivors below min(epoch, head).  Nothing else of the state changes."""
import numpy as np


def compact_model(st, deque=False):
    """(state after the compaction, kept) of a read_state()-style dict; kept[new] = old."""
    log = np.asarray(st["log"], np.int32)
    head = len(log)
    epoch = np.asarray(st["epoch"]).astype(np.int64)
    live = log >= 0
    if not deque:
        s = np.maximum(log, 0)
        live &= (np.asarray(st["reg"])[s] != 0) & (np.arange(head) >= epoch[s])
    below = np.concatenate([[0], np.cumsum(live)])  # survivors below q, q = 0 .. head
    kept = np.flatnonzero(live).astype(np.int64)
    out = dict(st)
    out.update(log=log[kept], epoch=below[np.minimum(epoch, head)].astype(np.uint32), head=len(kept))
    return out, kept


def host_compact(bal, deque=False):
    """The host path of GpuPushDispatcher.compact_log on a bare balancer: read the state,
    renumber with searchsorted, load it again.  Returns kept."""
    st = bal.read_state(with_log=True)
    log = st["log"]
    live = log >= 0
    if not deque:
        s = np.maximum(log, 0)
        live &= (st["reg"][s] != 0) & (np.arange(len(log)) >= st["epoch"][s].astype(np.int64))
    keep = np.flatnonzero(live).astype(np.int64)
    epoch = np.searchsorted(keep, st["epoch"].astype(np.int64), side="left").astype(np.uint32)
    bal.load_state(st["reg"], st["free"], st["hb"], epoch, st["queue"], log[keep])
    return keep
