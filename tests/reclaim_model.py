"""numpy model of fb_log_reclaim's rule (include/faasbal.h), shared by the CPU and GPU tests.

Let B = min(below_seq, head).  Entry q is reclaimed iff q < B, it is live by fb_log_compact's
rule (log[q] >= 0, its slot holds a record, q >= epoch[slot]) and its slot is in the mask (None:
every slot).  log[q] becomes -1 and the slot's in-flight count goes down by one; nothing else of
the state changes."""
import numpy as np


def live_entries(st):
    """Boolean array over the log: live by fb_log_compact's rule on a heartbeat context."""
    log = np.asarray(st["log"], np.int32)
    s = np.clip(log, 0, max(len(st["reg"]) - 1, 0))
    if not len(st["reg"]):
        return np.zeros(len(log), bool)
    return (log >= 0) & (log < len(st["reg"])) & (np.asarray(st["reg"])[s] != 0) & \
        (np.arange(len(log)) >= np.asarray(st["epoch"]).astype(np.int64)[s])


def inflight_model(st):
    """Per-slot count of live entries (what fb_read_inflight reports of this state)."""
    log = np.asarray(st["log"], np.int32)
    return np.bincount(log[live_entries(st)], minlength=len(st["reg"])).astype(np.uint32)


def reclaim_model(st, below_seq=None, mask=None):
    """(state after, seq, slot, per-slot drop) of a read_state()-style dict.  ``mask``: None or
    n_workers bytes (non-zero: the slot is taken from)."""
    log = np.asarray(st["log"], np.int32)
    head = len(log)
    B = head if below_seq is None else min(int(below_seq), head)
    if B < 0:
        raise ValueError("below_seq < 0")
    take = live_entries(st) & (np.arange(head) < B)
    if mask is not None:
        m = np.asarray(mask, np.uint8)
        take &= m[np.clip(log, 0, max(len(m) - 1, 0))] != 0 if len(m) else False
    seq = np.flatnonzero(take).astype(np.int64)
    slot = log[seq].astype(np.int32)
    out = dict(st)
    new_log = log.copy()
    new_log[seq] = -1
    out["log"] = new_log
    drop = np.bincount(slot, minlength=len(st["reg"])).astype(np.uint32)
    return out, seq, slot, drop


def slots_mask(n_workers, slots):
    m = np.zeros(n_workers, np.uint8)
    m[np.asarray(list(slots), np.int64)] = 1
    return m
