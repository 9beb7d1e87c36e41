"""numpy model of a rank's part of a shard group's reclaim (fb_log_reclaim_shard,
include/faasbal.h), shared by the CPU and GPU tests; ReclaimRank is the rank double that
carries it (tests/lcs_model.py's CompactRank with a reclaim_part).

A rank's state is a shard dict -- faasbal.sharded.split_state's or tests/shard_model.split's:
its slots [base, base + n), its log shard (log_slot: global slots, log_seq: the global
sequences, ascending) and the global head (``head`` or ``log_head``).

Let B = min(below_seq, head).  Local entry i is reclaimed iff log_seq[i] < B, it is live
(log_slot[i] is one of the rank's own slots, the slot holds a record and log_seq[i] >=
epoch[slot]: tests/lcs_model.live_mask) and its slot, rebased, is in the mask (None: every
slot).  log_slot[i] becomes -1; nothing else of the rank's state changes.  Merged over the
ranks that is tests/reclaim_model.reclaim_model on the global state.
"""
import numpy as np

from faasbal import _lib
from lcs_model import CompactRank, live_mask


def head_of(rs):
    return int(rs["head"] if "head" in rs else rs["log_head"])


def local_mask(rs, slots):
    """The rank's mask bytes from GLOBAL slots (None: no mask): those in its range, rebased."""
    if slots is None:
        return None
    m = np.zeros(max(int(rs["n"]), 1), np.uint8)
    idx = np.asarray(list(slots), np.int64).reshape(-1) - int(rs["base"])
    m[idx[(idx >= 0) & (idx < int(rs["n"]))]] = 1
    return m


def reclaim_part_model(rs, below_seq=None, mask=None):
    """(the rank's state after, seq, slot): the global sequences taken, ascending, and the
    global slot each was on.  ``mask``: None or the rank's n bytes, indexed locally."""
    head = head_of(rs)
    B = head if below_seq is None else min(int(below_seq), head)
    if B < 0:
        raise ValueError("below_seq < 0")
    slot = np.asarray(rs["log_slot"], np.int64)
    seq = np.asarray(rs["log_seq"], np.int64)
    take = live_mask(rs) & (seq < B)
    if mask is not None and len(slot):
        m = np.asarray(mask, np.uint8)
        take &= m[np.clip(slot - int(rs["base"]), 0, max(len(m) - 1, 0))] != 0
    out = dict(rs)
    new = np.asarray(rs["log_slot"]).copy()
    new[take] = -1
    out["log_slot"] = new
    return out, seq[take].astype(np.int64), slot[take].astype(np.int32)


def group_reclaim_model(shards, below_seq=None, slots=None):
    """(every rank's state after, the merged seq, the merged slot) of a group's reclaim."""
    outs = [reclaim_part_model(rs, below_seq, local_mask(rs, slots)) for rs in shards]
    seq = np.concatenate([o[1] for o in outs]) if outs else np.zeros(0, np.int64)
    slot = np.concatenate([o[2] for o in outs]) if outs else np.zeros(0, np.int32)
    order = np.argsort(seq, kind="stable")
    return [o[0] for o in outs], seq[order], slot[order]


class ReclaimRank(CompactRank):
    """TEST DOUBLE: the model rank with ShardedBalancer.reclaim_part.  Like the library's call
    it refuses while a tick is waited and not committed or a compaction is marked."""
    refuse_count = False  # the next count step refuses (injected)

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.reclaim_calls = []
        self._next = None

    def commit(self):
        super().commit()
        self._next = None

    def reclaim_part(self, below_seq=None, slots=None, count_only=False):
        self.reclaim_calls.append((below_seq, None if slots is None else sorted(int(s) for s in slots), bool(count_only)))
        if below_seq is not None and int(below_seq) < 0:
            raise _lib.FaasbalError(_lib.FB_EINVAL, "below_seq %d < 0" % below_seq)
        if count_only and self.refuse_count:
            self.refuse_count = False
            raise _lib.FaasbalError(_lib.FB_ESTATE, "fb_log_reclaim_shard between a tick's wait and its commit (injected)")
        if self.marked is not None:
            raise _lib.FaasbalError(_lib.FB_ESTATE, "a log compaction is marked: apply or cancel first")
        if self._next is not None:
            raise _lib.FaasbalError(_lib.FB_ESTATE, "fb_log_reclaim_shard between a tick's wait and its commit: fb_tick_commit first")
        new, seq, slot = reclaim_part_model(self.rs, below_seq, local_mask(self.rs, slots))
        if count_only:
            return {"n": len(seq), "seq": None, "slot": None}
        self.rs = new
        return {"n": len(seq), "seq": seq, "slot": slot}
