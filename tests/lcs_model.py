"""numpy model of a shard group's log compaction (fb_log_compact_shard_mark / _apply,
include/faasbal.h), per rank, shared by the CPU and GPU tests; CompactRank is the rank double
that carries it (tests/shard_model_balancer.py's model rank with the parts of a compaction).

A rank's state is tests/shard_model.split's dict: its slots [base, base + n), its log shard
(log_slot, and log_seq: the global sequences, ascending) and the global head.

mark:   bit q of the bitmap over [0, head) is set iff q is the sequence of one of the rank's
        entries and the entry is live -- log_slot >= 0, its slot holds a record and
        q >= epoch[slot] (tests/lc_model.compact_model's rule).  The bitmap is whole tiles of
        the head: 8 * LC_WORDS * cdiv(head, LC_TILE) bytes, bit q = bit q % 8 of byte q // 8.
apply:  against the ranks' union (the bytes summed: the sequences are disjoint, no byte
        carries): a live entry keeps its place in the shard and gets the number of set bits
        below its sequence; epoch[s] = set bits below min(epoch[s], head); head = the union's
        population, which must be the total the group agreed on.
"""
import threading

import numpy as np
import torch

from faasbal import _lib
from faasbal.sharded import InProcess, LocalShardGroup, rank_phases
from shard_model_balancer import ModelRankBalancer

LC_TILE, LC_WORDS = 2048, 32  # kLcTile, kLcWords (csrc/faasbal_layout.h)


def bitmap_bytes(head):
    return 8 * LC_WORDS * (-(-int(head) // LC_TILE))


def live_mask(rs):
    """The live entries of a rank's shard."""
    slot = np.asarray(rs["log_slot"], np.int64)
    seq = np.asarray(rs["log_seq"], np.int64)
    ls = np.clip(slot - rs["base"], 0, max(rs["n"] - 1, 0))
    if rs["n"] == 0:
        return np.zeros(len(slot), bool)
    own = (slot >= rs["base"]) & (slot < rs["base"] + rs["n"])
    return own & (np.asarray(rs["reg"])[ls] != 0) & (seq >= np.asarray(rs["epoch"]).astype(np.int64)[ls])


def mark_model(rs):
    """(the rank's bitmap as bytes, its live count)."""
    head = int(rs["head"])
    live = live_mask(rs)
    bits = np.zeros(bitmap_bytes(head) * 8, np.uint8)
    bits[np.asarray(rs["log_seq"], np.int64)[live]] = 1
    return np.packbits(bits, bitorder="little"), int(live.sum())


def apply_model(rs, reduced, total):
    """(the rank's state after the apply, the GLOBAL kept list) from the reduced bitmap;
    FB_ESTATE when its population is not ``total``."""
    head = int(rs["head"])
    bits = np.unpackbits(np.asarray(reduced, np.uint8), bitorder="little")
    assert len(bits) == bitmap_bytes(head) * 8
    if int(bits.sum()) != int(total) or bits[head:].any():
        raise _lib.FaasbalError(_lib.FB_ESTATE, "the reduced bitmap holds %d live entries, the group agreed on %d"
                                % (int(bits.sum()), int(total)))
    below = np.concatenate([[0], np.cumsum(bits[:head], dtype=np.int64)])  # set bits below q, q = 0 .. head
    live = live_mask(rs)
    seq = np.asarray(rs["log_seq"], np.int64)
    assert bits[seq[live]].all(), "a rank's own live bits are in the union"
    out = dict(rs)
    out.update(log_slot=np.asarray(rs["log_slot"])[live].copy(), log_seq=below[seq[live]],
               epoch=below[np.minimum(np.asarray(rs["epoch"]).astype(np.int64), head)].astype(np.asarray(rs["epoch"]).dtype),
               head=int(total))
    return out, np.flatnonzero(bits[:head]).astype(np.int64)


def group_model(shards):
    """Every rank's state after a group compaction and the kept list, from the ranks' states."""
    marks = [mark_model(rs) for rs in shards]
    union = np.sum([m for m, _ in marks], axis=0, dtype=np.int64).astype(np.uint8) if shards else np.zeros(0, np.uint8)
    total = sum(n for _, n in marks)
    outs = [apply_model(rs, union, total) for rs in shards]
    return [o for o, _ in outs], (outs[0][1] if outs else np.zeros(0, np.int64)), total


class CompactRank(ModelRankBalancer):
    """TEST DOUBLE: the model rank with ShardedBalancer's parts of a group compaction.  Like
    the library's mark it discards a tick that was waited for and never committed."""
    fail_mark = False   # the next mark raises (injected)
    marked = None

    def compact_bytes(self):
        return bitmap_bytes(self.rs["head"])

    def compact_exchange(self, zeroed=False):
        n = self.compact_bytes()
        buf = getattr(self, "_cbuf", None)
        if buf is None or buf.numel() != n:
            buf = self._cbuf = torch.zeros(n, dtype=torch.uint8)
        if zeroed:
            buf.zero_()
        return buf

    def compact_mark(self):
        if self.fail_mark:
            self.fail_mark = False
            raise _lib.FaasbalError(_lib.FB_EHIP, "mark failed (injected)")
        if self.marked is not None:
            raise _lib.FaasbalError(_lib.FB_ESTATE, "a log compaction is marked: apply or cancel first")
        self._next = None  # (an uncommitted tick is discarded)
        bits, live = mark_model(self.rs)
        self.compact_exchange().copy_(torch.from_numpy(bits))
        self.marked = live
        return live

    def compact_apply(self, total, want_kept=False):
        if self.marked is None:
            raise _lib.FaasbalError(_lib.FB_ESTATE, "fb_log_compact_shard_apply without fb_log_compact_shard_mark")
        live, self.marked = self.marked, None
        self.rs, kept = apply_model(self.rs, self.compact_exchange().numpy(), total)
        return {"n_kept": int(total), "n_kept_local": live, "kept": kept if want_kept else None}

    def compact_cancel(self):
        self.marked = None

    def tick(self, *a, **k):
        if self.marked is not None:
            raise _lib.FaasbalError(_lib.FB_ESTATE, "a log compaction is marked: apply or cancel first")
        return super().tick(*a, **k)


class ThreadedRanks(InProcess):
    """TEST DOUBLE's transport: in process, but a tick is every model rank's own tick() in a
    thread of its own, the exchange summed among them at a barrier (one all-reduce per tick)."""

    def phases(self, bals, op, kw):
        bar, xs, outs, bad = threading.Barrier(len(bals)), [], [None] * len(bals), []

        def allreduce(x):
            xs.append(x)
            if bar.wait() == 0:
                self.reduce(bals, xs)
            bar.wait()

        def run(i, b):
            outs[i] = rank_phases(b, op, kw, allreduce)
            if not outs[i][0]:
                bad.append(outs[i])  # (the first in time: the others' are the broken barrier)
                bar.abort()

        threads = [threading.Thread(target=run, args=(i, b)) for i, b in enumerate(bals)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        return bad[:1] * len(bals) or outs


class ModelGroup(LocalShardGroup):
    """TEST DOUBLE: a LocalShardGroup whose ranks are model ranks, over ThreadedRanks;
    everything else is LocalShardGroup's."""

    def __init__(self, world, n_workers, rank_cls=CompactRank):
        super().__init__(world, n_workers, 0, rank_factory=lambda r: rank_cls(r, world, n_workers))
        self.transport = ThreadedRanks(world)
