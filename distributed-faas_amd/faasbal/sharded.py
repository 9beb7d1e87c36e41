"""ShardedBalancer: one rank's share of a worker table split across GPUs.

The reference keeps every worker in one process (``self.workers`` dict and the
``free_workers`` OrderedDict, task_dispatcher.py:194, :327).  Here rank r of
``world`` owns the contiguous global slot range ``shard_range(W, world, r)``:
their records, their in-flight log entries and the dispatch of tasks to them.
The LRU queue order is replicated on every rank.  One tick is

    phase 1 (own slots: messages, purge, orphan flags, free counts)
    -> all-reduce(SUM) of a small uint8 exchange buffer over the ranks
    -> phase 2 (global water-filling from the exchanged counts; own writes)

and its whole-table result is bit-identical to the one-GPU tick.
The exchange buffer is a torch tensor so ``torch.distributed`` (RCCL over xGMI
on MI355X) can reduce it in place; the library runs on a torch stream that the
collective is issued on too, so kernels and collective are ordered on-device.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import functools
from collections import namedtuple

import numpy as np

from . import _lib
from .balancer import GpuBalancer, _arr, _p, draining_of
from ._lib import FB_ERERUN, FaasbalError
from .poolstats import HISTS, SCALARS, merge_summaries

MAX_RELAUNCH = 6  # FB_ERERUN: each relaunch at least doubles the round table
# a rank balancer's parts of a group compaction (ShardGroup.compact_log)
COMPACT_PARTS = ("compact_mark", "compact_exchange", "compact_apply", "compact_cancel")


def shard_range(n_workers, world, rank):
    """Global slot range [base, base + n) of ``rank``: contiguous blocks of ceil(W / world)."""
    per = -(-int(n_workers) // int(world))
    base = min(rank * per, n_workers)
    return base, min(per, n_workers - base)


def split_state(st, world, rank):
    """This rank's part of a global state dict (reg/free/hb/epoch/queue/log)."""
    W = len(st["reg"])
    base, n = shard_range(W, world, rank)
    log = np.asarray(st["log"], np.int32)
    seq = np.nonzero((log >= base) & (log < base + n))[0]
    epoch = st.get("epoch")
    epoch = np.zeros(W, np.uint32) if epoch is None else np.asarray(epoch, np.uint32)
    return dict(base=base, n=n, reg=np.asarray(st["reg"], np.uint8)[base:base + n],
                free=np.asarray(st["free"], np.int32)[base:base + n], hb=np.asarray(st["hb"], np.float64)[base:base + n],
                epoch=epoch[base:base + n], queue=np.asarray(st["queue"], np.int32), log_slot=log[seq],
                log_seq=seq.astype(np.uint32), log_head=len(log))


class ShardedBalancer(GpuBalancer):
    """Rank ``rank`` of ``world`` over a table of ``n_workers`` global slots."""

    def __init__(self, rank, world, n_workers, max_log, max_events=65536, device=0, lib_path=None):
        import torch  # the exchange buffer and the stream come from torch (plumbing, not compute)

        self.torch = torch
        self.rank, self.world, self.n_workers_global = int(rank), int(world), int(n_workers)
        self.base, self.n_local = shard_range(n_workers, world, rank)
        super().__init__(max(self.n_local, 1), max_log, max_events, device, lib_path)
        n = C.c_int64()
        self._chk(self.lib.fb_exchange_bytes(self.h, -1, C.byref(n)))
        self.xbuf = torch.zeros(n.value, dtype=torch.uint8, device="cuda:%d" % device)
        self._chk(self.lib.fb_bind_exchange(self.h, C.c_void_p(self.xbuf.data_ptr()), n.value))
        # kernels and the exchange collective share one torch stream (ordered, no host sync)
        self.stream = torch.cuda.Stream(device=device)
        self.set_stream(self.stream.cuda_stream)
        self._xbytes = 0

    def _create(self, max_workers, max_log, max_events, device):
        rc = self.lib.fb_create_sharded(C.byref(self.h), int(max_workers), self.n_workers_global, int(max_log),
                                        int(max_events), int(device), self.rank, self.world)
        if rc != 0:
            raise FaasbalError(rc, "fb_create_sharded(rank %d of %d, %d slots) failed"
                               % (self.rank, self.world, self.n_workers_global))

    # ----------------------------------------------------------------- state
    def load_state(self, *a, **k):
        raise FaasbalError(_lib.FB_ESTATE, "sharded context: use load() with the global state")

    # fb_log_compact refuses sharded contexts (sequence numbers are global across ranks)
    compact_log = None
    # fb_pool_stats too: a rank cannot answer for the group.  Its part is pool_stats_part;
    # ShardGroup.pool_stats gathers and merges the ranks' parts
    pool_stats = None
    # fb_log_reclaim as well (global sequences, and the bound is the group's).  Its part is
    # reclaim_part; ShardGroup.reclaim has every rank count before any rank takes and merges
    # the ranks' lists
    reclaim = None

    def reclaim_part(self, below_seq=None, slots=None, count_only=False):
        """fb_log_reclaim_shard: this rank's part of the group's reclaim -- every live entry
        of its log shard with a global sequence below ``below_seq`` (None: the head) on one of
        ``slots`` (GLOBAL slots, None: all; those outside this rank's range are another
        rank's and are dropped here) is completed on the device.  Returns dict(n, seq, slot):
        the global sequences (int64, ascending) and the global slot each was on (int32).
        ``count_only``: the call with outputs and no room -- dict(n, None, None), and nothing
        has changed; it makes every refusal the taking call would make.  Between ticks."""
        below = (1 << 62) if below_seq is None else int(below_seq)
        mask = None
        if slots is not None:
            mask = np.zeros(max(self.n_local, 1), np.uint8)
            idx = np.asarray(slots if isinstance(slots, np.ndarray) else list(slots), np.int64).reshape(-1) - self.base
            mask[idx[(idx >= 0) & (idx < self.n_local)]] = 1
        mp = None if mask is None else mask.ctypes.data_as(C.c_void_p)
        n = C.c_int64()
        cap = 0 if count_only else 256
        while True:
            seq = np.zeros(max(cap, 1), np.int64)
            slot = np.zeros(max(cap, 1), np.int32)
            n.value = -1
            rc = self.lib.fb_log_reclaim_shard(self.h, below, mp, seq.ctypes.data_as(C.c_void_p),
                                               slot.ctypes.data_as(C.c_void_p), cap, C.byref(n))
            if rc == _lib.FB_EINVAL and n.value > cap:  # nothing changed: the count, or come back with room
                if count_only:
                    return {"n": n.value, "seq": None, "slot": None}
                cap = n.value
                continue
            self._chk(rc)
            if count_only:
                return {"n": n.value, "seq": None, "slot": None}
            return {"n": n.value, "seq": seq[: n.value], "slot": slot[: n.value]}

    def pool_stats_part(self, now, tte, age_edges=()):
        """fb_pool_stats_shard: this rank's part of the group's pool summary as
        ``(dict, queue_len)`` -- the dict as ``GpuBalancer.pool_stats`` returns it, over this
        rank's slots, its log shard and the replicated queue's positions on its slots
        (``poolstats.merge_summaries`` folds the ranks' parts).  Reads only; between ticks."""
        edges = _arr(age_edges, np.float64).reshape(-1)
        out, qn = _lib.PoolSummary(), C.c_int64()
        self._chk(self.lib.fb_pool_stats_shard(self.h, float(now), float(tte), _p(edges), len(edges), C.byref(out),
                                               C.byref(qn)))
        d = {k: getattr(out, k) for k, _ in out._fields_[:-2]}
        d["free_hist"] = np.array(out.free_hist, np.int64)
        d["age_hist"] = np.array(out.age_hist, np.int64)
        return d, qn.value

    # ----------------------------------------------- the group's log compaction, this rank's parts
    def compact_bytes(self):
        """fb_log_compact_shard_bytes: the size of the live bitmap the ranks reduce (the same
        on every rank; 0 for an empty log)."""
        n = C.c_int64()
        self._chk(self.lib.fb_log_compact_shard_bytes(self.h, C.byref(n)))
        return n.value

    def compact_exchange(self, zeroed=False):
        """The bitmap to all-reduce (SUM over uint8): a view of a torch tensor kept between
        compactions and grown when the log needs more.  ``zeroed``: the view filled with zeros
        (a rank whose mark failed joins the reduction with nothing)."""
        n = self.compact_bytes()
        buf = getattr(self, "_cbuf", None)
        if buf is None or buf.numel() < n:
            buf = self._cbuf = self.torch.empty(max(2 * n, 4096), dtype=self.torch.uint8, device=self.xbuf.device)
        view = buf[:n]
        if zeroed:
            with self.torch.cuda.stream(self.stream):
                view.zero_()
        return view

    def compact_mark(self):
        """fb_log_compact_shard_mark: this rank's live bits into ``compact_exchange()``;
        returns its live count.  An uncommitted tick is discarded."""
        view = self.compact_exchange()
        live = C.c_int64()
        self._chk(self.lib.fb_log_compact_shard_mark(self.h, C.c_void_p(self._cbuf.data_ptr()), view.numel(),
                                                     C.byref(live)))
        return live.value

    def compact_apply(self, total, want_kept=False):
        """fb_log_compact_shard_apply after the reduction: ``total`` is the sum of the ranks'
        live counts.  Returns dict(n_kept, n_kept_local, kept): ``kept`` the GLOBAL kept list
        (``kept[new] = old``) with ``want_kept``, else None."""
        n = C.c_int64()
        kept = np.zeros(max(int(total), 1), np.int64) if want_kept else None
        self._chk(self.lib.fb_log_compact_shard_apply(self.h, int(total), None if kept is None else
                                                      kept.ctypes.data_as(C.c_void_p), int(total), C.byref(n)))
        return {"n_kept": int(total), "n_kept_local": n.value, "kept": None if kept is None else kept[: int(total)]}

    def compact_cancel(self):
        """fb_log_compact_shard_cancel: drop a mark (nothing has changed)."""
        self._chk(self.lib.fb_log_compact_shard_cancel(self.h))

    def load(self, st):
        """Load this rank's part of a global state dict."""
        sh = split_state(st, self.world, self.rank)
        self._chk(self.lib.fb_load_shard(self.h, sh["base"], sh["n"], _p(sh["reg"]), _p(sh["free"]), _p(sh["hb"]),
                                         _p(sh["epoch"]), _p(sh["queue"]), len(sh["queue"]), _p(sh["log_slot"]),
                                         _p(sh["log_seq"]), len(sh["log_slot"]), sh["log_head"]))
        # the round table of the first tick from the GLOBAL max free count (every rank
        # computes it from the same global state, so the exchange layouts agree)
        q = np.asarray(st["queue"], np.int64)
        mf = int(np.asarray(st["free"])[q].max()) if len(q) else 1
        self._chk(self.lib.fb_set_round_hint(self.h, max(1, min(mf, 1 << 30))))
        self.n_workers = sh["n"]

    def read_state(self, with_log=True):
        out = super().read_state(with_log)
        n, head = C.c_int64(), C.c_int64()
        seq = np.zeros(max(len(out.get("log", ())), 1), np.uint32)
        self._chk(self.lib.fb_read_shard_log(self.h, _p(seq) if with_log else None, C.byref(n), C.byref(head)))
        out["head"] = head.value
        out["log_len"] = n.value
        if with_log:
            out["log_seq"] = seq[: n.value]
        out["base"] = self.base
        return out

    def draining(self):
        """This rank's draining workers (``GpuBalancer.draining``), slots global."""
        return draining_of(self.read_state(with_log=False), self.base)

    # ----------------------------------------------------------------- ticks
    def launch(self, *a, **k):
        """Phase 1.  Afterwards all-reduce ``exchange()`` (SUM) over the ranks, then ``cont()``."""
        super().launch(*a, **k)
        self._launched()

    def purge_launch(self, now, tte):
        """Phase 1 of this rank's share of a purge: no events, nothing dispatched; the
        exchange and ``cont()`` follow as for a tick."""
        self._E = 0
        self._chk(self.lib.fb_purge_launch(self.h, float(now), float(tte)))
        self._launched()

    def _launched(self):
        # the launch's exchange size, asked once: exchange() is a view of that many bytes
        n = C.c_int64()
        self._chk(self.lib.fb_exchange_bytes(self.h, self._E, C.byref(n)))
        self._xbytes = n.value

    def exchange(self):
        """The tick's exchange region (a view of the bound torch tensor, kept while its size is)."""
        xv = getattr(self, "_xview", None)
        if xv is None or xv.numel() != self._xbytes:
            xv = self._xview = self.xbuf[: self._xbytes]
        return xv

    def cont(self):
        self._chk(self.lib.fb_tick_continue(self.h))

    def set_full_assign(self, on=True):
        """fb_set_full_assign: this rank's phase 2 also writes the whole tick's task -> slot
        array (assignments() then works here; the dispatcher's rank gathers no tasks)."""
        self._chk(self.lib.fb_set_full_assign(self.h, 1 if on else 0))
        self.full_assign = bool(on)

    def assignments(self, first=0, n=None):
        if not getattr(self, "full_assign", False):
            raise FaasbalError(_lib.FB_ESTATE, "sharded context: use local_assignments() (or set_full_assign)")
        return super().assignments(first, n)

    def tick_outputs(self, res):
        """A waited tick's outputs: the whole tick's assignments where this rank writes them
        (set_full_assign), else this rank's own (task, slot) pairs."""
        out = dict(result=res)
        if getattr(self, "full_assign", False):
            out.update(assign=self.assignments())
        else:
            task, slot = self.local_assignments()
            out.update(task=task, slot=slot)
        out.update(reconnect=self.event_status(), orphans=self.orphans(), evicted=self.evicted())
        return out

    def purge_outputs(self, res):
        return dict(result=res, evicted=self.evicted(), orphans=self.orphans())

    def purge(self, now, tte, commit=True, allreduce=None):
        """This rank's share of ``purge_workers`` (``task_dispatcher.py:241-249``):
        the exchange and phase 2 run as for a tick, nothing is dispatched; returns
        dict(result, evicted, orphans) of this rank's slots and log shard."""
        res = run_phases([self], lambda b: b.purge_launch(now, tte), functools.partial(dist_reduce, allreduce=allreduce))
        out = self.purge_outputs(res[0])
        if commit:
            self.commit()
        return out

    def tick(self, now, tte, ev_kind=(), ev_slot=(), ev_val=(), ev_ts=(), ev_seq=None, n_pending=0,
             commit=True, outputs=True, allreduce=None):
        """One sharded tick; ``allreduce(tensor)`` defaults to torch.distributed.all_reduce (SUM)."""
        res = run_phases([self], lambda b: b.launch(now, tte, ev_kind, ev_slot, ev_val, ev_ts, ev_seq, n_pending),
                         functools.partial(dist_reduce, allreduce=allreduce))
        out = self.tick_outputs(res[0]) if outputs else dict(result=res[0])
        if commit:
            self.commit()
        return out


def run_phases(bals, launch, reduce):
    """A tick or purge on the ranks this process holds: phase 1 on each (``launch(rank)``),
    the exchanges summed over the group (``reduce(ranks, tensors)``), phase 2 and the wait --
    again with a wider round table while the tick asks for it (FB_ERERUN: the same tick,
    relaunched; every rank gets the same answer, so the ranks' collectives stay matched).
    Every rank waits even after one failed (a rerun request reaches them all).  Returns the
    ranks' results, nothing committed; raises the first rank's failure."""
    for attempt in range(MAX_RELAUNCH + 1):
        for b in bals:
            launch(b)
        reduce(bals, [b.exchange() for b in bals])
        for b in bals:
            b.cont()
        res, err = [], None
        for b in bals:
            try:
                res.append(b.wait())
            except FaasbalError as e:
                err = err or e
        if err is None:
            return res
        if err.code != FB_ERERUN or attempt == MAX_RELAUNCH:
            raise err


def dist_reduce(bals, xs, allreduce=None):
    """torch.distributed's SUM, in place, of each held rank's uint8 tensor -- or the caller's
    ``allreduce(tensor)`` --, issued on the rank's stream where it has one: the explicit wait
    orders what follows after it on that stream (RCCL) or after its completion (gloo)."""
    for b, x in zip(bals, xs):
        stream = getattr(b, "stream", None)
        with (b.torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
            if allreduce is None:
                import torch.distributed as dist
                dist.all_reduce(x, async_op=True).wait()
            else:
                allreduce(x)


def merge_states(states, n_workers):
    """The global state (GpuBalancer.read_state layout) from every rank's read_state()."""
    reg = np.zeros(n_workers, np.uint8)
    free = np.zeros(n_workers, np.int32)
    hb = np.zeros(n_workers, np.float64)
    epoch = np.zeros(n_workers, np.uint32)
    for st in states:
        lo, n = st["base"], len(st["reg"])
        reg[lo:lo + n], free[lo:lo + n], hb[lo:lo + n], epoch[lo:lo + n] = st["reg"], st["free"], st["hb"], st["epoch"]
    head = states[0]["head"]
    out = dict(reg=reg, free=free, hb=hb, epoch=epoch, queue=np.asarray(states[0]["queue"], np.int32), head=head)
    if all("log" in st for st in states):
        log = np.full(head, -1, np.int32)
        for st in states:
            log[np.asarray(st["log_seq"], np.int64)] = st["log"]
        out["log"] = log
    return out


class ShardGroup:
    """A worker table sharded over ranks, behind GpuBalancer's tick API -- what
    GpuPushDispatcher drives (``balancer=``), so the drop-in's host loop, message
    flow and Redis I/O are the same for one GPU and for N.  Subclasses say which ranks
    this process holds and how they meet the others (the transport): all of them, in this
    process (LocalShardGroup), or rank 0 of a torch.distributed group (DistShardGroup)."""

    mode = "heartbeat"

    def __init__(self, n_workers, rank_balancers, transport):
        self.n_workers_global = int(n_workers)
        self.bals, self.transport = list(rank_balancers), transport
        # rank balancers (those this process holds) without a part of the summary, such as
        # test doubles: no device summary, and GpuPushDispatcher.pool_stats reads the state
        if not all(callable(getattr(b, "pool_stats_part", None)) for b in rank_balancers):
            self.pool_stats = None
        # ... or without the parts of a compaction: GpuPushDispatcher.compact_log takes its host path
        if not all(callable(getattr(b, m, None)) for b in rank_balancers for m in COMPACT_PARTS):
            self.compact_log = None
        # ... or without a part of a reclaim: GpuPushDispatcher refuses task_timeout over the group
        if not all(callable(getattr(b, "reclaim_part", None)) for b in rank_balancers):
            self.reclaim = None

    def _each(self, op, **kw):  # -> list of per-rank results, rank order
        self.transport.announce(op, kw)
        outs, bad = _OPS[op].run(self.transport, self.bals, op, kw)
        if bad is not None:
            code, msg = bad
            if code is None:
                raise RuntimeError("shard operation %r failed on a rank: %s" % (op, msg))
            raise FaasbalError(code, "shard operation %r failed on a rank: %s" % (op, msg))
        return outs

    def pool_stats(self, now, tte, age_edges=()):
        """The group's pool summary (``GpuBalancer.pool_stats``' dict): every rank's part,
        computed where its shard lives, merged here.  ``inflight_max`` is -1: sharded
        contexts keep no per-slot counts."""
        edges = np.asarray(age_edges, np.float64).reshape(-1)
        parts = self._each("stats", now=float(now), tte=float(tte), age_edges=edges)
        out = merge_summaries([p for p, _ in parts], [q for _, q in parts])
        if out["n_slots"] != self.n_workers_global:
            raise FaasbalError(_lib.FB_ESTATE, "the ranks' parts cover %d slots, the table has %d"
                               % (out["n_slots"], self.n_workers_global))
        return out

    def compact_log(self, expect=None, want_kept=True):
        """The group's in-flight log renumbered densely where the shards live
        (``GpuBalancer.compact_log``'s contract: dict(n_kept, kept), ``kept[new] = old``
        global sequence, or None without ``want_kept``): every rank marks its live bits, the
        bitmaps are all-reduced, every rank renumbers its shard against the union and remaps
        its epochs; the dispatcher's rank reads the kept list off the bitmap.  Everything else
        of the state and the ranks' tick pipelines stay.  ``expect``: the live count the
        caller's mirror holds -- FB_ESTATE, every rank cancelled and every shard as it was
        when the group's total differs, or when a rank could not mark."""
        out = self._each("compact", expect=-1 if expect is None else int(expect), want_kept=bool(want_kept))[0]
        return {"n_kept": out["n_kept"], "kept": out["kept"]}

    def reclaim(self, below_seq=None, slots=None):
        """Take live log entries back from workers that stay registered, where the shards
        live (``GpuBalancer.reclaim``'s contract: dict(n, seq, slot), ``seq`` int64 ascending
        across the whole group, ``slot`` the global slot each was on, int32; ``slots`` global,
        None: all).  A reclaim renumbers nothing, so each rank decides about its own entries
        and the device needs no collective; the group's part is agreement -- every rank
        counts first, which is every refusal it would make, and only when all of them can do
        the ranks take: a rank that refuses (FB_ESTATE: a tick not committed there, staged
        events, a marked compaction) leaves every shard as it was, and its code is raised.
        The ranks' lists are merged by sequence (they are disjoint).  Between ticks."""
        idx = None
        if slots is not None:
            idx = np.asarray(slots if isinstance(slots, np.ndarray) else list(slots), np.int64).reshape(-1)
            if len(idx) and (idx.min() < 0 or idx.max() >= self.n_workers_global):
                raise ValueError("slots outside [0, %d)" % self.n_workers_global)
            idx = idx.astype(np.int32)
        parts = self._each("reclaim", below_seq=(1 << 62) if below_seq is None else int(below_seq), slots=idx)
        return merge_reclaimed(parts)

    def load_state(self, reg, free, hb, epoch=None, queue=(), log=()):
        W = len(reg)
        st = dict(reg=np.asarray(reg, np.uint8), free=np.asarray(free, np.int32), hb=np.asarray(hb, np.float64),
                  epoch=np.zeros(W, np.uint32) if epoch is None else np.asarray(epoch, np.uint32),
                  queue=np.asarray(queue, np.int32), log=np.asarray(log, np.int32))
        self._each("load", st=st)

    def load(self, st):
        self.load_state(st["reg"], st["free"], st["hb"], st.get("epoch"), st["queue"], st["log"])

    def read_state(self, with_log=True):
        return merge_states(self._each("read", with_log=with_log), self.n_workers_global)

    def draining(self):
        """The group's draining workers (``GpuBalancer.draining``'s dict, slots global): every
        rank's own, from its state read without the log, merged in rank order."""
        parts = [draining_of(st, st["base"]) for st in self._each("read", with_log=False)]
        return {k: np.concatenate([p[k] for p in parts]).astype(np.int32) for k in ("slot", "free")}

    def tick(self, now, tte, ev_kind=(), ev_slot=(), ev_val=(), ev_ts=(), ev_seq=None, n_pending=0):
        k = np.asarray(ev_kind, np.uint8)
        ev = dict(ev_kind=k, ev_slot=np.asarray(ev_slot, np.int32), ev_val=np.asarray(ev_val, np.int32),
                  ev_ts=np.asarray(ev_ts, np.float64),
                  ev_seq=np.full(len(k), -1, np.int64) if ev_seq is None else np.asarray(ev_seq, np.int64))
        outs = self._each("tick", now=float(now), tte=float(tte), n_pending=int(n_pending), **ev)
        res = dict(outs[0]["result"])
        for key in ("n_local", "n_orphans_local"):
            res[key] = sum(int(o["result"][key]) for o in outs)
        res["n_evicted"] = sum(int(o["result"]["n_evicted"]) for o in outs)
        merged = merge_outputs(outs, int(res["n_assigned"]))
        merged["result"] = res
        return merged

    def purge(self, now, tte):
        outs = self._each("purge", now=float(now), tte=float(tte))
        res = dict(outs[0]["result"])
        res["n_evicted"] = sum(int(o["result"]["n_evicted"]) for o in outs)
        return dict(result=res, evicted=np.sort(np.concatenate([o["evicted"] for o in outs])).astype(np.int32),
                    orphans=np.sort(np.concatenate([o["orphans"] for o in outs])).astype(np.int64))

    def close(self):
        pass


def merge_reclaimed(parts):
    """The group's dict(n, seq, slot) from the ranks' reclaim_part results: one list ascending
    by sequence (the ranks' sequences are disjoint, each rank's ascending already)."""
    seq = np.concatenate([np.asarray(p["seq"], np.int64) for p in parts]) if parts else np.zeros(0, np.int64)
    slot = np.concatenate([np.asarray(p["slot"], np.int32) for p in parts]) if parts else np.zeros(0, np.int32)
    order = np.argsort(seq, kind="stable")
    return {"n": int(len(seq)), "seq": seq[order], "slot": slot[order]}


# ------------------------------------------------------------------ the group's protocols
# Every process of a group runs the same function for an operation -- rank 0's group,
# serve_shard on the other ranks, the group that holds every rank -- over the ranks it holds
# (``bals``) and a transport that says how those meet the others.  Each returns (the per-rank
# results in rank order where rank 0 is held, else None; the first failure or None).

def _guarded(f, *a, **k):
    """f's value as (True, value), its failure as (False, (code, message)) instead of raised:
    every rank must still reach the group's next collective, and the group raises the failure
    once every rank has answered."""
    try:
        return (True, f(*a, **k))
    except Exception as e:  # noqa: BLE001
        return (False, (getattr(e, "code", None), "%s: %s" % (type(e).__name__, e)))


def _first_bad(flags):
    return next((f[1] for f in flags if not f[0]), None)


def _call(tp, bals, op, kw):
    """A plain call (load, read, stats) on every rank, the parts brought together."""
    outs = tp.agree([_guarded(_OPS[op].call, b, kw) for b in bals], _OPS[op].reply)
    bad = _first_bad(outs)
    return (None, bad) if bad is not None else ([o[1] for o in outs], None)


def serve_op(bal, op, kw, allreduce=None, commit=True):
    """One group operation as the rank balancer's own call (``_OPS[op].call``), raised, not
    guarded.  ``commit=False`` leaves a tick / purge waited but uncommitted."""
    call = _OPS[op].call
    return call(bal, kw, allreduce=allreduce, commit=commit) if _OPS[op].run is _tick else call(bal, kw)


def rank_phases(bal, op, kw, allreduce=None):
    """A rank's own tick / purge, waited and not committed, guarded."""
    return _guarded(serve_op, bal, op, kw, allreduce, False)


def _tick(tp, bals, op, kw):
    """A tick or purge: the phases on the held ranks (run_phases), one header per rank
    agreed on, and only when every rank succeeded the commit -- so the shards never diverge
    -- and the ranks' lists to the group's caller."""
    outs = tp.phases(bals, op, kw)
    heads = tp.agree(outs, _TICK_HEAD)
    bad = _first_bad(heads)
    if bad is not None:
        return None, bad
    for b in bals:
        b.commit()
    return tp.collect([o[1] for o in outs], [h[1] for h in heads], _TICK_LISTS), None


def _compact_verdict(marks, expect):
    """(the group's live count, the first failure or None) from every rank's guarded mark."""
    bad = _first_bad(marks)
    total = sum(int(m[1]) for m in marks if m[0])
    if bad is None and expect >= 0 and expect != total:
        bad = (_lib.FB_ESTATE, "the group's log holds %d live entries, the caller expected %d" % (total, expect))
    return total, bad


def _compact(tp, bals, op, kw):
    """A group compaction: mark, the bitmaps reduced -- a rank whose mark failed joins with
    zeros of the agreed size, so that no rank blocks in the collective --, the ranks' ok
    flags and live counts agreed on, then every rank applies (rank 0 asks for the kept list)
    and they agree again, or every rank cancels: nothing has changed anywhere."""
    marks = [_guarded(b.compact_mark) for b in bals]
    xs = [b.compact_exchange(zeroed=not m[0]) for b, m in zip(bals, marks)]
    if xs[0].numel():
        tp.reduce(bals, xs)
    total, bad = _compact_verdict(tp.agree(marks, _WORD), kw["expect"])
    if bad is None:
        done = [_guarded(b.compact_apply, total, bool(kw["want_kept"]) and r == 0) for r, b in zip(tp.ranks, bals)]
        # (the count gives every rank the same verdict; what is left is a rank's own runtime error)
        bad = _first_bad(tp.agree([(ok, 0 if ok else v) for ok, v in done], _WORD))
    if bad is not None:
        for b in bals:
            b.compact_cancel()
        return None, bad
    return [d[1] for d in done], None


def _reclaim(tp, bals, op, kw):
    """A group reclaim: every rank counts -- every refusal it would make, with nothing changed
    anywhere -- and the counts are agreed on; only when all of them can do the ranks take, and
    agree again (a take that fails now, or takes another number than it counted, is the rank's
    own runtime error); then the lists to the group's caller."""
    args = (kw["below_seq"], kw["slots"])
    counts = tp.agree([_guarded(lambda b: b.reclaim_part(*args, True)["n"], b) for b in bals], _WORD)
    bad = _first_bad(counts)
    if bad is not None:
        return None, bad
    done = [_guarded(b.reclaim_part, *args) for b in bals]
    for i, r in enumerate(tp.ranks):
        if done[i][0] and done[i][1]["n"] != counts[r][1]:
            done[i] = (False, (_lib.FB_ESTATE, "rank %d counted %d entries to reclaim and took %d"
                               % (r, counts[r][1], done[i][1]["n"])))
    bad = _first_bad(tp.agree([(ok, 0 if ok else v) for ok, v in done], _WORD))
    if bad is not None:
        return None, bad
    return tp.collect([d[1] for d in done], [c[1] for c in counts], _RECLAIM_LISTS), None


# ------------------------------------------------------------------ the wire format
# A call is a fixed header of _HDR int64 words broadcast from rank 0 -- the operation's code,
# then the words its _OPS entry states (clocks as bit patterns) -- and the entry's payload
# tensor when it has elements.  What comes back is the protocol's: fixed records all-gathered
# (agree), byte lists gathered to rank 0 (collect), the exchange all-reduced in place (reduce).
# Loads and state reads (not per tick) travel pickled both ways, and so do failure messages.
_HDR = 8  # int64 words of the call header / the per-rank result header
_PS_WORDS = C.sizeof(_lib.PoolSummary) // 8  # fb_pool_summary's words (SCALARS' order, then HISTS')
_PS_REC = 3 + _PS_WORDS
_PS_DOUBLES = ("oldest_hb", "newest_hb")
_PICKLED = "pickled"
_TICK_ARGS = ("now", "tte", "ev_kind", "ev_slot", "ev_val", "ev_ts", "ev_seq", "n_pending")


def _bits(x):
    return int(np.float64(x).view(np.int64))


def _real(w):
    return float(np.int64(w).view(np.float64))


def _pack_summary(part, queue_len):
    """A part as the stats record's words (ok = 1, code = 0)."""
    w = [np.float64(part[k]).view(np.int64) if k in _PS_DOUBLES else np.int64(part[k]) for k in SCALARS]
    return np.concatenate([np.array([1, 0, int(queue_len)], np.int64), np.array(w, np.int64)]
                          + [np.asarray(part[k], np.int64) for k in HISTS])


def _unpack_summary(rec):
    """(part, queue_len) of an ok stats record."""
    rec = np.ascontiguousarray(rec, np.int64)
    body, n = rec[3:], len(SCALARS)
    part = {k: float(body[i:i + 1].view(np.float64)[0]) if k in _PS_DOUBLES else int(body[i])
            for i, k in enumerate(SCALARS)}
    part["free_hist"] = body[n:n + _lib.PS_FREE_BINS].copy()
    part["age_hist"] = body[n + _lib.PS_FREE_BINS:].copy()
    return part, int(rec[2])


def _pack_events(kw):
    """A tick's event batch as one byte array, 25 B per message."""
    k = np.ascontiguousarray(kw["ev_kind"], np.uint8)
    parts = [k.view(np.uint8), np.ascontiguousarray(kw["ev_slot"], np.int32).view(np.uint8),
             np.ascontiguousarray(kw["ev_val"], np.int32).view(np.uint8),
             np.ascontiguousarray(kw["ev_ts"], np.float64).view(np.uint8),
             np.ascontiguousarray(kw["ev_seq"], np.int64).view(np.uint8)]
    return np.concatenate(parts) if len(k) else np.zeros(0, np.uint8)


def _unpack_events(buf, E):
    o = [0, E, 5 * E, 9 * E, 17 * E, 25 * E]
    return dict(ev_kind=buf[o[0]:o[1]].copy(), ev_slot=buf[o[1]:o[2]].view(np.int32).copy(),
                ev_val=buf[o[2]:o[3]].view(np.int32).copy(), ev_ts=buf[o[3]:o[4]].view(np.float64).copy(),
                ev_seq=buf[o[4]:o[5]].view(np.int64).copy())


# what agree() carries per rank: ok, a code, then ``pack(value)`` in a record of ``width`` words
_Record = namedtuple("_Record", "width pack unpack")
_WORD = _Record(_HDR, lambda n: (int(n),), lambda w: int(w[0]))  # a count
_STATS = _Record(_PS_REC, lambda v: _pack_summary(*v)[2:], lambda w: _unpack_summary(np.concatenate([[1, 0], w])))
# a tick's / purge's result: the rank's counts, then the lengths of its lists (no tasks travel:
# rank 0 writes the whole assignment array itself, fb_set_full_assign)
_TICK_HEAD = _Record(_HDR, lambda out: (int(out["result"].get("n_local", 0)), int(out["result"].get("n_orphans_local", 0)),
                                        int(out["result"]["n_evicted"]), 0, len(out["orphans"]), len(out["evicted"])),
                     lambda w: w.copy())

# what collect() carries per rank: ``nbytes(agreed value)`` bytes of ``pack(value)``
_Lists = namedtuple("_Lists", "nbytes pack unpack")
_TICK_LISTS = _Lists(  # the orphans (int64), then the evicted slots (int32): a few KB
    lambda h: 8 * int(h[4]) + 4 * int(h[5]),
    lambda out: np.concatenate([np.ascontiguousarray(out["orphans"], np.int64).view(np.uint8),
                                np.ascontiguousarray(out["evicted"], np.int32).view(np.uint8)]),
    lambda h, b: dict(result=dict(n_local=int(h[0]), n_orphans_local=int(h[1]), n_evicted=int(h[2])),
                      orphans=b[:8 * int(h[4])].view(np.int64).copy(),
                      evicted=b[8 * int(h[4]):8 * int(h[4]) + 4 * int(h[5])].view(np.int32).copy(), reconnect=None))
_RECLAIM_LISTS = _Lists(  # 12 bytes per entry: the sequences (int64), then the slots (int32)
    lambda n: 12 * n,
    lambda part: np.concatenate([np.ascontiguousarray(part["seq"], np.int64).view(np.uint8),
                                 np.ascontiguousarray(part["slot"], np.int32).view(np.uint8)]),
    lambda n, b: dict(n=n, seq=b[:8 * n].view(np.int64).copy(), slot=b[8 * n:12 * n].view(np.int32).copy()))


class _Op:
    """One group operation.  ``head(kw)``: the call header's words 1..; ``payload``: None,
    _PICKLED (kw travels pickled) or (dtype, its element count from the header, its elements
    from kw); ``kw(header, payload)``: the receiver's kw; ``run``: the protocol; ``call``: the
    rank balancer's own call; ``reply``: a plain call's record (None: pickled); ``launch`` /
    ``outputs``: a tick's or purge's phase 1 and outputs, for run_phases."""

    def __init__(self, code, run=None, head=lambda kw: (), payload=None, kw=lambda h, p: {}, call=None, reply=None,
                 launch=None, outputs=None):
        self.code, self.run, self.head, self.payload, self.kw, self.call = code, run, head, payload, kw, call
        self.reply, self.launch, self.outputs = reply, launch, outputs


_OPS = {
    "tick": _Op(1, _tick,
                head=lambda kw: (len(kw["ev_kind"]), kw["n_pending"], _bits(kw["now"]), _bits(kw["tte"])),
                payload=(np.uint8, lambda h: 25 * h[1], _pack_events),
                kw=lambda h, p: dict(now=_real(h[3]), tte=_real(h[4]), n_pending=int(h[2]), **_unpack_events(p, int(h[1]))),
                call=lambda b, kw, **how: b.tick(*[kw[k] for k in _TICK_ARGS], **how),
                launch=lambda b, kw: b.launch(*[kw[k] for k in _TICK_ARGS]),
                outputs=lambda b, res: b.tick_outputs(res)),
    "purge": _Op(2, _tick,
                 head=lambda kw: (0, 0, _bits(kw["now"]), _bits(kw["tte"])),
                 kw=lambda h, p: dict(now=_real(h[3]), tte=_real(h[4])),
                 call=lambda b, kw, **how: b.purge(kw["now"], kw["tte"], **how),
                 launch=lambda b, kw: b.purge_launch(kw["now"], kw["tte"]),
                 outputs=lambda b, res: b.purge_outputs(res)),
    "load": _Op(3, _call, payload=_PICKLED, call=lambda b, kw: b.load(kw["st"])),
    "read": _Op(4, _call, payload=_PICKLED, call=lambda b, kw: b.read_state(with_log=kw["with_log"])),
    "stop": _Op(5),  # (the header is the whole call; serve_shard returns)
    "stats": _Op(6, _call,  # (reads only: nothing to commit)
                 head=lambda kw: (len(kw["age_edges"]), 0, _bits(kw["now"]), _bits(kw["tte"])),
                 payload=(np.float64, lambda h: h[1], lambda kw: kw["age_edges"]),
                 kw=lambda h, p: dict(now=_real(h[3]), tte=_real(h[4]), age_edges=p),
                 call=lambda b, kw: b.pool_stats_part(kw["now"], kw["tte"], kw["age_edges"]), reply=_STATS),
    "compact": _Op(7, _compact,  # (the header is the whole call; -1: no expected count)
                   head=lambda kw: (kw["expect"], 1 if kw["want_kept"] else 0),
                   kw=lambda h, p: dict(expect=int(h[1]), want_kept=bool(h[2]))),
    "reclaim": _Op(8, _reclaim,  # (-1 slots: no mask)
                   head=lambda kw: (kw["below_seq"], -1 if kw["slots"] is None else len(kw["slots"])),
                   payload=(np.int32, lambda h: h[2], lambda kw: kw["slots"]),
                   kw=lambda h, p: dict(below_seq=int(h[1]), slots=None if h[2] < 0 else p)),
}
_OP_NAMES = {spec.code: op for op, spec in _OPS.items()}


def _dev(dist):
    import torch
    return torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")


def _send_call(dist, dev, op, kw):
    """Rank 0: the call to every rank.  Returns nothing; the ranks read it with _recv_call."""
    import torch
    spec = _OPS[op]
    h = np.zeros(_HDR, np.int64)
    words = (spec.code,) + tuple(spec.head(kw))
    h[:len(words)] = words
    dist.broadcast(torch.from_numpy(h).to(dev), src=0)
    if spec.payload == _PICKLED:
        dist.broadcast_object_list([kw], src=0)
    elif spec.payload is not None and spec.payload[1](h) > 0:
        dist.broadcast(torch.from_numpy(np.ascontiguousarray(spec.payload[2](kw), spec.payload[0])).to(dev), src=0)


def _recv_call(dist, dev):
    """Ranks > 0: the next call of rank 0 as (op, kw)."""
    import torch
    h = torch.zeros(_HDR, dtype=torch.int64, device=dev)
    dist.broadcast(h, src=0)
    h = h.cpu().numpy()
    op = _OP_NAMES[int(h[0])]
    spec, p = _OPS[op], None
    if spec.payload == _PICKLED:
        box = [None]
        dist.broadcast_object_list(box, src=0)
        return op, box[0]
    if spec.payload is not None:
        p = torch.from_numpy(np.zeros(max(int(spec.payload[1](h)), 0), spec.payload[0])).to(dev)
        if p.numel():
            dist.broadcast(p, src=0)
        p = p.cpu().numpy()
    return op, spec.kw(h, p)


# ------------------------------------------------------------------ the transports
class InProcess:
    """Every rank of the group in this process (one GPU, or rank contexts on several
    devices): nothing travels; the exchange is summed on the device -- the reduction RCCL
    performs across GPUs, byte for byte (one contributor per byte)."""

    def __init__(self, world):
        self.ranks = range(world)

    def announce(self, op, kw):
        pass

    def agree(self, flags, record):
        return flags

    def collect(self, vals, heads, lists):
        return vals

    def reduce(self, bals, xs):
        sync = bals[0].torch.cuda.synchronize if xs[0].is_cuda else (lambda: None)
        sync()
        total = xs[0].clone()
        for x in xs[1:]:
            total += x
        for x in xs:
            x.copy_(total)
        sync()

    def phases(self, bals, op, kw):
        """The ranks' phases in step; a failure is every rank's (none of them commits)."""
        ok, res = _guarded(run_phases, bals, lambda b: _OPS[op].launch(b, kw), self.reduce)
        return [_guarded(_OPS[op].outputs, b, r) for b, r in zip(bals, res)] if ok else [(ok, res)] * len(bals)


class Distributed:
    """One rank per process (one process per GPU) over torch.distributed: rank 0 announces
    every call, and the ranks meet in the group's backend (RCCL over xGMI for ``nccl``)."""

    def __init__(self):
        import torch
        import torch.distributed as dist
        self.torch, self.dist, self.dev, self.ranks = torch, dist, _dev(dist), [dist.get_rank()]

    def announce(self, op, kw):
        _send_call(self.dist, self.dev, op, kw)

    reduce = staticmethod(dist_reduce)

    def phases(self, bals, op, kw):
        return [rank_phases(b, op, kw) for b in bals]

    def agree(self, flags, record):
        """The held rank's guarded value to every rank: one fixed record per rank, all-gathered
        -- (ok, code, the record's words) --, and only when a rank failed the messages, pickled.
        ``record`` None: the guarded values pickled whole.  Returns, on every rank, the list of
        (ok, value | (code, message)) in rank order."""
        torch, dist, world, (ok, val) = self.torch, self.dist, self.dist.get_world_size(), flags[0]
        if record is None:
            outs = [None] * world
            dist.all_gather_object(outs, flags[0])
            return outs
        rec = np.zeros(record.width, np.int64)
        if ok:
            words = record.pack(val)
            rec[0], rec[2:2 + len(words)] = 1, words
        else:
            rec[1] = val[0] if val[0] is not None else 0
        recs = [torch.zeros(record.width, dtype=torch.int64, device=self.dev) for _ in range(world)]
        dist.all_gather(recs, torch.from_numpy(rec).to(self.dev))
        recs = [x.cpu().numpy() for x in recs]
        msgs = [None] * world
        if not all(x[0] for x in recs):
            dist.all_gather_object(msgs, None if ok else val)
        return [(True, record.unpack(x[2:])) if x[0] else (False, msgs[i]) for i, x in enumerate(recs)]

    def collect(self, vals, heads, lists):
        """The ranks' lists to rank 0: one padded byte tensor per rank gathered there (none
        when no other rank has bytes; ``heads``: what the ranks agreed on, which sizes them).
        Returns, on rank 0, the ranks' values in rank order (its own as it is); else None."""
        torch, dist, rank = self.torch, self.dist, self.ranks[0]
        mx = max([lists.nbytes(h) for h in heads][1:], default=0)
        bufs = None
        if mx > 0:
            mine = torch.zeros(mx, dtype=torch.uint8)
            if rank != 0:
                payload = lists.pack(vals[0])
                mine[:len(payload)] = torch.from_numpy(payload)
            bufs = [torch.zeros(mx, dtype=torch.uint8, device=self.dev) for _ in heads] if rank == 0 else None
            dist.gather(mine.to(self.dev), bufs, dst=0)
        if rank != 0:
            return None
        none = np.zeros(0, np.uint8)
        return vals + [lists.unpack(heads[i], none if bufs is None else bufs[i].cpu().numpy()) for i in range(1, len(heads))]


class DistShardGroup(ShardGroup):
    """Rank 0's view of a table sharded over a torch.distributed group (one process
    per GPU): every call is broadcast to the ranks (serve_shard() runs on the
    others), each rank runs it on its own shard -- ticks with the exchange
    all-reduce over the group's backend -- and the per-rank results come back to rank 0."""

    def __init__(self, balancer, n_workers):
        super().__init__(n_workers, [balancer], Distributed())
        self.bal = balancer
        if self.transport.ranks[0] != 0:
            raise FaasbalError(_lib.FB_ESTATE, "DistShardGroup lives on rank 0; run serve_shard() on the others")
        # rank 0's phase 2 writes the whole assignment array (no (task, slot) pairs travel)
        balancer.set_full_assign(True)

    def close(self):
        self.transport.announce("stop", {})


def serve_shard(balancer):
    """Rank r > 0 of a DistShardGroup: run rank 0's calls on this shard until it stops."""
    tp = Distributed()
    while True:
        op, kw = _recv_call(tp.dist, tp.dev)
        if op == "stop":
            return
        _OPS[op].run(tp, [balancer], op, kw)  # rank 0 raises a failure; this rank keeps serving


class LocalShardGroup(ShardGroup):
    """Every rank's shard in this process (``.bals``), over the InProcess transport."""

    def __init__(self, world, n_workers, max_log, max_events=65536, device=0, rank_factory=None):
        make = rank_factory or (lambda r: ShardedBalancer(r, world, n_workers, max_log, max_events, device))
        super().__init__(n_workers, [make(r) for r in range(world)], InProcess(world))

    def _each(self, op, **kw):
        return self._collective_once(op, kw) if _OPS[op].run is _tick else super()._each(op, **kw)

    def _collective_once(self, op, kw):
        """A tick or purge on every rank, committed when all succeeded: the ranks' outputs, or
        the failure raised.  The one seam besides the transport: a group of rank doubles that
        cannot run the phases in step may put its own here (``serve_op`` per rank)."""
        return super()._each(op, **kw)

    def close(self):
        for b in self.bals:
            b.close()


def merge_outputs(outs, n_assigned):
    """Whole-table outputs from every rank's tick outputs (test / host-side helper): the
    assignment array of a rank that wrote it whole (set_full_assign), else the union of
    the ranks' (task, slot) pairs."""
    full = next((o["assign"] for o in outs if o.get("assign") is not None), None)
    if full is not None:
        assign = np.asarray(full, np.int32)
    else:
        assign = np.full(n_assigned, -1, np.int32)
        for o in outs:
            assign[o["task"]] = o["slot"]
    orphans = np.sort(np.concatenate([o["orphans"] for o in outs])) if outs else np.zeros(0, np.int64)
    evicted = np.sort(np.concatenate([o["evicted"] for o in outs])) if outs else np.zeros(0, np.int32)
    return dict(reconnect=outs[0]["reconnect"], assign=assign, orphans=orphans.astype(np.int64),
                evicted=evicted.astype(np.int32))
