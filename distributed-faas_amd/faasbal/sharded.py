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

import ctypes as C

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

    def _allreduce(self, allreduce):
        n = C.c_int64()
        self._chk(self.lib.fb_exchange_bytes(self.h, self._E, C.byref(n)))
        self._xbytes = n.value
        with self.torch.cuda.stream(self.stream):
            if allreduce is None:
                # issued on self.stream; the explicit wait orders phase 2 after it on that
                # stream (RCCL) or after its completion (gloo)
                self.torch.distributed.all_reduce(self.exchange(), async_op=True).wait()
            else:
                allreduce(self.exchange())

    def _run_phases(self, launch, allreduce):
        """Phase 1, the exchange, phase 2 and the wait -- again with a wider round table
        while the tick asks for it (FB_ERERUN: the same tick, relaunched; every rank
        gets the same answer, so the ranks' collectives stay matched)."""
        for attempt in range(MAX_RELAUNCH + 1):
            launch()
            self._allreduce(allreduce)
            self.cont()
            try:
                return self.wait()
            except FaasbalError as e:
                if e.code != FB_ERERUN or attempt == MAX_RELAUNCH:
                    raise

    def purge(self, now, tte, commit=True, allreduce=None):
        """This rank's share of ``purge_workers`` (``task_dispatcher.py:241-249``):
        the exchange and phase 2 run as for a tick, nothing is dispatched; returns
        dict(result, evicted, orphans) of this rank's slots and log shard."""
        self._E = 0
        res = self._run_phases(lambda: self._chk(self.lib.fb_purge_launch(self.h, float(now), float(tte))),
                               allreduce)
        out = dict(result=res, evicted=self.evicted(), orphans=self.orphans())
        if commit:
            self.commit()
        return out

    def tick(self, now, tte, ev_kind=(), ev_slot=(), ev_val=(), ev_ts=(), ev_seq=None, n_pending=0,
             commit=True, outputs=True, allreduce=None):
        """One sharded tick; ``allreduce(tensor)`` defaults to torch.distributed.all_reduce (SUM)."""
        res = self._run_phases(lambda: self.launch(now, tte, ev_kind, ev_slot, ev_val, ev_ts, ev_seq, n_pending),
                               allreduce)
        out = dict(result=res)
        if outputs:
            # the whole tick's assignments where this rank writes them (set_full_assign), else
            # this rank's own (task, slot) pairs
            if getattr(self, "full_assign", False):
                out.update(assign=self.assignments())
            else:
                task, slot = self.local_assignments()
                out.update(task=task, slot=slot)
            out.update(reconnect=self.event_status(), orphans=self.orphans(), evicted=self.evicted())
        if commit:
            self.commit()
        return out


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
    flow and Redis I/O are the same for one GPU and for N.  Subclasses say how a
    call reaches the ranks: in this process (LocalShardGroup) or over
    torch.distributed from rank 0 (DistShardGroup)."""

    mode = "heartbeat"

    def __init__(self, n_workers, rank_balancers=()):
        self.n_workers_global = int(n_workers)
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
        raise NotImplementedError

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


def _guarded(f, *a):
    try:
        return (True, f(*a))
    except Exception as e:  # noqa: BLE001 -- the group raises it once every rank has answered
        return (False, _failure(e))


def serve_op(bal, op, kw, allreduce=None, commit=True):
    """One group operation on this rank's balancer (every rank runs the same op).
    ``commit=False`` leaves a tick / purge waited but uncommitted (DistShardGroup
    commits only once every rank has succeeded)."""
    if op == "load":
        bal.load(kw["st"])
        return None
    if op == "read":
        return bal.read_state(with_log=kw["with_log"])
    if op == "tick":
        out = bal.tick(kw["now"], kw["tte"], kw["ev_kind"], kw["ev_slot"], kw["ev_val"], kw["ev_ts"], kw["ev_seq"],
                       kw["n_pending"], allreduce=allreduce, commit=commit)
        return out
    if op == "purge":
        return bal.purge(kw["now"], kw["tte"], allreduce=allreduce, commit=commit)
    if op == "stats":  # (reads only: nothing to commit, nothing to settle)
        return bal.pool_stats_part(kw["now"], kw["tte"], kw["age_edges"])
    if op == "compact":  # (a collective of its own: mark, reduce, agree, apply or cancel)
        import torch.distributed as dist
        out, bad = _compact_rank(dist, _dev(dist), bal, kw, allreduce)
        if bad is not None:
            _raise_bad(op, bad)
        return out
    if op == "reclaim":  # (an agreement of its own: count, agree, take)
        import torch.distributed as dist
        out, bad = _reclaim_rank(dist, _dev(dist), bal, kw)
        if bad is not None:
            _raise_bad(op, bad)
        return out
    raise ValueError("unknown group operation %r" % op)


def _raise_bad(op, bad):
    code, msg = bad
    if code is None:
        raise RuntimeError("shard operation %r failed on a rank: %s" % (op, msg))
    raise FaasbalError(code, "shard operation %r failed on a rank: %s" % (op, msg))


def _failure(e):
    return (getattr(e, "code", None), "%s: %s" % (type(e).__name__, e))


def _compact_verdict(marks, expect):
    """(the group's live count, the first failure or None) from every rank's guarded mark."""
    bad = next((m[1] for m in marks if not m[0]), None)
    total = sum(int(m[1]) for m in marks if m[0])
    if bad is None and expect >= 0 and expect != total:
        bad = (_lib.FB_ESTATE, "the group's log holds %d live entries, the caller expected %d" % (total, expect))
    return total, bad


def _compact_reduce(bal, x, allreduce):
    """The bitmap all-reduced in place, on the rank's stream where it has one (as a tick's exchange)."""
    import contextlib
    stream = getattr(bal, "stream", None)
    with (bal.torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
        if allreduce is None:
            import torch.distributed as dist
            dist.all_reduce(x, async_op=True).wait()
        else:
            allreduce(x)


def _gather_flags(dist, dev, ok, err, word=0):
    """One fixed header per rank, all-gathered: (ok, code, word).  Returns, on every rank, the
    list of (ok, word | (code, message)) in rank order; messages follow pickled only when a
    rank failed, as for ticks."""
    import torch
    world = dist.get_world_size()
    h = torch.zeros(_HDR, dtype=torch.int64)
    h[0] = 1 if ok else 0
    h[1] = 0 if ok or err[0] is None else int(err[0])
    h[2] = int(word)
    hs = [torch.zeros(_HDR, dtype=torch.int64, device=dev) for _ in range(world)]
    dist.all_gather(hs, h.to(dev))
    hs = [x.cpu().numpy() for x in hs]
    if all(x[0] for x in hs):
        return [(True, int(x[2])) for x in hs]
    msgs = [None] * world
    dist.all_gather_object(msgs, None if ok else err)
    return [(True, int(x[2])) if x[0] else (False, msgs[i]) for i, x in enumerate(hs)]


def _compact_rank(dist, dev, bal, kw, allreduce=None):
    """A group compaction on this rank (every rank runs it): mark, the bitmap's all-reduce --
    which a rank whose mark failed joins with zeros of the agreed size, so that no rank blocks
    in the collective --, one header all-gather of the ranks' ok flags and live counts, then
    every rank applies or every rank cancels.  Rank 0 asks for the kept list.  Returns
    (this rank's compact_apply result or None, the first failure or None)."""
    try:
        mark = (True, bal.compact_mark())
    except Exception as e:  # noqa: BLE001 -- reported to rank 0, which raises it
        mark = (False, _failure(e))
    x = bal.compact_exchange(zeroed=not mark[0])
    if x.numel():
        _compact_reduce(bal, x, allreduce)
    marks = _gather_flags(dist, dev, mark[0], None if mark[0] else mark[1], mark[1] if mark[0] else 0)
    total, bad = _compact_verdict(marks, kw["expect"])
    out = None
    if bad is None:
        try:
            done = (True, bal.compact_apply(total, bool(kw["want_kept"]) and dist.get_rank() == 0))
        except Exception as e:  # noqa: BLE001
            done = (False, _failure(e))
        # (the count gives every rank the same verdict; what is left is a rank's own runtime error)
        flags = _gather_flags(dist, dev, done[0], None if done[0] else done[1])
        bad = next((f[1] for f in flags if not f[0]), None)
        out = done[1] if done[0] else None
    if bad is not None:
        bal.compact_cancel()
    return out, bad


def _reclaim_rank(dist, dev, bal, kw):
    """A group reclaim on this rank (every rank runs it): count, one header all-gather of the
    ranks' ok flags and counts -- when a rank refused nothing has changed anywhere, and no rank
    takes --, take, a second header (a take that fails now is the rank's own runtime error),
    then the lists to rank 0 as one padded byte tensor per rank, 12 bytes per entry (the
    sequences, then the slots).  Returns (rank 0: the ranks' dict(n, seq, slot) in rank order;
    the others: None, the first failure or None)."""
    import torch
    rank, world = dist.get_rank(), dist.get_world_size()
    cnt = _guarded(bal.reclaim_part, kw["below_seq"], kw["slots"], True)
    flags = _gather_flags(dist, dev, cnt[0], None if cnt[0] else cnt[1], cnt[1]["n"] if cnt[0] else 0)
    bad = next((f[1] for f in flags if not f[0]), None)
    if bad is not None:
        return None, bad
    done = _guarded(bal.reclaim_part, kw["below_seq"], kw["slots"])
    if done[0] and done[1]["n"] != flags[rank][1]:
        done = (False, (_lib.FB_ESTATE, "rank %d counted %d entries to reclaim and took %d"
                        % (rank, flags[rank][1], done[1]["n"])))
    after = _gather_flags(dist, dev, done[0], None if done[0] else done[1])
    bad = next((f[1] for f in after if not f[0]), None)
    if bad is not None:
        return None, bad
    counts = [int(f[1]) for f in flags]
    mx = max(counts[1:], default=0)
    parts = [done[1]] + [dict(n=0, seq=np.zeros(0, np.int64), slot=np.zeros(0, np.int32)) for _ in range(world - 1)]
    if mx > 0:
        mine = torch.zeros(12 * mx, dtype=torch.uint8)
        if rank != 0 and counts[rank]:
            payload = np.concatenate([np.ascontiguousarray(done[1]["seq"], np.int64).view(np.uint8),
                                      np.ascontiguousarray(done[1]["slot"], np.int32).view(np.uint8)])
            mine[:len(payload)] = torch.from_numpy(payload)
        bufs = [torch.zeros(12 * mx, dtype=torch.uint8, device=dev) for _ in range(world)] if rank == 0 else None
        dist.gather(mine.to(dev), bufs, dst=0)
        if rank == 0:
            for i in range(1, world):
                b, n = bufs[i].cpu().numpy(), counts[i]
                parts[i] = dict(n=n, seq=b[:8 * n].view(np.int64).copy(), slot=b[8 * n:12 * n].view(np.int32).copy())
    return (parts if rank == 0 else None), None


def _serve_guarded(bal, op, kw):
    """serve_op on this rank, its failure returned instead of raised: every rank must
    still reach the group's gather (a rank that skipped it would leave the others
    blocked in the collective).  A tick / purge is not committed here."""
    try:
        return (True, serve_op(bal, op, kw, commit=False))
    except Exception as e:  # noqa: BLE001 -- reported to rank 0, which raises it
        return (False, (getattr(e, "code", None), "%s: %s" % (type(e).__name__, e)))


def _settle(bal, op, outs):
    """After the gather, on every rank: commit a tick / purge only when it succeeded
    on every rank (so the shards never diverge); returns the first failure or None."""
    bad = next((o[1] for o in outs if not o[0]), None)
    if bad is None and op in ("tick", "purge"):
        bal.commit()
    return bad


# DistShardGroup's wire format per call: a fixed header tensor broadcast from rank 0
# (operation, event count, tasks, clock), then for ticks / purges the event batch packed
# into one byte tensor (25 B per message), and back a fixed header per rank (all
# gathered: every rank commits only when all succeeded) plus one padded byte tensor
# per rank gathered to rank 0 (tasks, slots, orphans, evicted).  Loads and state reads
# (not per tick) and failure messages travel as pickled objects.
# A pool summary ("stats") travels as tensors too: the call header carries the number of
# age edges in the event count's word and the clock and tte in theirs, the edges follow as
# one float64 tensor when there are any, and every rank's part comes back as one fixed
# int64 record (an ok flag, a code, the queue's length, then fb_pool_summary's words in
# the struct's order, doubles as bit patterns), all-gathered so that every rank sees every
# flag; only when a rank failed do the messages follow, pickled, as for ticks.
# A log compaction ("compact") is a header alone: the caller's expected live count (-1: none)
# in the event count's word, whether rank 0 wants the kept list in the tasks' word.  Its
# payload is the live bitmap, all-reduced in place like a tick's exchange; one fixed header
# per rank (ok flag, code, live count) is all-gathered before the apply and one after it.
# A reclaim ("reclaim") travels as tensors as well, since with task_timeout it can run at the
# top of every tick: the call header carries below_seq in the event count's word and the number
# of slots in the tasks' word (-1: no mask), the global slots follow as one int32 tensor when
# there are any; one fixed header per rank (ok flag, code, count) is all-gathered after the
# count step and one after the take, and the lists come back as one padded byte tensor per rank
# gathered to rank 0, 12 bytes per entry (the int64 sequences, then the int32 slots); pickled
# messages follow only when a rank failed.
_OP_CODES = {"tick": 1, "purge": 2, "load": 3, "read": 4, "stop": 5, "stats": 6, "compact": 7, "reclaim": 8}
_OP_NAMES = {v: k for k, v in _OP_CODES.items()}
_HDR = 8  # int64 words of the call header / the per-rank result header
_PS_WORDS = C.sizeof(_lib.PoolSummary) // 8  # fb_pool_summary's words (SCALARS' order, then HISTS')
_PS_REC = 3 + _PS_WORDS
_PS_DOUBLES = ("oldest_hb", "newest_hb")


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


def _dev(dist):
    import torch
    return torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")


def _pack_events(kw):
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


def _bcast_call(dist, dev, op, kw):
    """Rank 0: the call to every rank.  Returns nothing; the ranks read it with _recv_call."""
    import torch
    h = torch.zeros(_HDR, dtype=torch.int64)
    h[0] = _OP_CODES[op]
    if op in ("tick", "purge"):
        E = len(kw.get("ev_kind", ())) if op == "tick" else 0
        h[1] = E
        h[2] = int(kw.get("n_pending", 0))
        h[3] = int(np.float64(kw["now"]).view(np.int64))
        h[4] = int(np.float64(kw["tte"]).view(np.int64))
    elif op == "stats":
        h[1] = len(kw["age_edges"])
        h[3] = int(np.float64(kw["now"]).view(np.int64))
        h[4] = int(np.float64(kw["tte"]).view(np.int64))
    elif op == "compact":  # (the header is the whole call)
        h[1] = int(kw["expect"])
        h[2] = 1 if kw["want_kept"] else 0
    elif op == "reclaim":
        h[1] = int(kw["below_seq"])
        h[2] = -1 if kw["slots"] is None else len(kw["slots"])
    dist.broadcast(h.to(dev), src=0)
    if op in ("tick", "purge"):
        if int(h[1]):
            dist.broadcast(torch.from_numpy(_pack_events(kw)).to(dev), src=0)
    elif op == "stats":
        if int(h[1]):
            dist.broadcast(torch.from_numpy(np.ascontiguousarray(kw["age_edges"], np.float64)).to(dev), src=0)
    elif op == "reclaim":
        if int(h[2]) > 0:
            dist.broadcast(torch.from_numpy(np.ascontiguousarray(kw["slots"], np.int32)).to(dev), src=0)
    elif op not in ("stop", "compact"):
        dist.broadcast_object_list([kw], src=0)


def _recv_call(dist, dev):
    """Ranks > 0: the next call of rank 0 as (op, kw)."""
    import torch
    h = torch.zeros(_HDR, dtype=torch.int64, device=dev)
    dist.broadcast(h, src=0)
    h = h.cpu().numpy()
    op = _OP_NAMES[int(h[0])]
    if op == "compact":
        return op, dict(expect=int(h[1]), want_kept=bool(h[2]))
    if op == "reclaim":
        slots = None
        if int(h[2]) >= 0:
            slots = torch.zeros(int(h[2]), dtype=torch.int32, device=dev)
            if int(h[2]):
                dist.broadcast(slots, src=0)
            slots = slots.cpu().numpy()
        return op, dict(below_seq=int(h[1]), slots=slots)
    if op == "stats":
        edges = torch.zeros(int(h[1]), dtype=torch.float64, device=dev)
        if int(h[1]):
            dist.broadcast(edges, src=0)
        return op, dict(now=float(h[3:4].view(np.float64)[0]), tte=float(h[4:5].view(np.float64)[0]),
                        age_edges=edges.cpu().numpy())
    if op not in ("tick", "purge"):
        if op == "stop":
            return op, {}
        box = [None]
        dist.broadcast_object_list(box, src=0)
        return op, box[0]
    E = int(h[1])
    kw = dict(now=float(h[3:4].view(np.float64)[0]), tte=float(h[4:5].view(np.float64)[0]), n_pending=int(h[2]))
    if op == "tick":
        if E:
            buf = torch.empty(25 * E, dtype=torch.uint8, device=dev)
            dist.broadcast(buf, src=0)
            kw.update(_unpack_events(buf.cpu().numpy(), E))
        else:
            z = np.zeros(0)
            kw.update(ev_kind=z.astype(np.uint8), ev_slot=z.astype(np.int32), ev_val=z.astype(np.int32),
                      ev_ts=z.astype(np.float64), ev_seq=z.astype(np.int64))
    return op, kw


def _gather_results(dist, dev, op, guarded):
    """Every rank: its guarded result of a tick / purge.  Returns, on every rank, the
    list of (ok, value | (code, message)) in rank order -- values complete on rank 0
    (the other ranks get headers only, enough to settle the commit)."""
    import torch
    ok, val = guarded
    rank, world = dist.get_rank(), dist.get_world_size()
    h = torch.zeros(_HDR, dtype=torch.int64)
    payload = np.zeros(0, np.uint8)
    if ok:
        r = val["result"]
        # (rank 0 writes the whole assignment array itself, fb_set_full_assign: the other
        # ranks send only their orphans and evicted slots, a few KB)
        task = np.zeros(0, np.int64)
        slot = np.zeros(0, np.int32)
        orph = np.asarray(val["orphans"], np.int64)
        evic = np.asarray(val["evicted"], np.int32)
        h[0] = 1
        h[2], h[3], h[4] = int(r.get("n_local", 0)), int(r.get("n_orphans_local", 0)), int(r["n_evicted"])
        h[5], h[6], h[7] = len(task), len(orph), len(evic)
        if rank != 0:
            payload = np.concatenate([task.view(np.uint8), slot.view(np.uint8), orph.view(np.uint8),
                                      evic.view(np.uint8)])
    else:
        h[1] = val[0] if val[0] is not None else 0
    hs = [torch.zeros(_HDR, dtype=torch.int64, device=dev) for _ in range(world)]
    dist.all_gather(hs, h.to(dev))
    hs = [x.cpu().numpy() for x in hs]
    if not all(x[0] for x in hs):
        # a rank failed: its message (pickled: failures only)
        msgs = [None] * world
        dist.all_gather_object(msgs, None if ok else val)
        return [(bool(x[0]), None if x[0] else msgs[i]) for i, x in enumerate(hs)]
    nbytes = [int(x[5]) * 12 + int(x[6]) * 8 + int(x[7]) * 4 for x in hs]
    mx = max(nbytes[1:], default=0)
    outs = [(True, val if rank == 0 else None)] + [(True, None)] * (world - 1)
    if world > 1 and mx > 0:
        mine = torch.zeros(mx, dtype=torch.uint8)
        if rank != 0:
            mine[:len(payload)] = torch.from_numpy(payload)
        bufs = [torch.zeros(mx, dtype=torch.uint8, device=dev) for _ in range(world)] if rank == 0 else None
        dist.gather(mine.to(dev), bufs, dst=0)
        if rank == 0:
            for i in range(1, world):
                b = bufs[i].cpu().numpy()
                nt, no, ne = int(hs[i][5]), int(hs[i][6]), int(hs[i][7])
                o = [0, 8 * nt, 12 * nt, 12 * nt + 8 * no, 12 * nt + 8 * no + 4 * ne]
                res = dict(n_local=int(hs[i][2]), n_orphans_local=int(hs[i][3]), n_evicted=int(hs[i][4]))
                d = dict(result=res, orphans=b[o[2]:o[3]].view(np.int64).copy(),
                         evicted=b[o[3]:o[4]].view(np.int32).copy(), reconnect=None)
                outs[i] = (True, d)
    elif rank == 0:
        for i in range(1, world):
            res = dict(n_local=int(hs[i][2]), n_orphans_local=int(hs[i][3]), n_evicted=int(hs[i][4]))
            d = dict(result=res, orphans=np.zeros(0, np.int64), evicted=np.zeros(0, np.int32), reconnect=None)
            outs[i] = (True, d)
    return outs


def _gather_stats(dist, dev, guarded):
    """Every rank: its guarded part of a pool summary.  Returns, on every rank, the list of
    (ok, (part, queue_len) | (code, message)) in rank order."""
    import torch
    ok, val = guarded
    world = dist.get_world_size()
    rec = np.zeros(_PS_REC, np.int64)
    if ok:
        rec = _pack_summary(*val)
    else:
        rec[1] = val[0] if val[0] is not None else 0
    recs = [torch.zeros(_PS_REC, dtype=torch.int64, device=dev) for _ in range(world)]
    dist.all_gather(recs, torch.from_numpy(rec).to(dev))
    recs = [x.cpu().numpy() for x in recs]
    if not all(x[0] for x in recs):
        msgs = [None] * world
        dist.all_gather_object(msgs, None if ok else val)
        return [(bool(x[0]), None if x[0] else msgs[i]) for i, x in enumerate(recs)]
    return [(True, _unpack_summary(x)) for x in recs]


def _gather(dist, dev, op, guarded):
    """The ranks' guarded results of one operation, on every rank, in rank order."""
    if op in ("tick", "purge"):
        return _gather_results(dist, dev, op, guarded)
    if op == "stats":
        return _gather_stats(dist, dev, guarded)
    outs = [None] * dist.get_world_size()
    dist.all_gather_object(outs, guarded)
    return outs


class DistShardGroup(ShardGroup):
    """Rank 0's view of a table sharded over a torch.distributed group (one process
    per GPU): every call is broadcast to the ranks (serve_shard() runs on the
    others), each rank runs it on its own shard -- ticks with the exchange
    all-reduce over the group's backend (RCCL over xGMI for ``nccl``) -- and the
    per-rank results come back to rank 0.  Ticks and purges travel as tensors (the
    event batch in one broadcast, the results in one gather) and so do pool summaries (one
    fixed record per rank), log compactions (the live bitmap all-reduced in place, a fixed
    header per rank) and reclaims (a fixed header per rank, the lists in one gather); loads and
    state reads as pickled objects."""

    def __init__(self, balancer, n_workers):
        super().__init__(n_workers, (balancer,))
        import torch.distributed as dist
        self.dist, self.bal = dist, balancer
        if dist.get_rank() != 0:
            raise FaasbalError(_lib.FB_ESTATE, "DistShardGroup lives on rank 0; run serve_shard() on the others")
        self.dev = _dev(dist)
        # rank 0's phase 2 writes the whole assignment array (the per-task gather is gone)
        balancer.set_full_assign(True)

    def _each(self, op, **kw):
        _bcast_call(self.dist, self.dev, op, kw)
        if op == "compact":
            out, bad = _compact_rank(self.dist, self.dev, self.bal, kw)
            if bad is not None:
                _raise_bad(op, bad)
            return [out]
        if op == "reclaim":
            parts, bad = _reclaim_rank(self.dist, self.dev, self.bal, kw)
            if bad is not None:
                _raise_bad(op, bad)
            return parts
        guarded = _serve_guarded(self.bal, op, kw)
        outs = _gather(self.dist, self.dev, op, guarded)
        bad = _settle(self.bal, op, outs)
        if bad is not None:
            _raise_bad(op, bad)
        return [o[1] for o in outs]

    def close(self):
        _bcast_call(self.dist, self.dev, "stop", {})


def serve_shard(balancer):
    """Rank r > 0 of a DistShardGroup: run rank 0's calls on this shard until it stops."""
    import torch.distributed as dist
    dev = _dev(dist)
    while True:
        op, kw = _recv_call(dist, dev)
        if op == "stop":
            return
        if op == "compact":
            _compact_rank(dist, dev, balancer, kw)  # rank 0 raises a failure; this rank keeps serving
            continue
        if op == "reclaim":
            _reclaim_rank(dist, dev, balancer, kw)  # (likewise: a refused reclaim changed nothing)
            continue
        guarded = _serve_guarded(balancer, op, kw)
        outs = _gather(dist, dev, op, guarded)
        _settle(balancer, op, outs)  # rank 0 raises a failure; this rank keeps serving


class LocalShardGroup(ShardGroup):
    """Every rank's shard in this process (one GPU, or rank contexts on several
    devices); the exchange is summed on the device -- the reduction RCCL performs
    across GPUs, byte for byte (one contributor per byte)."""

    def __init__(self, world, n_workers, max_log, max_events=65536, device=0, rank_factory=None):
        make = rank_factory or (lambda r: ShardedBalancer(r, world, n_workers, max_log, max_events, device))
        self.bals = [make(r) for r in range(world)]
        super().__init__(n_workers, self.bals)

    def _each(self, op, **kw):
        if op in ("tick", "purge"):
            return self._collective(op, kw)
        if op == "compact":
            return self._compact(kw)
        if op == "reclaim":
            return self._reclaim(kw)
        return [serve_op(b, op, kw) for b in self.bals]

    def _reclaim(self, kw):
        # every rank counts -- every refusal a rank would make, with nothing changed anywhere --
        # and only when all of them can do the ranks take
        counts = [_guarded(b.reclaim_part, kw["below_seq"], kw["slots"], True) for b in self.bals]
        bad = next((c[1] for c in counts if not c[0]), None)
        if bad is not None:
            _raise_bad("reclaim", bad)
        return [b.reclaim_part(kw["below_seq"], kw["slots"]) for b in self.bals]

    def _compact(self, kw):
        # mark on every rank, the bitmaps summed on the device (as _collective_once sums the
        # exchange), apply on every rank -- or, when a rank could not mark or the total is not
        # the caller's, cancel on every rank: nothing has changed anywhere
        def guarded(f, *a):
            try:
                return (True, f(*a))
            except Exception as e:  # noqa: BLE001 -- raised below, once every rank is cancelled
                return (False, _failure(e))

        total, bad = _compact_verdict([guarded(b.compact_mark) for b in self.bals], kw["expect"])
        outs = []
        if bad is None:
            xs = [b.compact_exchange() for b in self.bals]
            if xs[0].numel():
                sync = self.bals[0].torch.cuda.synchronize if xs[0].is_cuda else (lambda: None)
                sync()
                union = xs[0].clone()
                for x in xs[1:]:
                    union += x
                for x in xs:
                    x.copy_(union)
                sync()
            outs = [guarded(b.compact_apply, total, bool(kw["want_kept"]) and r == 0) for r, b in enumerate(self.bals)]
            bad = next((o[1] for o in outs if not o[0]), None)
        if bad is not None:
            for b in self.bals:
                b.compact_cancel()
            _raise_bad("compact", bad)
        return [o[1] for o in outs]

    def _collective(self, op, kw):
        # phase 1 on every rank, then the summed exchange, then phase 2 / outputs / commit;
        # relaunched with a wider round table while the ranks ask for it (FB_ERERUN)
        for attempt in range(MAX_RELAUNCH + 1):
            try:
                return self._collective_once(op, kw)
            except FaasbalError as e:
                if e.code != FB_ERERUN or attempt == MAX_RELAUNCH:
                    raise

    def _collective_once(self, op, kw):
        torch = self.bals[0].torch
        for b in self.bals:
            if op == "tick":
                b.launch(kw["now"], kw["tte"], kw["ev_kind"], kw["ev_slot"], kw["ev_val"], kw["ev_ts"], kw["ev_seq"],
                         kw["n_pending"])
            else:
                b._E = 0
                b._chk(b.lib.fb_purge_launch(b.h, kw["now"], kw["tte"]))
                n = C.c_int64()
                b._chk(b.lib.fb_exchange_bytes(b.h, 0, C.byref(n)))
                b._xbytes = n.value
        torch.cuda.synchronize()
        total = self.bals[0].exchange().clone()
        for b in self.bals[1:]:
            total += b.exchange()
        for b in self.bals:
            b.exchange().copy_(total)
        torch.cuda.synchronize()
        for b in self.bals:
            b.cont()
        res_all = []
        err = None
        for b in self.bals:  # every rank waits (a rerun request reaches them all)
            try:
                res_all.append(b.wait())
            except FaasbalError as e:
                err = err or e
        if err is not None:
            raise err
        outs = []
        for b, res in zip(self.bals, res_all):
            if op == "tick":
                task, slot = b.local_assignments()
                outs.append(dict(result=res, task=task, slot=slot, orphans=b.orphans(), evicted=b.evicted(),
                                 reconnect=b.event_status()))
            else:
                outs.append(dict(result=res, evicted=b.evicted(), orphans=b.orphans()))
        for b in self.bals:
            b.commit()
        return outs

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
