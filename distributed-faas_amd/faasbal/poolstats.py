"""The pool summary (fb_pool_stats, include/faasbal.h) over a ``read_state()`` dict in numpy.

``GpuPushDispatcher.pool_stats`` takes this path for balancers without a device summary (test
doubles); the tests and tools/stats_probe.py hold the device path against it.  Shard groups
summarise on the device too, a part per rank (fb_pool_stats_shard): ``pool_stats_part_model``
is a part's model and ``merge_summaries`` the fold of the parts (fb_pool_merge).
Liveness is the tick's ``(now - hb) > tte`` in float64, subtract then compare, and the age
bins use the same subtraction against the caller's edges -- no other arithmetic, so the
figures are the device's bit for bit.
"""
import numpy as np

from ._lib import PS_FREE_BINS as FREE_BINS, PS_MAX_EDGES as MAX_EDGES
SCALARS = ("n_slots", "n_registered", "n_expired", "n_queued", "n_queued_expired", "dispatchable", "free_total",
           "log_head", "inflight", "inflight_expired", "inflight_max", "oldest_hb", "newest_hb")
HISTS = ("free_hist", "age_hist")


def check_edges(age_edges):
    e = np.asarray(age_edges, np.float64).reshape(-1)
    if len(e) > MAX_EDGES:
        raise ValueError("%d age edges, at most %d" % (len(e), MAX_EDGES))
    if not np.all(np.isfinite(e)) or np.any(np.diff(e) <= 0):
        raise ValueError("age edges must be finite and strictly ascending")
    return e


def pool_stats_model(st, now, tte, age_edges=(), deque=False, inflight_counts=None):
    """The dict ``GpuBalancer.pool_stats`` returns, from reg / free / hb / epoch / queue / log.

    ``deque``: a context without liveness (nothing expires; ``now``, ``tte`` and the edges are
    ignored).  ``inflight_counts``: whether the context keeps per-slot in-flight counts
    (``inflight_max`` is -1 without them); by default heartbeat contexts do."""
    reg = np.asarray(st["reg"]) != 0
    free = np.asarray(st["free"]).astype(np.int64)
    hb = np.asarray(st["hb"], np.float64)
    epoch = np.asarray(st["epoch"]).astype(np.int64)
    queue = np.asarray(st["queue"]).astype(np.int64)
    log = np.asarray(st["log"]).astype(np.int64)
    W, head = len(reg), len(log)
    if inflight_counts is None:
        inflight_counts = not deque
    age_hist = np.zeros(MAX_EDGES + 1, np.int64)
    if deque:
        expired = np.zeros(W, bool)
    else:
        edges = check_edges(age_edges)
        with np.errstate(invalid="ignore", over="ignore"):
            age = np.float64(now) - hb
            expired = reg & (age > np.float64(tte))
            nbin = np.zeros(W, np.int64)
            for e in edges:
                nbin += age > e
        age_hist = np.bincount(nbin[reg], minlength=MAX_EDGES + 1).astype(np.int64)
    alive = reg & ~expired  # (the sums below: at most 2^31 slots of less than 2^31 each, exact in int64)
    qexp = expired[queue]
    live = (log >= 0) & (W > 0)  # (no slot, no entry)
    s = np.maximum(log, 0)
    if not deque and head and W:
        live &= reg[s] & (np.arange(head) >= epoch[s])
    lexp = live & expired[s] if head and W else np.zeros(head, bool)
    hbs = hb[alive & ~np.isnan(hb)]
    out = dict(
        n_slots=W, n_registered=int(reg.sum()), n_expired=int(expired.sum()),
        n_queued=int((~qexp).sum()), n_queued_expired=int(qexp.sum()),
        dispatchable=-1 if deque else int(np.maximum(free[queue[~qexp]], 1).sum(dtype=np.int64)),
        free_total=int(np.maximum(free[alive], 0).sum(dtype=np.int64)),
        log_head=head, inflight=int((live & ~lexp).sum()), inflight_expired=int(lexp.sum()),
        inflight_max=-1,
        oldest_hb=float(hbs.min()) if len(hbs) and not deque else float("nan"),
        newest_hb=float(hbs.max()) if len(hbs) and not deque else float("nan"),
        free_hist=np.bincount(np.clip(free[alive], 0, FREE_BINS - 1), minlength=FREE_BINS).astype(np.int64),
        age_hist=age_hist)
    if inflight_counts:
        per = np.bincount(log[live], minlength=W)[:W][reg] if W else np.zeros(0, np.int64)
        out["inflight_max"] = int(per.max()) if len(per) else 0
    return out


def pool_stats_part_model(sh, now, tte, age_edges=()):
    """One rank's part of a shard group's summary (fb_pool_stats_shard) as ``(dict, queue_len)``,
    over a ``split_state`` or ``ShardedBalancer.read_state`` dict: its own slots, the positions
    of the replicated queue on them, its log shard (global slots; an entry is live by its global
    sequence), the global log head; ``inflight_max`` is -1."""
    base = int(sh["base"])
    reg = np.asarray(sh["reg"]) != 0
    free = np.asarray(sh["free"]).astype(np.int64)
    hb = np.asarray(sh["hb"], np.float64)
    epoch = np.asarray(sh["epoch"]).astype(np.int64)
    queue = np.asarray(sh["queue"]).astype(np.int64)
    log = np.asarray(sh["log_slot"] if "log_slot" in sh else sh["log"]).astype(np.int64)
    seq = np.asarray(sh["log_seq"]).astype(np.int64)
    head = int(sh["log_head"] if "log_head" in sh else sh["head"])
    W = len(reg)
    edges = check_edges(age_edges)
    with np.errstate(invalid="ignore", over="ignore"):
        age = np.float64(now) - hb
        expired = reg & (age > np.float64(tte))
        nbin = np.zeros(W, np.int64)
        for e in edges:
            nbin += age > e
    alive = reg & ~expired
    own = queue[(queue >= base) & (queue < base + W)] - base
    qexp = expired[own]
    ls = log - base
    live = (log >= 0) & (ls >= 0) & (ls < W)
    s = np.clip(ls, 0, max(W - 1, 0))
    if len(log) and W:
        live &= reg[s] & (seq >= epoch[s])
        lexp = live & expired[s]
    else:
        live = np.zeros(len(log), bool)
        lexp = live
    hbs = hb[alive & ~np.isnan(hb)]
    out = dict(
        n_slots=W, n_registered=int(reg.sum()), n_expired=int(expired.sum()),
        n_queued=int((~qexp).sum()), n_queued_expired=int(qexp.sum()),
        dispatchable=int(np.maximum(free[own[~qexp]], 1).sum(dtype=np.int64)),
        free_total=int(np.maximum(free[alive], 0).sum(dtype=np.int64)),
        log_head=head, inflight=int((live & ~lexp).sum()), inflight_expired=int(lexp.sum()), inflight_max=-1,
        oldest_hb=float(hbs.min()) if len(hbs) else float("nan"),
        newest_hb=float(hbs.max()) if len(hbs) else float("nan"),
        free_hist=np.bincount(np.clip(free[alive], 0, FREE_BINS - 1), minlength=FREE_BINS).astype(np.int64),
        age_hist=np.bincount(nbin[reg], minlength=MAX_EDGES + 1).astype(np.int64))
    return out, len(queue)


def merge_summaries(parts, queue_lens):
    """fb_pool_merge: the ranks' parts folded into the group's summary.  ``ValueError`` where
    the C call returns FB_EINVAL (no parts, differing log heads or queue lengths, queue
    positions that do not sum to the queue's length)."""
    parts, queue_lens = list(parts), [int(q) for q in queue_lens]
    if not parts or len(parts) != len(queue_lens):
        raise ValueError("merge_summaries: %d parts, %d queue lengths" % (len(parts), len(queue_lens)))
    if any(p["log_head"] != parts[0]["log_head"] for p in parts):
        raise ValueError("merge_summaries: the parts' log heads differ: %r" % [p["log_head"] for p in parts])
    if any(q != queue_lens[0] for q in queue_lens):
        raise ValueError("merge_summaries: the parts' queue lengths differ: %r" % queue_lens)
    out = {k: sum(int(p[k]) for p in parts)
           for k in ("n_slots", "n_registered", "n_expired", "n_queued", "n_queued_expired", "dispatchable",
                     "free_total", "inflight", "inflight_expired")}
    if out["n_queued"] + out["n_queued_expired"] != queue_lens[0]:
        raise ValueError("merge_summaries: the parts hold %d + %d queue positions, the queue %d"
                         % (out["n_queued"], out["n_queued_expired"], queue_lens[0]))
    out["log_head"] = int(parts[0]["log_head"])
    imax = [int(p["inflight_max"]) for p in parts]
    out["inflight_max"] = -1 if min(imax) < 0 else max(imax)
    for k, f in (("oldest_hb", min), ("newest_hb", max)):
        v = [float(p[k]) for p in parts if p[k] == p[k]]
        out[k] = f(v) if v else float("nan")
    for k in HISTS:
        out[k] = np.sum([np.asarray(p[k], np.int64) for p in parts], axis=0).astype(np.int64)
    return out


def diff_summary(a, b):
    """The fields in which two summaries differ: {key: (a's, b's)} (for assertion messages)."""
    out = {}
    for k in SCALARS:
        x, y = a[k], b[k]
        if not (x == y or (isinstance(x, float) and isinstance(y, float) and x != x and y != y)):
            out[k] = (x, y)
    for k in HISTS:
        if not np.array_equal(np.asarray(a[k]), np.asarray(b[k])):
            out[k] = (np.asarray(a[k]).tolist(), np.asarray(b[k]).tolist())
    return out


def same_summary(a, b):
    """Field-for-field equality of two summaries (NaN equals NaN; extra keys are ignored)."""
    return not diff_summary(a, b)
