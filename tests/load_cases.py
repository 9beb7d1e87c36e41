"""What a load installs (csrc/faasbal_load.h) -- TEST ONLY: the states, the numpy statement of
the image and the table of refusals that tests/test_load_host.py asks tests/load_probe.cpp
about and tests/test_gpu_load.py asks the device about.

A state is the caller's side of fb_load_shard: dict(base, n, reg, free, hb, epoch (or None),
queue, log_slot, log_seq (None on one GPU: the index), log_head).  A kind is the context's
facts (LoadKind): "hb" one GPU with in-flight counts, "win" one GPU with window buffers,
"deque", "shard" a rank of a 3-rank group.
"""
import numpy as np

from faasbal.sharded import shard_range, split_state

PART2 = 1 << 30
W, LOG, WORLD = 70, 200, 3  # 70 slots: no multiple of 64; ranks of 24, 24 and 22
KINDS = ("hb", "win", "deque", "shard")


def facts(kind, W_cap=W, W_global=W, log_cap=256, Wq_cap=None):
    """The context's facts of a kind, as create_ctx derives them."""
    deque, sharded = kind == "deque", kind == "shard"
    return dict(deque=int(deque), sharded=int(sharded), inflight=int(kind == "hb"), win=int(kind == "win"),
                W_cap=W_cap, W_global=W_global, Wq_cap=(3 * W_cap if deque else W_global) if Wq_cap is None else Wq_cap,
                log_cap=log_cap)


def global_state(seed, deque=False, n=W, log=LOG, null_epoch=False):
    """A whole table with everything a load has a rule for: an unregistered slot with log
    entries (3), a slot whose epoch lies above some of its entries and at or below others (5),
    completed entries, and on a deque a queue that repeats slot 7 three times."""
    rng = np.random.default_rng(seed)
    reg = (rng.random(n) < 0.8).astype(np.uint8)
    free = rng.integers(0, 5, n).astype(np.int32)
    hb = 1000.0 + rng.random(n) * 50
    epoch = np.where(rng.random(n) < 0.5, 0, rng.integers(0, log + 2, n)).astype(np.uint32)
    lg = rng.integers(0, max(n, 1), log).astype(np.int32) if n else np.zeros(0, np.int32)
    lg[rng.random(len(lg)) < 0.25] = -1
    if n > 7 and log >= 160:
        reg[3], reg[5], reg[7] = 0, 1, 1
        epoch[5] = 100
        lg[[10, 120]] = 3
        lg[[20, 99, 100, 150]] = 5
        lg[[0, 199]] = -1
    live = np.nonzero(reg)[0]
    queue = rng.permutation(live)[: len(live) * 2 // 3].astype(np.int32)
    if deque and n > 7:
        queue = np.concatenate([queue[queue != 7], [7, 7], rng.permutation(live)[:9], [7]]).astype(np.int32)
        assert (queue == 7).sum() >= 3
    return dict(reg=reg, free=free, hb=hb, epoch=None if null_epoch else epoch, queue=queue, log=lg)


def local_state(st, kind, rank=0):
    """The caller's side of the load of st on a context of this kind (a shard: rank's part)."""
    if kind == "shard":
        sh = split_state(st, WORLD, rank)
        if st.get("epoch") is None:
            sh["epoch"] = None
        return sh
    n = len(st["reg"])
    return dict(base=0, n=n, reg=st["reg"], free=st["free"], hb=st["hb"], epoch=st.get("epoch"), queue=st["queue"],
                log_slot=st["log"], log_seq=None, log_head=len(st["log"]))


def as_one_rank_shard(a):
    """A one-GPU load as the shard case it is: the index for the sequence, log_head = log_len."""
    return dict(a, log_seq=np.arange(len(a["log_slot"]), dtype=np.uint32), log_head=len(a["log_slot"]))


def image(f, a):
    """The image of an accepted load, stated independently of the header; None: the kind has
    no such array."""
    base, n = a["base"], a["n"]
    reg = np.asarray(a["reg"][:n]) != 0
    free = np.asarray(a["free"][:n], np.int64)
    hb_in = np.asarray(a["hb"][:n], np.float64)
    epoch = np.zeros(n, np.int64) if a["epoch"] is None else np.asarray(a["epoch"][:n], np.int64)
    q = np.asarray(a["queue"], np.int64)
    own = (q >= base) & (q < base + n)
    lq = q[own] - base
    inq = np.zeros(n, np.int64)
    inq[lq] = 1
    log = np.asarray(a["log_slot"], np.int64).copy()
    seq = np.arange(len(log)) if a["log_seq"] is None else np.asarray(a["log_seq"], np.int64)
    named = log >= 0
    ls = np.where(named, log - base, 0)
    if not f["deque"]:  # (a deque keeps every entry)
        log[named & (~reg[ls] | (seq < epoch[ls]))] = -1
    out = dict(reg=reg.astype(np.int64), hb=np.where(reg, hb_in, np.nan), epoch=epoch, free=free, inq=inq, log=log,
               maxc=max([1] + free[lq].tolist()), pos=None, qfree=None, qhb=None, tokcnt=None, qrank=None, bud=None)
    if f["win"]:
        out["pos"] = np.zeros(n, np.int64)
        out["pos"][lq] = np.nonzero(own)[0]
    if not f["sharded"]:
        out["qfree"], out["qhb"] = free[q], hb_in[q]
    if f["deque"]:
        out["tokcnt"] = np.bincount(q, minlength=n)[:n] if n else np.zeros(0, np.int64)
        out["qrank"] = np.array([(q[: i + 1] == s).sum() | PART2 for i, s in enumerate(q)], np.int64)
    if f["inflight"]:
        live = np.bincount(log[log >= 0] - base, minlength=n)[:n] if n else np.zeros(0, np.int64)
        out["bud"] = np.where(reg, live + free, 0)
    return out


# --------------------------------------------------------------------------- the refusals
def tiny(kind):
    """A minimal accepted state of the kind and its facts: two slots, one queued, one log entry
    (a shard: global slots [2, 4) of 6)."""
    f = facts(kind, W_cap=4, W_global=6 if kind == "shard" else 4, log_cap=8, Wq_cap=6 if kind == "deque" else None)
    b = 2 if kind == "shard" else 0
    a = dict(base=b, n=2, reg=np.array([1, 1], np.uint8), free=np.array([1, 1], np.int32), hb=np.array([1.0, 1.0]),
             epoch=None, queue=np.array([b], np.int32), log_slot=np.array([b], np.int32),
             log_seq=np.array([0], np.uint32) if kind == "shard" else None, log_head=1)
    return f, a


NULL = "null"  # an array argument replaced by a null pointer, its count kept


def _i(*v):
    return np.array(v, np.int32)


# (kind, condition, what the tiny state is changed to, the message).  One row at least for every
# fail(...) of fb_load_state and fb_load_shard before the check moved into the header, then the
# null arrays.  qlen / llen override the counts the arrays would give.
REFUSALS = [
    ("hb", "n_workers", dict(n=5), "n_workers 5 outside [0, 4]"),
    ("hb", "n_workers", dict(n=-1), "n_workers -1 outside [0, 4]"),
    ("deque", "n_workers", dict(n=5), "n_workers 5 outside [0, 4]"),
    ("hb", "log_len", dict(llen=9), "log_len 9 exceeds capacity"),
    ("win", "log_len", dict(llen=-1), "log_len -1 exceeds capacity"),
    ("hb", "queue_len", dict(qlen=3), "queue_len 3"),
    ("hb", "queue_len", dict(qlen=-1), "queue_len -1"),
    ("deque", "queue_len", dict(qlen=7), "queue_len 7"),
    ("shard", "queue_len", dict(qlen=7), "queue_len 7"),
    ("hb", "queue_entry", dict(queue=_i(2)), "queue[0] = 2 is out of range, unregistered or duplicated"),
    ("hb", "queue_entry", dict(queue=_i(-1)), "queue[0] = -1 is out of range, unregistered or duplicated"),
    ("win", "queue_entry", dict(queue=_i(1), reg=np.array([1, 0], np.uint8)),
     "queue[0] = 1 is out of range, unregistered or duplicated"),
    ("hb", "queue_entry", dict(queue=_i(1, 1)), "queue[1] = 1 is out of range, unregistered or duplicated"),
    ("deque", "queue_entry", dict(queue=_i(0, 0, 2)), "queue[2] = 2 is out of range, unregistered or duplicated"),
    ("hb", "log_slot", dict(log_slot=_i(2)), "log_slot[0] = 2 out of range"),
    ("deque", "log_slot", dict(log_slot=_i(0, -2)), "log_slot[1] = -2 out of range"),
    ("shard", "slot_range", dict(base=5), "slot range [5, 5 + 2) outside the 6-slot table"),
    ("shard", "slot_range", dict(n=5), "slot range [2, 2 + 5) outside the 6-slot table"),
    ("shard", "slot_range", dict(base=-1), "slot range [-1, -1 + 2) outside the 6-slot table"),
    ("shard", "log_len_head", dict(log_head=0), "log_len 1 / log_head 0"),
    ("shard", "log_len_head", dict(log_head=1 << 31), "log_len 1 / log_head 2147483648"),
    ("shard", "log_len_head", dict(llen=9, log_head=9), "log_len 9 / log_head 9"),
    ("shard", "queue_entry_shard", dict(queue=_i(6)), "queue[0] = 6 is out of range or duplicated"),
    ("shard", "queue_entry_shard", dict(queue=_i(0, 2, 0)), "queue[2] = 0 is out of range or duplicated"),
    ("shard", "queue_unregistered", dict(queue=_i(0, 3), reg=np.array([1, 0], np.uint8)), "queue[1] = 3 is not registered"),
    ("shard", "log_slot_shard", dict(log_slot=_i(1)), "log_slot[0] = 1 is not one of this rank's slots"),
    ("shard", "log_slot_shard", dict(log_slot=_i(4)), "log_slot[0] = 4 is not one of this rank's slots"),
    ("shard", "log_slot_shard", dict(log_slot=_i(-2)), "log_slot[0] = -2 is not one of this rank's slots"),
    ("shard", "log_seq", dict(log_seq=np.array([1], np.uint32)), "log_seq must ascend below log_head (entry 0)"),
    ("shard", "log_seq", dict(log_slot=_i(2, 3), log_seq=np.array([1, 1], np.uint32), log_head=5),
     "log_seq must ascend below log_head (entry 1)"),
    # a null array with a count that says it is read
    ("hb", "null_array", dict(reg=NULL), "registered is null with n_workers = 2"),
    ("deque", "null_array", dict(free=NULL), "free_processes is null with n_workers = 2"),
    ("shard", "null_array", dict(hb=NULL), "last_heartbeat is null with n_workers = 2"),
    ("hb", "null_array", dict(queue=NULL), "queue is null with queue_len = 1"),
    ("shard", "null_array", dict(queue=NULL), "queue is null with queue_len = 1"),
    ("win", "null_array", dict(log_slot=NULL), "log_slot is null with log_len = 1"),
    ("shard", "null_array", dict(log_seq=NULL), "log_seq is null with log_len = 1"),
    # two offences: the earlier condition is the one named
    ("hb", "n_workers", dict(n=5, queue=_i(9)), "n_workers 5 outside [0, 4]"),
    ("shard", "log_slot_shard", dict(log_slot=_i(0), log_seq=np.array([7], np.uint32)),
     "log_slot[0] = 0 is not one of this rank's slots"),
    ("shard", "null_array", dict(reg=NULL, base=5), "registered is null with n_workers = 2"),
]
TWICE = REFUSALS[-3:]
# the fail(...)s of the two loaders before: 5 in fb_load_state, 7 in fb_load_shard
N_PARENT_FAILS = 12

# What stays accepted right beside a refusal: the differences between the kinds.
ACCEPTED = [
    ("deque", dict(queue=_i(0, 0, 1))),                 # a deque may repeat a slot
    ("deque", dict(queue=_i(0, 1, 0, 1, 1))),           # ... beyond n_workers entries
    ("shard", dict(queue=_i(0, 5, 2))),                 # other ranks' slots, registered or not
    ("shard", dict(log_slot=_i(-1))),                   # completed
    ("hb", dict(log_slot=_i(1, -1, 0))),
    ("hb", dict(n=0, queue=None, log_slot=None, reg=NULL, free=NULL, hb=NULL)),  # nothing is read
    ("shard", dict(n=0, queue=None, log_slot=None, log_seq=None, reg=NULL, free=NULL, hb=NULL, log_head=0)),
    ("hb", dict(log_seq=NULL)),                          # one GPU: the index is the sequence
]


def offending(kind, change):
    """(facts, state, counts) of a tiny state with the row's change applied."""
    f, a = tiny(kind)
    was = dict(qlen=len(a["queue"]), llen=len(a["log_slot"]))
    a.update({k: v for k, v in change.items() if k not in was})
    counts = {}
    for key, k in (("queue", "qlen"), ("log_slot", "llen")):
        if a[key] is None:  # (no entries, no array)
            a[key] = NULL
            was[k] = 0
        counts[k] = change.get(k, was[k] if a[key] is NULL else len(a[key]))
    return f, a, counts
