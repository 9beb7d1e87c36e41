#!/usr/bin/env python
"""fb_log_reclaim on the device against the host path, same box, same state.

For each case (a log of `head` entries, all in flight, W workers; a fraction of them taken
back, by a prefix alone or by a prefix and a slot mask that halves it) it times
  device   GpuBalancer.reclaim (fb_log_reclaim): wall time with the two lists read back (what
           GpuPushDispatcher pays, the first call that learns the count included), and the
           kernels' device times per launch from fb_timing_read (lr_flag, lc_scan, lr_take);
  host     the path a dispatcher without the call would take: read_state(with_log=True), the
           rule in numpy, load_state.
One warm-up and `--reps` timed repetitions per leg, alternating the legs; every repetition
starts from the same loaded state (the load is not timed) and the two legs' resulting states
and in-flight counts are compared once per case.  Medians go to the JSON.

    python tools/reclaim_probe.py --out profiles/reclaim_probe.json

With ``--world N[,N..]`` the same cases run on a shard group instead (LocalShardGroup: N rank
contexts on this one GPU, fb_log_reclaim_shard behind ShardGroup.reclaim -- every rank counts,
then every rank takes) against the group's host path (ShardGroup.read_state, the rule in numpy,
ShardGroup.load_state); the kernels' times are per rank and launch (the mean and the maximum
over the ranks).  A group's collectives across GPUs are not in these numbers.

    python tools/reclaim_probe.py --world 2,8 --out profiles/reclaim_shard_probe.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "distributed-faas_amd"))

from faasbal import GpuBalancer  # noqa: E402

SIZES = {"1M": dict(head=1 << 20, W=1 << 16), "16M": dict(head=1 << 24, W=1 << 16), "tiny": dict(head=5000, W=300)}
FRACTIONS = (0.01, 0.5)


def make_state(head, W, seed=0):
    rng = np.random.default_rng(seed)
    free = rng.integers(0, 8, W).astype(np.int32)
    return dict(reg=np.ones(W, np.uint8), free=free, hb=np.full(W, 1000.0), epoch=np.zeros(W, np.uint32),
                queue=rng.permutation(np.flatnonzero(free > 0)).astype(np.int32),
                log=rng.integers(0, W, head).astype(np.int32))


def host_path(g, below, mask):
    st = g.read_state(with_log=True)
    log = st["log"]
    s = np.maximum(log, 0)
    take = (log >= 0) & (st["reg"][s] != 0) & (np.arange(len(log)) >= st["epoch"][s].astype(np.int64))
    take[below:] = False
    if mask is not None:
        take &= mask[s] != 0
    seq = np.flatnonzero(take)
    slot = log[seq]
    log = log.copy()
    log[seq] = -1
    g.load_state(st["reg"], st["free"], st["hb"], st["epoch"], st["queue"], log)
    return seq, slot


def med(x):
    return float(np.median(x))


class _Group:
    """A LocalShardGroup behind the calls run_case makes of a GpuBalancer.  The untimed loads
    install shards split once (fb_load_shard, as ShardedBalancer.load does)."""

    def __init__(self, world, W, head):
        from faasbal.sharded import LocalShardGroup
        self.g = LocalShardGroup(world, W, 2 * head // world + 65536, max_events=64)
        self.world, self.shards = world, None

    def load(self, st):
        from faasbal.balancer import _p
        from faasbal.sharded import split_state
        if self.shards is None or self.shards[0] is not st:
            q = np.asarray(st["queue"], np.int64)
            hint = max(1, min(int(np.asarray(st["free"])[q].max()) if len(q) else 1, 1 << 30))
            self.shards = (st, [split_state(st, self.world, r) for r in range(self.world)], hint)
        for b, sh in zip(self.g.bals, self.shards[1]):
            b._chk(b.lib.fb_load_shard(b.h, sh["base"], sh["n"], _p(sh["reg"]), _p(sh["free"]), _p(sh["hb"]),
                                       _p(sh["epoch"]), _p(sh["queue"]), len(sh["queue"]), _p(sh["log_slot"]),
                                       _p(sh["log_seq"]), len(sh["log_slot"]), sh["log_head"]))
            b._chk(b.lib.fb_set_round_hint(b.h, self.shards[2]))
            b.n_workers = sh["n"]

    def sync(self):
        for b in self.g.bals:
            b.sync()

    def reclaim(self, below, slots):
        return self.g.reclaim(below, slots)

    def read_state(self, with_log=True):
        return self.g.read_state(with_log)

    def load_state(self, *a):
        return self.g.load_state(*a)

    def inflight(self):  # (sharded contexts keep no per-slot counts)
        return np.zeros(0, np.uint32)

    def timing_enable(self, on=True):
        for b in self.g.bals:
            b.timing_enable(on)

    def timing_read(self):
        """Per kernel: (the mean over the ranks of a rank's time per launch, 1), and under
        ``<name>.max`` the slowest rank's."""
        per = {}
        for b in self.g.bals:
            for k, (ms, cnt) in b.timing_read().items():
                per.setdefault(k, []).append(ms / max(cnt, 1))
        out = {k: (float(np.mean(v)), 1) for k, v in per.items()}
        out.update({k + ".max": (float(np.max(v)), 1) for k, v in per.items()})
        return out

    def close(self):
        self.g.close()


def run_case(g, st, below, slots, reps):
    mask = None
    if slots is not None:
        mask = np.zeros(len(st["reg"]), np.uint8)
        mask[slots] = 1
    dev, host, kern = [], [], {}
    ends = {}
    for r in range(reps + 1):
        for leg in ("device", "host"):
            g.load(st)
            g.sync()
            t0 = time.perf_counter()
            out = g.reclaim(below, slots) if leg == "device" else host_path(g, below, mask)
            dt = (time.perf_counter() - t0) * 1e3
            if r == 0:
                n = out["n"] if leg == "device" else len(out[0])
                ends[leg] = (n, g.read_state(), g.inflight())
                continue
            (dev if leg == "device" else host).append(dt)
    # the kernels' device times, in repetitions of their own (event timing is off in the wall-time ones)
    g.timing_enable(True)
    for r in range(reps):
        g.load(st)
        g.sync()
        g.timing_read()
        g.reclaim(below, slots)
        for k, (ms, cnt) in g.timing_read().items():
            kern.setdefault(k, []).append(ms / max(cnt, 1))
    g.timing_enable(False)
    (nd, sd, fd), (nh, sh, fh) = ends["device"], ends["host"]
    same = nd == nh and all(np.array_equal(sd[k], sh[k]) for k in ("reg", "free", "epoch", "queue", "log")) \
        and np.array_equal(fd, fh)
    return dict(n_reclaimed=int(nd), device_ms=med(dev), host_ms=med(host), speedup=med(host) / med(dev),
                device_ms_all=[round(x, 3) for x in dev], host_ms_all=[round(x, 3) for x in host],
                kernels_ms={k: med(v) for k, v in sorted(kern.items())}, same_state=bool(same))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="1M,16M")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--world", default=None, help="shard groups of N ranks on this GPU, e.g. 2,8 (default: one GPU)")
    a = ap.parse_args()
    res = {}
    worlds = [None] if a.world is None else [int(w) for w in a.world.split(",")]
    for name in a.sizes.split(","):
        sz = SIZES[name]
        st = make_state(sz["head"], sz["W"])
        for world in worlds:
            g = GpuBalancer(sz["W"], sz["head"] + 4096, max_events=64) if world is None else _Group(world, sz["W"], sz["head"])
            even = np.arange(0, sz["W"], 2)
            for frac in FRACTIONS:
                for masked in (False, True):
                    # a mask of every other slot halves what a prefix holds: twice the prefix for the same count
                    below = int(sz["head"] * frac * (2 if masked else 1))
                    key = "%s_%g%s%s" % (name, frac, "_mask" if masked else "", "" if world is None else "_N%d" % world)
                    res[key] = dict(head=sz["head"], W=sz["W"], below_seq=below, masked=masked,
                                    **({} if world is None else {"world": world}),
                                    **run_case(g, st, below, even if masked else None, a.reps))
                    print(key, json.dumps(res[key]), flush=True)
            g.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
