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
    a = ap.parse_args()
    res = {}
    for name in a.sizes.split(","):
        sz = SIZES[name]
        st = make_state(sz["head"], sz["W"])
        g = GpuBalancer(sz["W"], sz["head"] + 4096, max_events=64)
        even = np.arange(0, sz["W"], 2)
        for frac in FRACTIONS:
            for masked in (False, True):
                # a mask of every other slot halves what a prefix holds: twice the prefix for the same count
                below = int(sz["head"] * frac * (2 if masked else 1))
                key = "%s_%g%s" % (name, frac, "_mask" if masked else "")
                res[key] = dict(head=sz["head"], W=sz["W"], below_seq=below, masked=masked,
                                **run_case(g, st, below, even if masked else None, a.reps))
                print(key, json.dumps(res[key]), flush=True)
        g.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
