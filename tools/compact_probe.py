#!/usr/bin/env python
"""Log compaction on the device against the host path, same box, same state.

For each case (a log of `head` entries, `live` of them in flight, W workers) it times
  device   GpuBalancer.compact_log (fb_log_compact): wall time with the kept list read back
           (what GpuPushDispatcher pays), wall time without it, and the kernels' device times
           from fb_timing_read (lc_flag, lc_scan, lc_move, lc_copy);
  host     the path GpuPushDispatcher.compact_log took before: read_state(with_log=True),
           searchsorted of the epochs over the kept sequences, load_state -- reimplemented here
           on the balancer, without the dispatcher's dict work (which both paths share).
One warm-up and `--reps` timed repetitions per leg, alternating the legs; every repetition
starts from the same loaded state (the load is not timed) and the two legs' resulting states
are compared once per case.  Medians go to the JSON; bytes per pass are computed from the
shapes (the layout of csrc/faasbal_layout.h) and divided by the kernel times.

    python tools/compact_probe.py --out profiles/compact_probe.json
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

HBM_PEAK = 8.0e12  # bytes/s (spec)
CASES = {
    "configs2_like": dict(head=1 << 20, live=469_000, W=1 << 16),
    "configs3_like": dict(head=1 << 24, live=7_600_000, W=1 << 20),
    "tiny": dict(head=5000, live=2200, W=300),  # rehearsal
}


def make_state(head, live, W, seed=0):
    rng = np.random.default_rng(seed)
    log = np.full(head, -1, np.int32)
    at = rng.choice(head, size=live, replace=False)
    log[at] = rng.integers(0, W, live).astype(np.int32)
    free = rng.integers(0, 8, W).astype(np.int32)
    queue = rng.permutation(np.flatnonzero(free > 0)).astype(np.int32)
    return dict(reg=np.ones(W, np.uint8), free=free, hb=np.full(W, 1000.0), epoch=np.zeros(W, np.uint32),
                queue=queue, log=log)


def host_path(g):
    st = g.read_state(with_log=True)
    keep = np.flatnonzero(st["log"] >= 0).astype(np.int64)
    epoch = np.searchsorted(keep, st["epoch"].astype(np.int64), side="left").astype(np.uint32)
    g.load_state(st["reg"], st["free"], st["hb"], epoch, st["queue"], st["log"][keep])
    return keep


def pass_bytes(head, live, W, kept):
    nt = -(-head // 2048)
    nw = 32 * nt
    return {
        "lc_flag": 4 * head + 12 * nw + 4 * nt,                 # log in; bitmap, word ranks, tile counts out
        "lc_scan": 8 * nt + 4,                                  # tile counts in, prefixes out
        "lc_move": 4 * head + 12 * nw + 4 * nt + (4 + (8 if kept else 0)) * live + 8 * W,
        "lc_copy": 8 * live,                                    # the survivors back into the log
    }


def med(x):
    return float(np.median(x))


def run_case(name, head, live, W, reps):
    st = make_state(head, live, W)
    g = GpuBalancer(W, head, max_events=64)
    g.timing_enable(True)
    legs = {"device": [], "device_no_kept": [], "host": []}
    kern = {True: {}, False: {}}
    final = {}
    for rep in range(reps + 1):
        for leg in legs:
            g.load(st)
            g.sync()
            # load_state's copies from pageable memory may still be landing when it returns: a
            # blocking read queues behind them, and a waited launch on the context's stream takes
            # whatever that stream still owes them, so the clock starts on an idle device
            g.read_state(with_log=False)
            g.selftest()
            g.timing_read()
            kept = None  # (the last leg's list is freed outside the clock)
            t0 = time.perf_counter()
            if leg == "host":
                kept = host_path(g)
            else:
                kept = g.compact_log(expect=live, want_kept=leg == "device")["kept"]
            g.sync()
            dt = time.perf_counter() - t0
            times = g.timing_read()
            if rep == 0:  # warm-up; the states compared once
                s = g.read_state()
                final[leg] = (s, kept)
                continue
            legs[leg].append(dt * 1e3)
            if leg != "host":
                for k, (ms, n) in times.items():
                    if k.startswith("lc_"):
                        kern[leg == "device"].setdefault(k, []).append(ms)
    for leg in ("device_no_kept", "host"):
        for k in ("reg", "free", "hb", "epoch", "queue", "log"):
            if not np.array_equal(final["device"][0][k], final[leg][0][k], equal_nan=(k == "hb")):
                raise SystemExit("%s: %s differs between device and %s" % (name, k, leg))
    if not np.array_equal(final["device"][1], final["host"][1]):
        raise SystemExit("%s: kept lists differ" % name)
    g.close()
    out = dict(head=head, live=live, W=W, reps=reps,
               wall_ms={k: dict(median=med(v), min=float(min(v)), max=float(max(v))) for k, v in legs.items()},
               speedup_device_vs_host=med(legs["host"]) / med(legs["device"]), kernels={})
    for kept in (True, False):
        by = pass_bytes(head, live, W, kept)
        rows = {}
        for k, v in kern[kept].items():
            ms = med(v)
            rows[k] = dict(ms=ms, bytes=by[k], gbps=by[k] / (ms * 1e-3) / 1e9 if ms > 0 else None,
                           hbm_peak_frac=by[k] / (ms * 1e-3) / HBM_PEAK if ms > 0 else None)
        rows["sum_ms"] = sum(r["ms"] for r in rows.values())
        out["kernels"]["with_kept" if kept else "no_kept"] = rows
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="configs2_like,configs3_like")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"hbm_peak_bytes_per_s": HBM_PEAK, "cases": {}}
    for name in a.cases.split(","):
        res["cases"][name] = run_case(name, reps=a.reps, **CASES[name])
        print(name, json.dumps(res["cases"][name]["wall_ms"]), "x%.1f" % res["cases"][name]["speedup_device_vs_host"],
              flush=True)
    txt = json.dumps(res, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
