#!/usr/bin/env python
"""The pool summary on the device against the only other way to get its numbers, same box.

For each case (W workers, about a sixth of them expired at the probe's clock, a queue of
those with free processes, a log of `head` entries with `live` of them in flight) it times
  device   GpuBalancer.pool_stats (fb_pool_stats): wall time of the call, and the kernels'
           device times from fb_timing_read (ps_slots, ps_log, ps_fold);
  host     read_state(with_log=True) and the numpy model (faasbal.poolstats), on a twin
           context loaded with the same state, so whatever one leg leaves behind on its
           context (a settled log, warm caches) does not help the other.
One warm-up and `--reps` timed repetitions per leg, alternating the legs; neither leg changes
the state.  The two legs' summaries must be equal, field for field.  Medians go to the JSON;
bytes per role are computed from the shapes (the layout of csrc/faasbal_layout.h; gathers
counted at the bytes they use, not the sectors they move) and divided by the kernel times.

    python tools/stats_probe.py --out profiles/stats_probe.json

``--world N``: the same cases on a shard group -- a LocalShardGroup of N rank contexts on this
one GPU, whose ranks run one after another (a real group's run side by side, one per GPU,
followed by one small gather).  Per repetition it times every rank's
ShardedBalancer.pool_stats_part (fb_pool_stats_shard: wall time of the call and its kernels'
device times) and the merge of the parts; the host leg is the group's read_state(with_log=True)
plus the model on a twin group.  Reported: the median over repetitions of a rank's call, of
the slowest rank's call (what a parallel group waits for), of the ranks' calls in sequence
plus the merge (what this one-GPU group takes), and of the host leg.

    python tools/stats_probe.py --world 2 --out profiles/stats_probe_shard_w2.json
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
from faasbal.poolstats import diff_summary, pool_stats_model  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s (spec)
NOW, TTE = 1000.0, 10.0
EDGES = (2.5, 5.0, 7.5, 10.0)
COUNTS_MAX_W = 1 << 17  # contexts of more slots keep no in-flight counts (inflight_max = -1)
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
    hb = NOW - rng.uniform(0.0, 12.0, W)
    return dict(reg=np.ones(W, np.uint8), free=free, hb=hb, epoch=np.zeros(W, np.uint32), queue=queue, log=log)


def role_bytes(head, live, W, Q, counts, window):
    slot_wgs, queue_wgs, log_wgs = -(-W // 1024), -(-Q // 1024), -(-(-(-head // 2048)) // 4)
    return {
        # reg, {free, queued}, hb (and the in-flight budget) in; the expired bitmap and a row per workgroup out
        "slots": W * (1 + 8 + 8 + (4 if counts else 0)) + W // 8 + 512 * slot_wgs,
        # the position's slot (and its tombstone word) in, free and hb gathered; a row out
        "queue": Q * (4 + (4 if window else 0) + 4 + 8) + 32 * queue_wgs,
        # the log in, a bitmap word gathered per entry; a row out
        "log": 4 * head + 8 * head + 16 * log_wgs,
        "fold": 512 * slot_wgs + 32 * queue_wgs + 16 * log_wgs + 512,
    }


def med(x):
    return float(np.median(x))


def run_case(name, head, live, W, reps):
    st = make_state(head, live, W)
    counts = W <= COUNTS_MAX_W
    g, twin = GpuBalancer(W, head, max_events=64), GpuBalancer(W, head, max_events=64)
    g.timing_enable(True)
    for b in (g, twin):
        b.load(st)
        b.sync()
        b.read_state(with_log=False)  # (load_state's copies from pageable memory have landed)
        b.selftest()
    g.timing_read()
    legs = {"device": [], "host": [], "host_read_only": []}
    kern = {}
    got = {}
    for rep in range(reps + 1):
        for leg in ("device", "host"):
            t0 = time.perf_counter()
            if leg == "device":
                s = g.pool_stats(NOW, TTE, EDGES)
                dt = time.perf_counter() - t0
            else:
                state = twin.read_state(with_log=True)
                t1 = time.perf_counter()
                s = pool_stats_model(state, NOW, TTE, EDGES, inflight_counts=counts)
                dt = time.perf_counter() - t0
                state = None
            times = g.timing_read() if leg == "device" else {}
            if rep == 0:  # warm-up; the summaries compared once
                got[leg] = s
                continue
            legs[leg].append(dt * 1e3)
            if leg == "host":
                legs["host_read_only"].append((t1 - t0) * 1e3)
            for k, (ms, n) in times.items():
                if k.startswith("ps_"):
                    kern.setdefault(k, []).append(ms)
    d = diff_summary(got["device"], got["host"])
    if d:
        raise SystemExit("%s: the device's summary and the host's differ: %r" % (name, d))
    Q = len(st["queue"])
    g.close()
    twin.close()
    by = role_bytes(head, live, W, Q, counts, window=W > COUNTS_MAX_W)
    kbytes = {"ps_slots": by["slots"] + by["queue"], "ps_log": by["log"], "ps_fold": by["fold"]}
    rows = {}
    for k, v in kern.items():
        ms = med(v)
        rows[k] = dict(ms=ms, bytes=kbytes[k], gbps=kbytes[k] / (ms * 1e-3) / 1e9 if ms > 0 else None,
                       hbm_peak_frac=kbytes[k] / (ms * 1e-3) / HBM_PEAK if ms > 0 else None)
    rows["sum_ms"] = sum(r["ms"] for r in rows.values())
    summary = {k: (v.tolist() if isinstance(v, np.ndarray) else None if isinstance(v, float) and v != v else v)
               for k, v in got["device"].items()}
    return dict(head=head, live=live, W=W, Q=Q, reps=reps,
                wall_ms={k: dict(median=med(v), min=float(min(v)), max=float(max(v))) for k, v in legs.items()},
                speedup_device_vs_host=med(legs["host"]) / med(legs["device"]),
                host_bytes_over_pcie=W * 21 + 4 * Q + 4 * head, device_bytes_over_pcie=512,
                role_bytes=by, kernels=rows, summary=summary)


def run_case_shard(name, head, live, W, reps, world):
    import torch  # noqa: F401  (loads the HIP runtime before the library)
    from faasbal.poolstats import merge_summaries
    from faasbal.sharded import LocalShardGroup

    st = make_state(head, live, W)
    # (a rank's log shard holds the live entries on its slots: at most `live`)
    grp, twin = (LocalShardGroup(world, W, live + 64, max_events=64) for _ in range(2))
    for g in (grp, twin):
        g.load(st)
        for b in g.bals:
            b.sync()
            b.read_state(with_log=False)
            b.selftest()
    for b in grp.bals:
        b.timing_enable(True)
        b.timing_read()
    legs = {"rank_call": [], "slowest_rank_call": [], "merge": [], "device_sequential": [], "host": [], "host_read_only": []}
    kern, got = {}, {}
    for rep in range(reps + 1):
        for leg in ("device", "host"):
            if leg == "device":
                t0 = time.perf_counter()
                calls, parts = [], []
                for b in grp.bals:
                    t1 = time.perf_counter()
                    parts.append(b.pool_stats_part(NOW, TTE, EDGES))
                    calls.append(time.perf_counter() - t1)
                t2 = time.perf_counter()
                s = merge_summaries([p for p, _ in parts], [q for _, q in parts])
                t3 = time.perf_counter()
                times = [b.timing_read() for b in grp.bals]
            else:
                t0 = time.perf_counter()
                state = twin.read_state(with_log=True)
                t1 = time.perf_counter()
                s = pool_stats_model(state, NOW, TTE, EDGES, inflight_counts=False)
                t3 = time.perf_counter()
                state = None
            if rep == 0:  # warm-up; the summaries compared once
                got[leg] = s
                continue
            if leg == "device":
                legs["rank_call"].extend(c * 1e3 for c in calls)
                legs["slowest_rank_call"].append(max(calls) * 1e3)
                legs["merge"].append((t3 - t2) * 1e3)
                legs["device_sequential"].append((t3 - t0) * 1e3)
                for tr in times:
                    for k, (ms, n) in tr.items():
                        if k.startswith("ps_"):
                            kern.setdefault(k, []).append(ms)
            else:
                legs["host"].append((t3 - t0) * 1e3)
                legs["host_read_only"].append((t1 - t0) * 1e3)
    d = diff_summary(got["device"], got["host"])
    if d:
        raise SystemExit("%s, world %d: the group's summary and the host's differ: %r" % (name, world, d))
    shard_logs = [int(b.read_state(with_log=False)["log_len"]) for b in grp.bals]
    grp.close()
    twin.close()
    summary = {k: (v.tolist() if isinstance(v, np.ndarray) else None if isinstance(v, float) and v != v else v)
               for k, v in got["device"].items()}
    return dict(head=head, live=live, W=W, Q=len(st["queue"]), reps=reps, world=world, shard_log_entries=shard_logs,
                wall_ms={k: dict(median=med(v), min=float(min(v)), max=float(max(v))) for k, v in legs.items()},
                speedup_slowest_rank_vs_host=med(legs["host"]) / med(legs["slowest_rank_call"]),
                speedup_sequential_vs_host=med(legs["host"]) / med(legs["device_sequential"]),
                kernels_per_rank_ms={k: med(v) for k, v in kern.items()},
                record_bytes_per_rank=8 * 65, summary=summary)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="configs2_like,configs3_like")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--world", type=int, default=0, help="N > 0: a shard group of N ranks on this GPU")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"hbm_peak_bytes_per_s": HBM_PEAK, "now": NOW, "tte": TTE, "age_edges": list(EDGES), "cases": {}}
    if a.world > 0:
        res["world"] = a.world
        for name in a.cases.split(","):
            c = res["cases"][name] = run_case_shard(name, reps=a.reps, world=a.world, **CASES[name])
            print(name, "world", a.world, json.dumps(c["wall_ms"]), json.dumps(c["kernels_per_rank_ms"]), flush=True)
        txt = json.dumps(res, indent=1)
        if a.out:
            with open(a.out, "w") as f:
                f.write(txt + "\n")
        print(json.dumps(res))
        return
    for name in a.cases.split(","):
        res["cases"][name] = run_case(name, reps=a.reps, **CASES[name])
        print(name, json.dumps(res["cases"][name]["wall_ms"]), "x%.1f" % res["cases"][name]["speedup_device_vs_host"],
              json.dumps(res["cases"][name]["kernels"]), flush=True)
    txt = json.dumps(res, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
