#!/usr/bin/env python
"""A shard group's log compaction on the device against the host path, same box, same group.

tools/compact_probe.py's sharded sibling, over a LocalShardGroup of N rank contexts on one GPU
(the bitmaps summed on the device, where RCCL would all-reduce them across GPUs: the
collective's own time is not measurable here).  For each case (tools/compact_probe.py's states:
a log of `head` entries, `live` of them in flight, W workers) and each N it times
  device   ShardGroup.compact_log (fb_log_compact_shard_mark, the summed bitmap,
           fb_log_compact_shard_apply on every rank): wall time with rank 0's kept list read back
           (what GpuPushDispatcher pays), wall time without it, and the kernels' device times
           from fb_timing_read, per rank (median over ranks and repetitions) and summed over
           the ranks;
  host     the path GpuPushDispatcher.compact_log takes on a group without the device path
           (and took on every group before it existed): read_state(with_log=True) of every
           rank, merged, searchsorted of the epochs over the kept sequences, load_state on
           every rank -- without the dispatcher's dict work, which both paths share.
One warm-up and `--reps` timed repetitions per leg, alternating the legs; every repetition
starts from the same freshly loaded state (the load is not timed).  After each leg one tick
(1000 tasks, no messages) is run and its `reruns` recorded, and the legs' merged states after
the warm-up are compared.  Medians go to the JSON.

    python tools/compact_shard_probe.py --out profiles/compact_shard_probe.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "distributed-faas_amd"))
sys.path.insert(0, HERE)

import torch  # noqa: E402,F401  (before the library: one HIP runtime per process)

from compact_probe import CASES, make_state, med  # noqa: E402
from faasbal.sharded import LocalShardGroup  # noqa: E402

KERNELS = ("lcs_flag", "lcs_mark", "lcs_count", "lcs_move", "lc_scan", "lc_copy")


def host_path(g):
    st = g.read_state(with_log=True)
    keep = np.flatnonzero(st["log"] >= 0).astype(np.int64)
    epoch = np.searchsorted(keep, st["epoch"].astype(np.int64), side="left").astype(np.uint32)
    g.load_state(st["reg"], st["free"], st["hb"], epoch, st["queue"], st["log"][keep])
    return keep


def run_case(name, world, head, live, W, reps):
    st = make_state(head, live, W)
    g = LocalShardGroup(world, W, head, max_events=64)
    for b in g.bals:
        b.timing_enable(True)
    legs = {"device": [], "device_no_kept": [], "host": []}
    kern = {k: [] for k in KERNELS}      # per rank and repetition (the leg with the kept list)
    kern_sum = {k: [] for k in KERNELS}  # summed over the ranks, per repetition
    reruns = {k: [] for k in legs}
    final = {}
    for rep in range(reps + 1):
        for leg in legs:
            g.load(st)
            for b in g.bals:
                b.read_state(with_log=False)  # (a blocking read: the load's copies have landed)
                b.timing_read()
            torch.cuda.synchronize()
            kept = None
            t0 = time.perf_counter()
            if leg == "host":
                kept = host_path(g)
            else:
                kept = g.compact_log(expect=live, want_kept=leg == "device")["kept"]
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            times = [b.timing_read() for b in g.bals]
            if rep == 0:
                final[leg] = (g.read_state(), kept)
            res = g.tick(1000.5, 10.0, n_pending=1000)["result"]
            if rep == 0:
                continue
            legs[leg].append(dt * 1e3)
            reruns[leg].append(int(res["reruns"]))
            if leg == "device":
                for k in KERNELS:
                    per = [t[k][0] for t in times if k in t]
                    kern[k].extend(per)
                    kern_sum[k].append(sum(per))
    for leg in ("device_no_kept", "host"):
        for k in ("reg", "free", "hb", "epoch", "queue", "log", "head"):
            if not np.array_equal(final["device"][0][k], final[leg][0][k], equal_nan=(k == "hb")):
                raise SystemExit("%s N=%d: %s differs between device and %s" % (name, world, k, leg))
    if not np.array_equal(final["device"][1], final["host"][1]):
        raise SystemExit("%s N=%d: kept lists differ" % (name, world))
    g.close()
    rows = {k: dict(per_rank_ms=med(v), all_ranks_ms=med(kern_sum[k])) for k, v in kern.items() if v}
    return dict(head=head, live=live, W=W, world=world, reps=reps, exchange_bytes=8 * 32 * (-(-head // 2048)),
                wall_ms={k: dict(median=med(v), min=float(min(v)), max=float(max(v))) for k, v in legs.items()},
                speedup_device_vs_host=med(legs["host"]) / med(legs["device"]),
                first_tick_reruns={k: dict(max=max(v), sum=sum(v)) for k, v in reruns.items()},
                kernels=dict(rows, sum_per_rank_ms=sum(r["per_rank_ms"] for r in rows.values()),
                             sum_all_ranks_ms=sum(r["all_ranks_ms"] for r in rows.values())),
                states_equal=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="configs2_like,configs3_like")
    ap.add_argument("--worlds", default="2,4,8")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"note": "one GPU, LocalShardGroup: the bitmap all-reduce is a device sum here, RCCL's time is not in these numbers",
           "cases": {}}
    for name in a.cases.split(","):
        for world in (int(x) for x in a.worlds.split(",")):
            key = "%s_n%d" % (name, world)
            res["cases"][key] = r = run_case(name, world, reps=a.reps, **CASES[name])
            print(key, json.dumps(r["wall_ms"]), "x%.1f" % r["speedup_device_vs_host"], json.dumps(r["first_tick_reruns"]),
                  flush=True)
            if a.out:  # (kept as the cases finish)
                with open(a.out, "w") as f:
                    f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
