#!/usr/bin/env python3
"""Propagation latency of a benchmark workload, counted on the device
(include/gs_latency.h): how many hops until a message has reached 50 / 95 /
99 / 100 % of the hosts that take it.

    python scripts/latency_cdf.py --workload config4 [--peers N] [--steps K] [--warmup W]

Builds bench.py's engine with WithLatencyStats(), runs the warm-up rounds,
resets the per-topic table and runs the timed rounds.  Prints one JSON line per
topic group (p50 / p95 / p99 / max age in hops and the number of first
deliveries), one for all topics, and a last line with ms per round with the
statistics on and the two latency kernels' time per hop."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "go-libp2p-pubsub_amd"))
import bench  # noqa: E402
from pubsub_amd import WithLatencyStats, latency_quantiles  # noqa: E402

QS = (0.5, 0.95, 0.99, 1.0)


def group_line(workload, label, rows):
    row = rows.sum(axis=0)
    p50, p95, p99, top = (int(x) for x in latency_quantiles(row, QS))
    return {"workload": workload, "topics": label, "p50": p50, "p95": p95, "p99": p99, "max_age": top,
            "deliveries": int(row.sum()), "hist": row[:top + 1].tolist() if top >= 0 else []}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="config4", choices=["config4", "config3", "config5", "config2"])
    ap.add_argument("--peers", type=int, default=0, help="override the workload's peer count")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--topic-groups", type=int, default=4, help="lines per run: the topics in this many groups")
    ap.add_argument("--lib", default=None, help="timing experiments only: another build of the product library")
    args = ap.parse_args()
    wl = dict(bench.WORKLOADS[args.workload])
    if args.peers:
        wl["n"] = args.peers
    hps = bench.hops_per_step(wl)
    eng, _ = bench.build_engine(wl, args.warmup + args.steps + 1, 3, 0, extra=(WithLatencyStats(),), lib=args.lib)
    eng.step(1 + args.warmup * hps)
    eng.reset_latency_stats()
    d0 = eng.counters()["deliveries"]
    eng.set_profiling(True)
    eng.sync()
    t0 = time.perf_counter()
    eng.step(args.steps * hps)
    eng.sync()
    elapsed = time.perf_counter() - t0
    lat = eng.latency_kernel_stats()
    eng.set_profiling(False)
    hist = eng.latency_hist()
    assert hist.sum() == eng.counters()["deliveries"] - d0, "histogram total differs from the deliveries counter"
    T = wl["topics"]
    groups = max(1, min(args.topic_groups, T))
    if groups > 1:
        for g in range(groups):
            lo, hi = g * T // groups, (g + 1) * T // groups
            print(json.dumps(group_line(args.workload, f"{lo}..{hi - 1}", hist[lo:hi])))
    print(json.dumps(group_line(args.workload, "all", hist)))
    hops = args.steps * hps
    print(json.dumps({"workload": args.workload, "peers": wl["n"], "steps": args.steps, "warmup": args.warmup,
                      "latency_stats": True, "bins": int(hist.shape[1]),
                      "ms_per_step": round(elapsed / args.steps * 1e3, 3),
                      "lat_count_us_per_hop": round(lat["lat_count"][0] / hops * 1e3, 2),
                      "lat_fold_us_per_hop": round(lat["lat_fold"][0] / hops * 1e3, 2),
                      "lat_count_launches": lat["lat_count"][1],
                      "phase_a_reads": "frontier bitmaps" if eng.frontier_dense else "frontier lists"}))


if __name__ == "__main__":
    main()
