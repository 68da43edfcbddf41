#!/usr/bin/env python3
"""Scores and mesh health of a benchmark workload over time, taken on the
device (include/gs_inspect.h): per tick, how many peer scores sit below each
threshold and the mesh-degree quantiles per topic group.

    python scripts/score_inspect.py --workload config4 [--peers N] [--steps K] [--warmup W] [--period-hops P]

Builds bench.py's engine with WithPeerScoreInspect (a tick per heartbeat by
default), runs the warm-up rounds and then the timed rounds as one step().
Prints one JSON line per tick of the timed rounds and topic group, and a last
line with ms per round and the three inspection passes' ms per tick.  --off
runs the same rounds without inspection (the last line only), for the cost."""
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
from pubsub_amd import WithPeerScoreInspect, default_inspect_bounds, eth2_thresholds, latency_quantiles  # noqa: E402

QS = (0.05, 0.5, 0.95)


def tick_lines(workload, k, row, bounds, groups):
    hist, deg = row["score_hist"], row["mesh_deg"]
    below = np.cumsum(hist)[:-1]
    out = {"workload": workload, "tick": k, "hop": row["hop"], "edges": int(hist.sum()),
           "below": {repr(float(b)): int(c) for b, c in zip(bounds, below)}}
    T = deg.shape[0]
    lines = []
    for g in range(groups):
        lo, hi = g * T // groups, (g + 1) * T // groups
        d = deg[lo:hi].sum(axis=0)
        p5, p50, p95 = (int(x) for x in latency_quantiles(d, QS))
        nz = np.flatnonzero(d)
        lines.append(dict(out, topics=f"{lo}..{hi - 1}", mesh_deg_p5=p5, mesh_deg_p50=p50, mesh_deg_p95=p95,
                          mesh_deg_min=int(nz[0]), mesh_deg_max=int(nz[-1]), nodes_without_mesh=int(d[0])))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="config4", choices=["config4", "config3", "config5"])
    ap.add_argument("--peers", type=int, default=0, help="override the workload's peer count")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--period-hops", type=int, default=0, help="hops per tick (default: the heartbeat interval)")
    ap.add_argument("--topic-groups", type=int, default=4, help="lines per tick: the topics in this many groups")
    ap.add_argument("--off", action="store_true", help="no inspection: the same rounds, for the cost")
    ap.add_argument("--lib", default=None, help="timing experiments only: another build of the product library")
    args = ap.parse_args()
    wl = dict(bench.WORKLOADS[args.workload])
    if args.peers:
        wl["n"] = args.peers
    hps = bench.hops_per_step(wl)
    period = args.period_hops or bench.HOPS_PER_ROUND  # HeartbeatInterval 1 s = 10 hops of 100 ms
    bounds = default_inspect_bounds(eth2_thresholds())
    total = 1 + (args.warmup + args.steps) * hps
    extra = () if args.off else (WithPeerScoreInspect(None, period * 100 * bench.Millisecond, bounds=bounds,
                                                      ticks=total // period + 1),)
    eng, _ = bench.build_engine(wl, args.warmup + args.steps + 1, 3, 0, extra=extra, lib=args.lib)
    eng.step(1 + args.warmup * hps)
    first = 0 if args.off else eng.inspect_ticks()
    eng.set_profiling(True)
    eng.sync()
    t0 = time.perf_counter()
    eng.step(args.steps * hps)
    eng.sync()
    elapsed = time.perf_counter() - t0
    last = {"workload": args.workload, "peers": wl["n"], "steps": args.steps, "warmup": args.warmup,
            "inspect": not args.off, "lib": os.path.basename(os.path.dirname(args.lib)) if args.lib else "this",
            "ms_per_step": round(elapsed / args.steps * 1e3, 3)}
    if not args.off:
        ks = eng.inspect_kernel_stats()
        eng.set_profiling(False)
        taken = eng.inspect_ticks()
        groups = max(1, min(args.topic_groups, wl["topics"]))
        for k in range(first, taken):
            for line in tick_lines(args.workload, k, eng.inspect_row(k), bounds, groups):
                print(json.dumps(line))
        n = max(1, taken - first)
        last.update(period_hops=period, ticks=taken - first,
                    **{name + "_ms_per_tick": round(ks[name][0] / n, 3) for name in ks},
                    **{name + "_launches": ks[name][1] for name in ks})
    print(json.dumps(last))


if __name__ == "__main__":
    main()
