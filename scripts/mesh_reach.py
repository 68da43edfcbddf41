#!/usr/bin/env python3
"""If a host published now, whom would eager push reach, and in how many hops?
Mesh reach of a benchmark workload over time, counted on the device
(include/gs_mesh_reach.h): per tick and topic group the targets reached and not
reached from random publishers and the hops the push needs to 50 / 95 / 100 %
of the targets, beside the hops the run's real messages took
(include/gs_latency.h, scripts/latency_cdf.py's figures); then the cost per tick.

    python scripts/mesh_reach.py --workload config4 [--peers N] [--steps K] [--warmup W] [--sources S]

Builds the workload as scripts/mesh_health.py does (config4: 64 topics, every
host subscribed; config5: one topic, 20 % Sybils, the honest hosts as `nodes`
and as sources) with a tick per heartbeat and the latency statistics on, runs
the warm-up rounds and then the timed rounds as one step().  Prints one JSON
line per tick of the timed rounds and topic group, one line per topic group
with the predicted and the measured hops over the timed rounds, and a last line
with ms per round and, per tick, the kernels' ms, the passes, the levels and
the bytes moved.  --off runs the same rounds without mesh reach (the last line
only), for the cost."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "go-libp2p-pubsub_amd"))
from mesh_health import HOP, HOPS_PER_ROUND, WORKLOADS, build_engine, sybils  # noqa: E402
from pubsub_amd import WithLatencyStats, WithMeshReach, latency_quantiles  # noqa: E402

QS = (0.5, 0.95, 1.0)


def predicted_hops(hist, unreached):
    """Hops until eager push has reached 50 / 95 / 100 % of the targets: over
    depth_hist summed over sources, topics and ticks, the targets never reached
    counted in the total (-1: that share is never reached; 63 stands for every
    depth >= 63)."""
    cum, total = np.cumsum(hist), int(hist.sum() + unreached)
    out = []
    for q in QS:
        need = -(-round(q * 100) * total // 100)  # ceil(q x total), exactly
        hit = np.flatnonzero(cum >= need)
        out.append(int(hit[0]) if total and len(hit) else -1)
    return out


def tick_lines(workload, k, row, groups):
    T = row["reached"].shape[1]
    lines = []
    for g in range(groups):
        lo, hi = g * T // groups, (g + 1) * T // groups
        p50, p95, p100 = predicted_hops(row["depth_hist"][:, lo:hi].sum(axis=(0, 1)), row["unreached"][:, lo:hi].sum())
        lines.append({"workload": workload, "tick": k, "hop": row["hop"], "topics": f"{lo}..{hi - 1}",
                      "reached": int(row["reached"][:, lo:hi].sum()), "unreached": int(row["unreached"][:, lo:hi].sum()),
                      "ecc_max": int(row["ecc"][:, lo:hi].max()), "ecc_min": int(row["ecc"][:, lo:hi].min()),
                      "hops_p50": p50, "hops_p95": p95, "hops_p100": p100})
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="config4", choices=sorted(WORKLOADS))
    ap.add_argument("--peers", type=int, default=0, help="override the workload's peer count")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--sources", type=int, default=64, help="random publishers (honest ones at config5), at most 256")
    ap.add_argument("--period-hops", type=int, default=0, help="hops per tick (default: the heartbeat interval)")
    ap.add_argument("--topic-groups", type=int, default=4, help="lines per tick: the topics in this many groups")
    ap.add_argument("--off", action="store_true", help="no mesh reach: the same rounds, for the cost")
    ap.add_argument("--lib", default=None, help="timing experiments only: another build of the product library")
    args = ap.parse_args()
    wl = dict(WORKLOADS[args.workload])
    if args.peers:
        wl["n"] = args.peers
    period = args.period_hops or HOPS_PER_ROUND
    total = 1 + (args.warmup + args.steps) * HOPS_PER_ROUND
    mask = ~sybils(wl["n"], args.seed) if wl.get("adversarial") else None
    pool = np.arange(wl["n"]) if mask is None else np.flatnonzero(mask)
    sources = np.random.default_rng(args.seed + 23).choice(pool, args.sources, replace=False)
    extra = [WithLatencyStats()]
    if not args.off:
        extra.append(WithMeshReach(period * HOP, sources, nodes=mask, ticks=total // period + 1))
    eng = build_engine(wl, args.warmup + args.steps + 1, args.seed, extra=tuple(extra), lib=args.lib)
    eng.step(1 + args.warmup * HOPS_PER_ROUND)
    first = 0 if args.off else eng.mesh_reach_ticks()
    eng.reset_latency_stats()
    eng.set_profiling(True)
    eng.sync()
    t0 = time.perf_counter()
    eng.step(args.steps * HOPS_PER_ROUND)
    eng.sync()
    elapsed = time.perf_counter() - t0
    last = {"workload": args.workload, "peers": wl["n"], "steps": args.steps, "warmup": args.warmup,
            "mesh_reach": not args.off, "sources": 0 if args.off else len(sources),
            "hosts": "all" if mask is None else f"{int(mask.sum())} honest",
            "ms_per_step": round(elapsed / args.steps * 1e3, 3)}
    T = wl["topics"]
    groups = max(1, min(args.topic_groups, T))
    measured = eng.latency_hist()
    if not args.off:
        ks = eng.mesh_reach_kernel_stats()
        eng.set_profiling(False)
        taken = eng.mesh_reach_ticks()
        rows = [eng.mesh_reach_row(k) for k in range(first, taken)]
        for k, row in zip(range(first, taken), rows):
            for line in tick_lines(args.workload, k, row, groups):
                print(json.dumps(line))
        hist = sum(row["depth_hist"] for row in rows).sum(axis=0)  # [T, 64]
        unreached = sum(row["unreached"] for row in rows).sum(axis=0)  # [T]
        for g in range(groups):
            lo, hi = g * T // groups, (g + 1) * T // groups
            got = [int(x) for x in latency_quantiles(measured[lo:hi].sum(axis=0), QS)]
            print(json.dumps({"workload": args.workload, "topics": f"{lo}..{hi - 1}",
                              "predicted_hops_p50_p95_p100": predicted_hops(hist[lo:hi].sum(axis=0), unreached[lo:hi].sum()),
                              "measured_hops_p50_p95_p100": got,
                              "first_deliveries_measured": int(measured[lo:hi].sum())}))
        n = max(1, taken - first)
        kernels = [name for name in ks if name not in ("passes", "levels", "bytes")]
        last.update(period_hops=period, ticks=taken - first,
                    ms_per_tick=round(sum(ks[name][0] for name in kernels) / n, 3),
                    **{name + "_ms_per_tick": round(ks[name][0] / n, 3) for name in kernels},
                    **{name + "_launches": ks[name][1] for name in kernels},
                    passes_per_tick=round(ks["passes"] / n, 2), levels_per_tick=round(ks["levels"] / n, 2),
                    mbytes_per_tick=round(ks["bytes"] / n / 1e6, 1))
    print(json.dumps(last))
    eng.close()


if __name__ == "__main__":
    main()
