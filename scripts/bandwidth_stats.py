#!/usr/bin/env python3
"""Who pays, and for what?  Bandwidth statistics of a benchmark workload over
time, counted on the device (include/gs_bandwidth.h): per tick the egress and
ingress p50 / p95 / p99 / max per peer, the eager, pulled and overhead shares
of the bytes, then the cost per tick.

    python scripts/bandwidth_stats.py --workload config4 [--peers N] [--steps K] [--warmup W] [--period-hops P]

Builds the workload with pubsub_amd as scripts/mesh_health.py does (the
benchmark's config4 or config5), with RPC accounting on (messages of
--msg-size bytes) and a tick per heartbeat, runs the warm-up rounds and then
the timed rounds as one step().  Prints one JSON line per tick of the timed
rounds, and a last line with ms per round and, per tick, the three kernels' ms.
The quantiles are upper bin edges (bandwidth_quantiles: the smallest bound the
quantile lies below; -1 in the last, open bin); --fine bins by powers of 2
instead of 4.  --off runs the same rounds with the accounting alone (the last
line only), for the cost."""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "go-libp2p-pubsub_amd"))
from mesh_health import HOP, HOPS_PER_ROUND, WORKLOADS, build_engine  # noqa: E402
from pubsub_amd import (WithBandwidthStats, WithRPCAccounting, _abi, bandwidth_quantiles,  # noqa: E402
                        default_bandwidth_bounds)

QS = (0.5, 0.95, 0.99)


def tick_line(workload, k, row, bounds):
    line = {"workload": workload, "tick": k, "hop": row["hop"], "bytes": int(row["total"][0]),
            "rpcs": int(row["total_rpcs"])}
    q = bandwidth_quantiles(row["hist"][:, 0], bounds, QS)
    for d, name in enumerate(_abi.BW_DIRS):
        for i, p in enumerate(("p50", "p95", "p99")):
            line[f"{name}_{p}_below"] = int(q[d, i])
        line[f"{name}_max"] = int(row["max"][d, 0])
        line[f"{name}_max_node"] = int(row["argmax"][d, 0])
    total = max(int(row["total"][0]), 1)
    for c, name in enumerate(_abi.BW_CLASSES[1:], start=1):
        line[f"{name}_share"] = round(int(row["total"][c]) / total, 4)
    line["silent_peers"] = int(row["hist"][0, 0, 0]) if bounds[0] == 1 else None
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="config4", choices=sorted(WORKLOADS))
    ap.add_argument("--peers", type=int, default=0, help="override the workload's peer count")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--msg-size", type=int, default=1024, help="bytes of a message (WithRPCAccounting)")
    ap.add_argument("--period-hops", type=int, default=0, help="hops per tick (default: the heartbeat interval)")
    ap.add_argument("--fine", action="store_true", help="bounds at the powers of 2 from 64 B to 16 GiB")
    ap.add_argument("--off", action="store_true", help="the accounting alone: the same rounds, for the cost")
    ap.add_argument("--lib", default=None, help="timing experiments only: another build of the product library")
    args = ap.parse_args()
    wl = dict(WORKLOADS[args.workload])
    if args.peers:
        wl["n"] = args.peers
    period = args.period_hops or HOPS_PER_ROUND
    total = 1 + (args.warmup + args.steps) * HOPS_PER_ROUND
    bounds = [1] + [1 << s for s in range(6, 35)] if args.fine else default_bandwidth_bounds()
    extra = [WithRPCAccounting(args.msg_size)]
    if not args.off:
        extra.append(WithBandwidthStats(period * HOP, bounds=bounds, ticks=total // period + 1))
    eng = build_engine(wl, args.warmup + args.steps + 1, args.seed, extra=tuple(extra), lib=args.lib)
    eng.step(1 + args.warmup * HOPS_PER_ROUND)
    first = 0 if args.off else eng.bandwidth_ticks()
    if not args.off:
        eng.set_profiling(True)
    eng.sync()
    t0 = time.perf_counter()
    eng.step(args.steps * HOPS_PER_ROUND)
    eng.sync()
    elapsed = time.perf_counter() - t0
    last = {"workload": args.workload, "peers": wl["n"], "steps": args.steps, "warmup": args.warmup,
            "msg_size": args.msg_size, "bandwidth_stats": not args.off,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3)}
    if not args.off:
        ks = eng.bandwidth_kernel_stats()
        eng.set_profiling(False)
        taken = eng.bandwidth_ticks()
        for k in range(first, taken):
            print(json.dumps(tick_line(args.workload, k, eng.bandwidth_row(k), bounds)))
        n = max(1, taken - first)
        last.update(period_hops=period, ticks=taken - first,
                    ms_per_tick=round(sum(v[0] for v in ks.values()) / n, 3),
                    **{name + "_ms_per_tick": round(v[0] / n, 3) for name, v in ks.items()},
                    **{name + "_launches": v[1] for name, v in ks.items()})
    print(json.dumps(last))
    eng.close()


if __name__ == "__main__":
    main()
