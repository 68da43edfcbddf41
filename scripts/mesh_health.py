#!/usr/bin/env python3
"""Is each topic's mesh one piece?  Mesh health of a benchmark workload over
time, counted on the device (include/gs_mesh_health.h): per tick and topic
group the components, the largest one, and the isolated, one-sided, outside and
eclipsed counts; then the cost per tick.

    python scripts/mesh_health.py --workload config4 [--peers N] [--steps K] [--warmup W] [--period-hops P]

Builds the workload with pubsub_amd (the benchmark's config4: 64 topics, every
host subscribed; config5: one topic, 20 % Sybils, and the mask of the honest
hosts as `nodes`) with a tick per heartbeat, runs the warm-up rounds and then
the timed rounds as one step().  Prints one JSON line per tick of the timed
rounds and topic group, and a last line with ms per round and, per tick, the
four passes' ms, the label iterations and the bytes moved.  --off runs the same
rounds without mesh health (the last line only), for the cost; --all-hosts
counts config5's Sybils too."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "go-libp2p-pubsub_amd"))
from pubsub_amd import (GS_BEHAVE_GRAFT_SPAM, GS_BEHAVE_IHAVE_SPAM, GS_BEHAVE_IWANT_SPAM, GS_MSG_PHANTOM,  # noqa: E402
                        GS_MSG_REJECT, DefaultPeerGaterParams, Millisecond, NewGossipSub, WithBehaviour, WithHop,
                        WithMeshHealth, WithMessageWindow, WithPeerGater, WithPeerScore, WithSeed, WithValidation,
                        eth2_peer_score_params, eth2_thresholds, graphs)

HOP = 100 * Millisecond
HOPS_PER_ROUND = 10  # HeartbeatInterval 1 s
WORKLOADS = {
    "config4": dict(n=1_000_000, k=32, topics=64, slots=192, msgs=1000),
    "config5": dict(n=1_000_000, k=32, topics=1, slots=10240, msgs=500, adversarial=True),
}
SUMS = ("members", "components", "isolated", "one_sided", "outside", "eclipsed")


def sybils(n, seed):
    return np.random.default_rng(seed + 11).random(n) < 0.2


def build_engine(wl, rounds, seed, extra=(), lib=None):
    """The benchmark's engine of the workload: a random 32-regular graph, every
    host subscribed to every topic, Eth2 scoring, msgs per round spread over its
    hops and topics; config5 adds the adversarial mix."""
    n, T = wl["n"], wl["topics"]
    g = graphs.random_regular_fast(n, wl["k"], seed)
    opts = [WithPeerScore(eth2_peer_score_params(T), eth2_thresholds()), WithHop(HOP), WithMessageWindow(wl["slots"]),
            WithSeed(seed)]
    rng = np.random.default_rng(seed + 7)
    hops = np.repeat(np.arange(1, rounds * HOPS_PER_ROUND + 1, dtype=np.int64), wl["msgs"] // HOPS_PER_ROUND)
    src = rng.integers(0, n, len(hops)).astype(np.int32)
    top = (np.arange(len(hops)) % T).astype(np.int32)
    kind, kw = None, {}
    if wl.get("adversarial"):
        arng = np.random.default_rng(seed + 11)
        sybil = arng.random(n) < 0.2
        ids = np.flatnonzero(sybil)
        kind_of = arng.integers(0, 4, len(ids))  # 0 IWANT spam, 1 GRAFT spam, 2 phantom IHAVE, 3 invalid
        beh = np.zeros(n, np.uint8)
        beh[ids[kind_of == 0]] = GS_BEHAVE_IWANT_SPAM
        beh[ids[kind_of == 1]] = GS_BEHAVE_GRAFT_SPAM
        beh[ids[kind_of == 2]] = GS_BEHAVE_IHAVE_SPAM
        ipv4 = (np.arange(n) + (10 << 24)).astype(np.uint32)
        ipv4[ids] = (192 << 24) + (np.arange(len(ids)) // 20).astype(np.uint32)  # 20 Sybils per IP
        kw["ipv4"] = ipv4
        opts += [WithBehaviour(beh), WithValidation([1] * T, 32), WithPeerGater(DefaultPeerGaterParams())]
        honest = np.flatnonzero(~sybil)
        src = honest[rng.integers(0, len(honest), len(hops))].astype(np.int32)
        kind = np.zeros(len(hops), np.uint8)
        r = rng.random(len(hops))
        inv, ph = ids[kind_of == 3], ids[kind_of == 2]
        sel = r < 1 / 3  # a third invalid messages, a sixth phantom ids
        src[sel] = inv[rng.integers(0, len(inv), int(sel.sum()))]
        kind[sel] = GS_MSG_REJECT
        sel = (r >= 1 / 3) & (r < 0.5)
        src[sel] = ph[rng.integers(0, len(ph), int(sel.sum()))]
        kind[sel] = GS_MSG_PHANTOM
    eng = NewGossipSub(n, T, g, graphs.all_subscribed(n, T), *opts, *extra, lib=lib, **kw)
    eng.publish(src, top, hops, kind=kind)
    return eng


def tick_lines(workload, k, row, groups):
    T = len(row["members"])
    lines = []
    for g in range(groups):
        lo, hi = g * T // groups, (g + 1) * T // groups
        line = {"workload": workload, "tick": k, "hop": row["hop"], "topics": f"{lo}..{hi - 1}"}
        line.update({f: int(row[f][lo:hi].sum()) for f in SUMS})
        line["largest_min"] = int(row["largest"][lo:hi].min())
        line["components_max"] = int(row["components"][lo:hi].max())
        sizes = row["comp_hist"][lo:hi].sum(axis=0)
        line["comp_hist"] = {f"2^{b}": int(c) for b, c in enumerate(sizes) if c}
        lines.append(line)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="config4", choices=sorted(WORKLOADS))
    ap.add_argument("--peers", type=int, default=0, help="override the workload's peer count")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--period-hops", type=int, default=0, help="hops per tick (default: the heartbeat interval)")
    ap.add_argument("--topic-groups", type=int, default=4, help="lines per tick: the topics in this many groups")
    ap.add_argument("--all-hosts", action="store_true", help="config5: count the Sybils too (nodes = None)")
    ap.add_argument("--off", action="store_true", help="no mesh health: the same rounds, for the cost")
    ap.add_argument("--lib", default=None, help="timing experiments only: another build of the product library")
    args = ap.parse_args()
    wl = dict(WORKLOADS[args.workload])
    if args.peers:
        wl["n"] = args.peers
    period = args.period_hops or HOPS_PER_ROUND
    total = 1 + (args.warmup + args.steps) * HOPS_PER_ROUND
    mask = ~sybils(wl["n"], args.seed) if wl.get("adversarial") and not args.all_hosts else None
    extra = () if args.off else (WithMeshHealth(period * HOP, nodes=mask, ticks=total // period + 1),)
    eng = build_engine(wl, args.warmup + args.steps + 1, args.seed, extra=extra, lib=args.lib)
    eng.step(1 + args.warmup * HOPS_PER_ROUND)
    first = 0 if args.off else eng.mesh_health_ticks()
    eng.set_profiling(True)
    eng.sync()
    t0 = time.perf_counter()
    eng.step(args.steps * HOPS_PER_ROUND)
    eng.sync()
    elapsed = time.perf_counter() - t0
    last = {"workload": args.workload, "peers": wl["n"], "steps": args.steps, "warmup": args.warmup,
            "mesh_health": not args.off, "hosts": "all" if mask is None else f"{int(mask.sum())} honest",
            "ms_per_step": round(elapsed / args.steps * 1e3, 3)}
    if not args.off:
        ks = eng.mesh_health_kernel_stats()
        eng.set_profiling(False)
        taken = eng.mesh_health_ticks()
        groups = max(1, min(args.topic_groups, wl["topics"]))
        for k in range(first, taken):
            for line in tick_lines(args.workload, k, eng.mesh_health_row(k), groups):
                print(json.dumps(line))
        n = max(1, taken - first)
        passes = [name for name in ks if name not in ("iterations", "bytes")]
        last.update(period_hops=period, ticks=taken - first,
                    ms_per_tick=round(sum(ks[name][0] for name in passes) / n, 3),
                    **{name + "_ms_per_tick": round(ks[name][0] / n, 3) for name in passes},
                    **{name + "_launches": ks[name][1] for name in passes},
                    iterations_per_tick=round(ks["iterations"] / n, 2),
                    mbytes_per_tick=round(ks["bytes"] / n / 1e6, 1))
    print(json.dumps(last))
    eng.close()


if __name__ == "__main__":
    main()
