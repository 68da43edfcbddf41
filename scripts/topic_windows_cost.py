#!/usr/bin/env python3
"""What the table lookup of uneven topic windows costs (include/gs_window.h).

    python scripts/topic_windows_cost.py [--workload config4] [--peers N] [--steps K] [--warmup W]

Builds bench.py's engine twice through WithTopicWindows: with every topic's
ring at the workload's own size (uniform: the engine keeps the multiply), and
with topic 0's ring one word larger (the same traffic through the lookup
tables); then, where the layout has room, the same pair with a word more per
topic, which keeps the words per lane equal within the pair.  Prints one JSON
line per run with ms per step and the deliveries per step, which must agree;
the difference in ms within a pair is the price of the uneven layout.
For information: bench.py remains the yardstick."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "go-libp2p-pubsub_amd"))
import bench  # noqa: E402
from pubsub_amd import WithTopicWindows  # noqa: E402


def run(wl, slots, label, steps, warmup, lib):
    hps = bench.hops_per_step(wl)
    eng, _ = bench.build_engine(wl, warmup + steps + 1, 3, 0, extra=(WithTopicWindows(slots=slots),), lib=lib)
    eng.step(1 + warmup * hps)
    d0 = eng.counters()["deliveries"]
    eng.sync()
    t0 = time.perf_counter()
    eng.step(steps * hps)
    eng.sync()
    elapsed = time.perf_counter() - t0
    line = {"windows": label, "slots_topic0": slots[0], "slots_others": slots[-1], "peers": wl["n"], "steps": steps,
            "warmup": warmup, "ms_per_step": round(elapsed / steps * 1e3, 3),
            "deliveries_per_step": (eng.counters()["deliveries"] - d0) / steps}
    eng.close()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="config4", choices=["config4"])
    ap.add_argument("--peers", type=int, default=0, help="override the workload's peer count")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--lib", default=None, help="timing experiments only: another build of the product library")
    args = ap.parse_args()
    wl = dict(bench.WORKLOADS[args.workload])
    if args.peers:
        wl["n"] = args.peers
    T, st = wl["topics"], wl["slots"]
    lines = [run(wl, [st] * T, "uniform", args.steps, args.warmup, args.lib),
             run(wl, [st + 64] + [st] * (T - 1), "uneven", args.steps, args.warmup, args.lib)]
    if T * (st + 64) <= 16384:
        # the uneven run above may need one more word per lane than the uniform
        # one (config4: 193 words against 192, four per lane against three); this
        # pair has the same words per lane in both runs, so it isolates the lookup
        lines += [run(wl, [st + 64] * T, "uniform, a word more per topic", args.steps, args.warmup, args.lib),
                  run(wl, [st] + [st + 64] * (T - 1), "uneven, a word more per topic but one", args.steps, args.warmup,
                      args.lib)]
    for line in lines:
        print(json.dumps(dict(line, workload=args.workload)))
    assert len({line["deliveries_per_step"] for line in lines}) == 1, "the runs delivered differently"


if __name__ == "__main__":
    main()
