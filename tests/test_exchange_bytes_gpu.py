"""Wire volume of the per-hop exchange (csrc/gs_exchange_wire.h) pinned per
rank: the bytes a rank received (`exchange_stats()`) and the transport calls
it made over a whole scenario equal the values recorded in
tests/golden/exchange_bytes.json (tests/golden/make_golden_exchange.py).  Both
are sums of deterministic per-hop counts, so the comparison is exact.  The
scenarios cover the sections of the wire between them:
  push_overflow  lists shipped after the deferred decision, -1 push records
  c4shape        push blocks, lists staying home
  randomsub_100  randomsub masks behind the list entries
  spam_iwant     lists always shipped, IWANT-spam records
  px_star        peer-exchange dials and PX arena lists"""
import json
import multiprocessing as mp
import os
import socket
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "exchange_bytes.json")

CASES = [(2, "push_overflow"), (2, "c4shape"), (3, "randomsub_100"), (2, "spam_iwant"), (3, "px_star")]


def _worker(rank, world, port, name, q):
    try:
        sys.path.insert(0, HERE)
        sys.path.insert(0, os.path.join(os.path.dirname(HERE), "go-libp2p-pubsub_amd"))
        import torch
        import torch.distributed as dist

        import scenarios
        from pubsub_amd import PRODUCT_LIB, WithPartition
        from pubsub_amd.transport import TorchTransport
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
        tr = TorchTransport(memory="device")
        e, hops = scenarios.SCENARIOS[name](PRODUCT_LIB, (WithPartition(rank, world, tr),))
        e.step(hops)
        q.put((rank, {"bytes_in": int(e.exchange_stats()[1]), "calls": int(tr.calls)}))
        dist.destroy_process_group()
    except Exception as ex:  # report instead of hanging the parent
        import traceback
        q.put((rank, f"worker raised: {ex!r}\n{traceback.format_exc()}"))


def measure(world, name):
    """Per rank: {"bytes_in", "calls"} after the whole scenario."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = [ctx.Process(target=_worker, args=(r, world, port, name, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = sorted((q.get(timeout=240) for _ in range(world)), key=lambda r: r[0])
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    assert all(isinstance(r[1], dict) for r in res), res
    return [r[1] for r in res]


@pytest.mark.gpu
@pytest.mark.parametrize("world,name", CASES)
def test_exchange_volume_equals_recorded(world, name):
    want = json.load(open(GOLDEN))[name]
    assert want["world"] == world
    got = measure(world, name)
    print(name, got)
    assert got == want["ranks"]
    assert all(r["bytes_in"] > 0 and r["calls"] > 0 for r in got)
