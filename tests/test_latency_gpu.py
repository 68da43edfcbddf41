"""Latency statistics counted on the device (include/gs_latency.h) against the
oracle's per-message deliveries (tests/latency_ref.py).  Every comparison is
exact.  The scenarios are the smallest that reach each path: the bitmap
counter (floodsub on dense frontiers), the list counter, a GS_BEHAVE_NO_FORWARD
host (no list of its own), validation and gater drops under the long
adversarial window, T = 64 (four words per lane), the last bin and a slot used
again exactly retireHops after its first use (the window families' _edge
members; the _over members, which must fail, are not run here).
tests/test_latency.py holds the scenarios' preconditions."""
import ctypes as C
import functools
import multiprocessing as mp
import os
import sys

import numpy as np
import pytest

import latency_ref
import scenarios
from pubsub_amd import (PRODUCT_LIB, GossipEngineError, WithFrontierBitmaps, WithFrontierLists, WithLatencyStats,
                        _abi)
from test_partition_gpu import _free_port

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
MODES = {"default": (), "lists": (WithFrontierLists(),), "bitmaps": (WithFrontierBitmaps(),)}
# the other frontier form of the scenarios phase A can read either way
VARIANTS = [("floodsub_multitopic", "lists"), ("win_flood_3t", "lists"), ("gossipsub_dense", "bitmaps"),
            ("win_gossip", "bitmaps")]
CASES = [(name, "default") for name in sorted(latency_ref.TABLE)] + VARIANTS


class Got:
    """One run on the GPU with the statistics on, everything read back."""

    def __init__(self, oracle, name, mode):
        r = latency_ref.ref(oracle, name)
        e, hops = latency_ref.builder(name)(PRODUCT_LIB, (WithLatencyStats(),) + MODES[mode])
        assert hops == r.hops
        e.step(hops)
        self.dense = e.frontier_dense
        self.bins = e.latency_bins()
        self.hist = e.latency_hist()
        self.deliveries = e.counters()["deliveries"]
        self.live = list(r.live_ids)
        self.rows = e.message_latency(self.live)
        self.refused = None
        if 0 not in self.live:  # a window family: id 0's slot has a new owner
            with pytest.raises(GossipEngineError) as ei:
                e.message_latency([0])
            self.refused = (ei.value.code, str(ei.value))
        e.close()


@functools.lru_cache(maxsize=None)
def got(oracle, name, mode):
    return Got(oracle, name, mode)


@pytest.mark.parametrize("name,mode", CASES)
def test_topic_histogram_equals_oracle(oracle_path, name, mode):
    r, g = latency_ref.ref(oracle_path, name), got(oracle_path, name, mode)
    if mode != "default":
        assert g.dense == (mode == "bitmaps")
    elif "flood" in name:
        assert g.dense  # the bitmap counter is the default on floodsub
    assert g.bins > r.max_age and g.hist.shape == (r.T, g.bins) and g.hist.dtype == np.int64
    want = r.hist(g.bins)
    assert np.array_equal(g.hist, want), f"first differences at {np.argwhere(g.hist != want)[:5].tolist()}"
    assert g.hist.sum() == g.deliveries == r.counters["deliveries"]


@pytest.mark.parametrize("name,mode", CASES)
def test_message_rows_equal_oracle(oracle_path, name, mode):
    r, g = latency_ref.ref(oracle_path, name), got(oracle_path, name, mode)
    want = r.message_rows(g.live, g.bins)
    assert g.rows.dtype == np.uint32 and g.rows.shape == want.shape
    bad = np.flatnonzero((g.rows != want).any(axis=1))
    assert len(bad) == 0, f"{len(bad)} messages differ, first ids {[g.live[i] for i in bad[:5]]}"
    if name in latency_ref.WINDOWS:
        # the reused slot's first owner is refused in gs_read_deliveries' words;
        # the new owner's row (among the live ids) holds its own counts only
        assert g.refused == (_abi.GS_ESTATE, f"gossip engine error {_abi.GS_ESTATE}: "
                             "message slot already recycled (window moved on)")
    else:
        assert g.refused is None


def test_scheduled_but_unpublished_reads_zeros(oracle_path):
    """win_flood after 20 hops: slot 0 holds id 0's counts, and its next owner
    (the 65th message of the 64-slot ring) is scheduled but not published."""
    r = latency_ref.ref(oracle_path, "win_flood")
    e, _ = latency_ref.builder("win_flood")(PRODUCT_LIB, (WithLatencyStats(),))
    slots = scenarios.WINDOW_FAMILIES["win_flood"]["slots"]
    nxt, last = r.live_ids[0], r.live_ids[-1]  # the schedule's last `slots` messages own the ring
    assert nxt == len(e.msg_hop) - slots and e.msg_hop[nxt - slots] < 15 and e.msg_hop[nxt] > 20
    e.step(20)  # nxt's slot holds the counts of its earlier owner, nxt - slots
    bins = e.latency_bins()
    assert e.latency_hist().sum() > 0
    assert not e.message_latency([nxt, last]).any()
    with pytest.raises(GossipEngineError) as ei:  # the earlier owner lost the slot when nxt was scheduled
        e.message_latency([nxt - slots])
    assert ei.value.code == _abi.GS_ESTATE
    # once published, nxt's row starts from zero: its own counts only
    upto = int(e.msg_hop[nxt]) + 8
    e.step(upto - 20)
    ages = r.age[nxt][(r.age[nxt] >= 0) & (r.hop[nxt] < upto)]
    assert len(ages) > 0
    assert np.array_equal(e.message_latency([nxt, last]), [np.bincount(ages, minlength=bins), np.zeros(bins)])
    e.close()


def test_reset_keeps_later_deliveries_only(oracle_path):
    name = "gossipsub_multitopic"
    r = latency_ref.ref(oracle_path, name)
    e, hops = latency_ref.builder(name)(PRODUCT_LIB, (WithLatencyStats(),))
    half = hops // 2
    e.step(half)
    bins = e.latency_bins()
    before = e.latency_hist()
    assert np.array_equal(before, r.hist(bins) - r.hist(bins, from_hop=half)) and before.sum() > 0
    e.reset_latency_stats()
    assert not e.latency_hist().any()
    e.step(hops - half)
    want = r.hist(bins, from_hop=half)
    assert want.sum() > 0 and np.array_equal(e.latency_hist(), want)
    # the per-message table is not reset
    assert np.array_equal(e.message_latency(r.live_ids), r.message_rows(r.live_ids, bins))
    e.close()


@pytest.mark.parametrize("name", ["gossipsub_scored", "adversarial_mix", "win_gossip_4t"])
def test_nothing_else_moves(name):
    make = scenarios._win(name) if name in scenarios.WINDOW_FAMILIES else scenarios.SCENARIOS[name]
    snaps = []
    for extra in ((), (WithLatencyStats(),)):
        e, hops = make(PRODUCT_LIB, extra)
        e.step(hops)
        snaps.append(scenarios.snapshot(e, getattr(e, "snapshot_ids", range(e.n_published))))
        e.close()
    bad = scenarios.compare(*snaps)
    assert bad == [], "\n".join(bad)


def test_refusals():
    e, _ = scenarios.SCENARIOS["gossipsub_dense"](PRODUCT_LIB, (WithLatencyStats(),))
    lib, h = e.lib, e.h
    assert lib.gs_latency_bins(h) == _abi.GS_ESTATE  # not started
    e.step(25)
    assert lib.gs_set_latency_stats(h, 0) == _abi.GS_ESTATE
    assert lib.gs_set_latency_stats(h, 1) == _abi.GS_ESTATE
    bins = e.latency_bins()
    assert bins == 3 * 10 + 1  # three heartbeats of 10 hops
    hist = np.zeros((e.T, bins + 1), np.int64)
    rows = np.zeros((1, bins + 1), np.uint32)
    ids = np.zeros(1, np.int64)
    hp, rp, ip = (hist.ctypes.data_as(C.POINTER(C.c_int64)), rows.ctypes.data_as(C.POINTER(C.c_uint32)),
                  ids.ctypes.data_as(C.POINTER(C.c_int64)))
    for wrong in (bins - 1, bins + 1, 0):
        assert lib.gs_read_latency_hist(h, hp, wrong) == _abi.GS_EINVAL
        assert lib.gs_read_message_latency(h, 1, ip, rp, wrong) == _abi.GS_EINVAL
    assert not hist.any() and not rows.any()
    for unknown in (-1, e.n_published):
        ids[0] = unknown
        assert lib.gs_read_message_latency(h, 1, ip, rp, bins) == _abi.GS_EINVAL
    assert e.message_latency([]).shape == (0, bins)
    e.close()
    # statistics off: every read is refused, before and after the start
    e, _ = scenarios.SCENARIOS["gossipsub_dense"](PRODUCT_LIB)
    for _ in range(2):
        for call in (e.latency_bins, e.latency_hist, e.reset_latency_stats, lambda: e.message_latency([0])):
            with pytest.raises(GossipEngineError) as ei:
                call()
            assert ei.value.code == _abi.GS_ESTATE
        e.step(1)
    e.close()


# ---------------------------------------------------------------- partitioned
def _worker(rank, world, port, name, oracle, q):
    try:
        sys.path.insert(0, HERE)
        sys.path.insert(0, os.path.join(os.path.dirname(HERE), "go-libp2p-pubsub_amd"))
        import torch
        import torch.distributed as dist

        import latency_ref
        from pubsub_amd import PRODUCT_LIB, WithLatencyStats, WithPartition
        from pubsub_amd.transport import TorchTransport
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
        tr = TorchTransport(memory="device")
        e, hops = latency_ref.builder(name)(PRODUCT_LIB, (WithPartition(rank, world, tr), WithLatencyStats()))
        e.step(hops)
        bins, hist, own = e.latency_bins(), e.latency_hist(), e.node_range
        live = list(getattr(e, "snapshot_ids", range(e.n_published)))
        rows = e.message_latency(live)
        deliveries = e.counters()["deliveries"]
        r = latency_ref.ref(oracle, name)
        bad = []
        want = r.hist(bins, own)
        if not np.array_equal(hist, want):
            bad.append(f"rank {rank} {own}: {int((hist != want).sum())} histogram entries differ")
        if hist.sum() != deliveries:
            bad.append(f"rank {rank}: histogram total {hist.sum()} != its deliveries counter {deliveries}")
        if not np.array_equal(rows, r.message_rows(live, bins, own)):
            bad.append(f"rank {rank} {own}: per-message rows differ")
        total = torch.from_numpy(hist.copy())
        dist.all_reduce(total)
        if not np.array_equal(total.numpy(), r.hist(bins)):
            bad.append("the ranks' tables do not add up to the whole graph's")
        q.put((rank, bad, own))
        dist.destroy_process_group()
    except Exception as ex:  # report instead of hanging the parent
        import traceback
        q.put((rank, [f"worker raised: {ex!r}\n{traceback.format_exc()}"], None))


@pytest.mark.parametrize("world,name", [(2, "gossipsub_multitopic"), (2, "adversarial_mix"), (3, "ladder_64t")])
def test_partitioned_rank_counts_its_own_nodes(oracle_path, world, name):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, name, oracle_path, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in range(world):
            res.append(q.get(timeout=240))
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    res.sort(key=lambda x: x[0])
    assert [x[0] for x in res] == list(range(world))
    for rank, bad, own in res:
        assert bad == [], "\n".join(bad)
    assert res[0][2][0] == 0 and res[-1][2][1] == latency_ref.TABLE[name][0]
