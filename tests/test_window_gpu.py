"""The engine's message window at its edges (gs_engine.h setWindow), against
the oracle, which has no window.  The registered `_edge` scenarios (a first
delivery of age exactly maxAge, a slot used again exactly retireHops after its
earlier use) run through the parity, golden, frontier, peertx, partition and
trace tests; here:

- one hop past the limit: a first delivery of age maxAge + 1 is reported as
  GS_ECAPACITY at the hop the oracle makes it, never dropped or counted as a
  duplicate, on every kernel path that carries the age rule;
- one inside and two past: maxAge - 1 runs, maxAge + 2 is refused at the first
  over-age hop;
- the publish guard: a slot is refused retireHops - 1 hops after its earlier
  use and taken at retireHops, and no state of the earlier message reaches
  the new one;
- parameters that move the formula.

tests/test_window.py holds the formula and the scenarios' preconditions."""
import functools
import multiprocessing as mp
import os
import re
import sys

import numpy as np
import pytest

import scenarios
from pubsub_amd import (PRODUCT_LIB, GossipEngineError, WithFrontierBitmaps, WithFrontierLists, WithValidation, _abi)
from test_partition_gpu import _free_port
from test_window import FAMILIES, NEAR, builder, family_window, first_over_hop, ran

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

# the families phase A can read either way (k_flood_a, k_phase_a's dense pass 1)
BOTH_MODES = ["win_flood", "win_flood_3t", "win_gossip", "win_gossip_h7"]
MODES = {"bitmaps": WithFrontierBitmaps, "lists": WithFrontierLists, "default": None}
CASES = [(f, m) for f in FAMILIES for m in (("bitmaps", "lists") if f in BOTH_MODES else ("default",))]


def _extra(mode):
    return () if MODES[mode] is None else (MODES[mode](),)


def _snap(e):
    return scenarios.snapshot(e, getattr(e, "snapshot_ids", range(e.n_published)))


@functools.lru_cache(maxsize=None)
def oracle_snap(oracle, fam, d=0):
    """The oracle's snapshot of the family's run (shared, read only)."""
    return _snap(ran(oracle, fam, d).e)


def _gpu_equals_oracle(oracle, fam, d, mode):
    e, hops = builder(fam, d)(PRODUCT_LIB, _extra(mode))
    e.step(hops)
    if mode != "default":
        assert e.frontier_dense == (mode == "bitmaps")
    bad = scenarios.compare(oracle_snap(oracle, fam, d), _snap(e))
    e.close()
    assert bad == [], "\n".join(bad)


def _refused_late(oracle, fam, d, mode):
    """The run whose tail is d past the _edge one stops with the late-delivery
    error at the oracle's first over-age hop, twice in the same words."""
    e, hops = builder(fam, d)(PRODUCT_LIB, _extra(mode))
    said = []
    for n in (hops, 1):
        with pytest.raises(GossipEngineError) as ei:
            e.step(n)
        assert ei.value.code == _abi.GS_ECAPACITY
        said.append(str(ei.value))
    e.close()
    print(fam, mode, said[0])
    assert "later than" in said[0] and said[0] == said[1]
    assert int(re.search(r"hop (\d+):", said[0]).group(1)) == first_over_hop(oracle, fam, d)


@pytest.mark.parametrize("fam,mode", CASES)
def test_one_past_the_limit_is_reported(oracle_path, fam, mode):
    _refused_late(oracle_path, fam, 1, mode)
    # the refusal leaves nothing behind: the _edge member runs in this process
    _gpu_equals_oracle(oracle_path, fam, 0, mode)


@pytest.mark.parametrize("fam,mode", [(f, m) for f, m in CASES if f in NEAR])
def test_one_inside_and_two_past(oracle_path, fam, mode):
    _gpu_equals_oracle(oracle_path, fam, -1, mode)
    _refused_late(oracle_path, fam, 2, mode)


# ---------------------------------------------------------------- partitioned
def _late_worker(rank, world, port, q):
    try:
        sys.path.insert(0, HERE)
        sys.path.insert(0, os.path.join(os.path.dirname(HERE), "go-libp2p-pubsub_amd"))
        import torch
        import torch.distributed as dist

        import scenarios
        from pubsub_amd import PRODUCT_LIB, GossipEngineError, WithPartition
        from pubsub_amd.transport import TorchTransport
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
        tr = TorchTransport(memory="device")
        e, hops = scenarios.WINDOW_OVER["win_gossip_over"](PRODUCT_LIB, (WithPartition(rank, world, tr),))
        try:
            e.step(hops)
            q.put((rank, None, e.hop))
        except GossipEngineError as ex:
            q.put((rank, (ex.code, str(ex)), e.hop))
        dist.destroy_process_group()
    except Exception as ex:  # report instead of hanging the parent
        import traceback
        q.put((rank, ("raised", f"{ex!r}\n{traceback.format_exc()}"), -1))


def test_partitioned_over_limit_stops_every_rank(oracle_path):
    """win_gossip_over on 2 ranks: the over-age delivery happens on one rank,
    both return GS_ECAPACITY at the same hop, the oracle's."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_late_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = sorted((q.get(timeout=180) for _ in range(world)), key=lambda r: r[0])
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    assert all(r[1] is not None for r in res), res
    assert all(r[1][0] == _abi.GS_ECAPACITY and "later than" in r[1][1] for r in res), res
    assert res[0][2] == res[1][2], res
    want = first_over_hop(oracle_path, "win_gossip")
    assert [int(re.search(r"hop (\d+):", r[1][1]).group(1)) for r in res] == [want, want], res


# ---------------------------------------------------------------- the publish guard
GUARD_SLOTS = 64
GUARD_READABLE = range(2, GUARD_SLOTS + 2)


def _guard_run(lib, fam, probe):
    """The family's _edge network with a 64-slot ring: 64 messages in the
    family's first publish hop (the body author and the tip in turn), then two
    more (the tip's, the body author's) retireHops later: the first hop at
    which gs_publish gives slots 0 and 1 out again.  probe: publish the first
    of the two one hop sooner first, after the engine has run 10 hops past
    the burst, and return what that raised."""
    kw = dict(scenarios.WINDOW_FAMILIES[fam], slots=GUARD_SLOTS)
    _, retire = family_window(fam)
    e = scenarios.window_engine(lib, **kw)
    s = kw["start"]
    src = np.where(np.arange(GUARD_SLOTS) % 2, e.tip, scenarios.WIN_AUTHOR).astype(np.int32)
    ids = e.publish(src, np.zeros(GUARD_SLOTS, np.int32), np.full(GUARD_SLOTS, s, np.int64))
    assert ids.tolist() == list(range(GUARD_SLOTS))
    e.step(s + 10)
    raised = None
    if probe:
        with pytest.raises(GossipEngineError) as ei:
            e.publish([e.tip], [0], [s + retire - 1])
        raised = ei.value
    ids = e.publish([e.tip, scenarios.WIN_AUTHOR], [0, 0], [s + retire, s + retire])
    assert ids.tolist() == [GUARD_SLOTS, GUARD_SLOTS + 1]
    e.step(retire + kw["tail"] + 12 - 10)
    return e, raised


@functools.lru_cache(maxsize=None)
def _guard_oracle(oracle, fam):
    """The oracle given the accepted publishes only, and its snapshot (of the
    messages whose slots were not used again: 2..65)."""
    e, _ = _guard_run(oracle, fam, False)
    return e, scenarios.snapshot(e, GUARD_READABLE)


@pytest.mark.parametrize("probe", [True, False], ids=["refused_then_accepted", "accepted"])
@pytest.mark.parametrize("fam", NEAR)
def test_publish_guard_at_retire_hops(oracle_path, fam, probe):
    max_age, retire = family_window(fam)
    eo, ref = _guard_oracle(oracle_path, fam)
    e, raised = _guard_run(PRODUCT_LIB, fam, probe)
    if probe:
        assert raised.code == _abi.GS_ECAPACITY and "message window too small" in str(raised)
        assert int(re.search(r"within (\d+) hops", str(raised)).group(1)) == retire
    bad = scenarios.compare(ref, scenarios.snapshot(e, GUARD_READABLE))
    assert bad == [], "\n".join(bad)
    # the nodes that took a slot's earlier message at age maxAge (the far end
    # from its author) take the slot's new message as the oracle says
    at_edge = 0
    for slot in (0, 1):
        old_hop, _ = eo.deliveries(slot)
        took = np.flatnonzero(old_hop == scenarios.WINDOW_FAMILIES[fam]["start"] + max_age)
        at_edge += len(took)
        hop, frm = e.deliveries(GUARD_SLOTS + slot)
        want_hop, want_frm = eo.deliveries(GUARD_SLOTS + slot)
        assert (want_hop >= 0).all()
        assert np.array_equal(hop[took], want_hop[took]) and np.array_equal(frm[took], want_frm[took])
    assert at_edge
    e.close()


# ---------------------------------------------------------------- parameters that move the formula
def test_shorter_history_and_heartbeat(oracle_path):
    """HistoryLength 3, HistoryGossip 2, a 700 ms heartbeat and the default
    IWantFollowupTime: maxAge 21 and retireHops 56 hops, slots used again at
    56.  The run equals the oracle, or start() refuses the parameters and
    names the reason; never a third outcome."""
    fam = "win_gossip_h7"
    assert family_window(fam)[1] == scenarios.WINDOW_FAMILIES[fam]["reuse"] < family_window("win_gossip")[1]
    e, hops = builder(fam)(PRODUCT_LIB)
    try:
        e.step(1)
    except GossipEngineError as ex:
        assert ex.code in (_abi.GS_EUNSUPPORTED, _abi.GS_EINVAL) and e.hop == 0
        assert re.search("IWantFollowupTime|HistoryLength|HistoryGossip|HeartbeatInterval", str(ex)), str(ex)
        return
    e.step(hops - 1)
    bad = scenarios.compare(oracle_snap(oracle_path, fam), _snap(e))
    assert bad == [], "\n".join(bad)


def test_validator_alone_switches_the_long_window_on(oracle_path):
    """win_gossip_over's network and traffic with an accepting validator (and
    the ring the longer retireHops then needs): the same ages are now well
    inside the window (the adversarial instantiation's)."""
    long = family_window("win_adv")[1]
    make = scenarios._win("win_gossip", 1, slots=-(-long // 64) * 64, reuse=long)
    e, hops = make(PRODUCT_LIB, (WithValidation([1], 0),))
    e.step(hops)
    eo, _ = make(oracle_path, (WithValidation([1], 0),))
    eo.step(hops)
    bad = scenarios.compare(_snap(eo), _snap(e))
    assert bad == [], "\n".join(bad)
