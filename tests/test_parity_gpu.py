"""GPU parity: the HIP engine (product library) against the CPU oracle on the
same seeded scenarios, through the identical C-ABI calls.  Everything is
compared bit-exactly: counters, per-(node, message) first-delivery hop and
sender, mesh/fanout masks, backoff expiries, every float64 score counter and
score (on their bit patterns, tolerance 0)."""
import numpy as np
import pytest

import scenarios
from pubsub_amd import PRODUCT_LIB

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(scenarios.SCENARIOS))
def test_gpu_matches_oracle(oracle_path, name):
    ref = scenarios.run(oracle_path, name)
    got = scenarios.run(PRODUCT_LIB, name)
    bad = scenarios.compare(ref, got)
    assert bad == [], "\n".join(bad)


def test_gpu_stepwise_equals_one_call(oracle_path):
    """gs_step(1) x K and gs_step(K) produce identical state."""
    e1, hops = scenarios.SCENARIOS["gossipsub_scored"](PRODUCT_LIB)
    for _ in range(hops):
        e1.step(1)
    e2, _ = scenarios.SCENARIOS["gossipsub_scored"](PRODUCT_LIB)
    e2.step(hops)
    ids = range(e1.counters()["published"])
    assert scenarios.compare(scenarios.snapshot(e1, ids), scenarios.snapshot(e2, ids)) == []


def _dense_1200(lib, batches):
    """gossipsub_dense's network with one message per hop from hop 20, 1200 in
    all, published in `batches` (lists of index ranges) with the engine stepped
    up to each batch's first hop in between; the last 100 messages' snapshot
    (older slots are recycled: 256 slots, at most 100 live)."""
    from pubsub_amd import NewGossipSub, WithHop, WithMessageWindow, WithRecordDeliveries, WithSeed, graphs
    n = 20
    e = NewGossipSub(n, 1, graphs.dense_connect(n, 1), graphs.all_subscribed(n, 1), WithRecordDeliveries(),
                     WithSeed(1), WithHop(scenarios.HOP), WithMessageWindow(256), lib=lib)
    src, top, hops = scenarios._publish_schedule(n, 1, 1200, 20, 1, 1)
    done = 0
    for lo, hi in batches:
        if lo:
            e.step(int(hops[lo - 1]) + 1 - done)
            done = int(hops[lo - 1]) + 1
        e.publish(src[lo:hi], top[lo:hi], hops[lo:hi])
    e.step(int(hops[-1]) + 40 - done)
    return scenarios.snapshot(e, range(1100, 1200))


def test_gpu_batched_publish_equals_one_publish(oracle_path):
    """Publishing after the first step appends to the device's message arrays;
    the third batch takes them from 600 to 1200 entries, past their first
    capacity of 1024, so they are reallocated and uploaded again mid-run.  The
    result equals the same schedule published in one call."""
    once = [(0, 1200)]
    ref = _dense_1200(oracle_path, once)
    got = _dense_1200(PRODUCT_LIB, [(0, 300), (300, 600), (600, 1200)])
    bad = scenarios.compare(ref, got)
    assert bad == [], "\n".join(bad)
    bad = scenarios.compare(_dense_1200(PRODUCT_LIB, once), got)
    assert bad == [], "\n".join(bad)


def test_gpu_start_refusal_is_repeatable(oracle_path):
    """A start() that refuses its parameters (GossipRetransmission > 253, a
    host-side check) leaves nothing behind: the next step refuses in the same
    words, and after the engine is destroyed a valid one runs as usual."""
    from pubsub_amd import (GossipEngineError, NewGossipSub, WithGossipSubParams, WithHop, WithMessageWindow,
                            WithSeed, _abi, graphs)
    p = scenarios.GossipSubParams()
    p.GossipRetransmission = 254
    n = 20
    e = NewGossipSub(n, 1, graphs.dense_connect(n, 1), graphs.all_subscribed(n, 1), WithSeed(1),
                     WithHop(scenarios.HOP), WithMessageWindow(256), WithGossipSubParams(p), lib=PRODUCT_LIB)
    said = []
    for _ in range(2):
        with pytest.raises(GossipEngineError) as ei:
            e.step(1)
        assert ei.value.code == _abi.GS_EUNSUPPORTED
        said.append(str(ei.value))
    assert said[0] == said[1] and "GossipRetransmission" in said[0]
    e.close()
    bad = scenarios.compare(scenarios.run(oracle_path, "gossipsub_dense"), scenarios.run(PRODUCT_LIB, "gossipsub_dense"))
    assert bad == [], "\n".join(bad)


def _fanout_all_topics(lib):
    """Hosts 0-3 of gossipsub_dense's network have joined none of the 4 topics
    and publish to all four in the same hop, every 7 hops: k_fanout_pub runs
    four waves on one host's row at once (one per (host, topic) pair)."""
    from pubsub_amd import NewGossipSub, WithHop, WithMessageWindow, WithRecordDeliveries, WithSeed, graphs
    n, T = 20, 4
    subs = graphs.all_subscribed(n, T)
    subs[:4] = 0
    e = NewGossipSub(n, T, graphs.dense_connect(n, 1), subs, WithRecordDeliveries(), WithSeed(1),
                     WithHop(scenarios.HOP), WithMessageWindow(64), lib=lib)
    hops = np.repeat(np.arange(12, 47, 7), 16).astype(np.int64)
    src = np.tile(np.repeat(np.arange(4), T), 5).astype(np.int32)
    top = np.tile(np.arange(T), 20).astype(np.int32)
    e.publish(src, top, hops)
    e.step(60)
    return scenarios.snapshot(e, range(e.n_published))


def test_gpu_fanout_to_several_topics_in_one_hop(oracle_path):
    """Publish to several unjoined topics in one hop (gossipsub.go:977-994 per
    message): every topic's fanout peers are kept, none lost to the others'
    waves (ladder_mixed_4t found the lost update)."""
    ref = _fanout_all_topics(oracle_path)
    fo = ref["fanout"]
    assert all(((fo >> np.uint64(t)) & np.uint64(1)).sum() > 0 for t in range(4))
    for _ in range(3):
        bad = scenarios.compare(ref, _fanout_all_topics(PRODUCT_LIB))
        assert bad == [], "\n".join(bad)


def test_gpu_degree_limit_refusal_is_repeatable(oracle_path):
    """One wave per node: a node with 65 peers is refused on the host (the
    oracle runs that graph, tests/test_ladder.py), in the same words each
    time; after the engine is destroyed, a graph whose largest degree is
    exactly 64 runs and equals the oracle."""
    from pubsub_amd import GossipEngineError, _abi
    e, _ = scenarios.degree65_star(PRODUCT_LIB)
    said = []
    for _ in range(2):
        with pytest.raises(GossipEngineError) as ei:
            e.step(1)
        assert ei.value.code == _abi.GS_EUNSUPPORTED
        said.append(str(ei.value))
    assert said[0] == said[1] and "degree" in said[0]
    e.close()
    bad = scenarios.compare(scenarios.run(oracle_path, "ladder_scored"), scenarios.run(PRODUCT_LIB, "ladder_scored"))
    assert bad == [], "\n".join(bad)


def _retuned(lib):
    """Topic.SetScoreParams mid-run (score.go:192-232): topic 1 gets lower
    first/mesh delivery caps (the recap clamps existing counters) and new
    weights; topic 2, unscored so far, becomes scored."""
    from pubsub_amd import eth2_topic_score_params
    e, hops = scenarios.SCENARIOS["gossipsub_multitopic"](lib)
    e.step(hops // 2)
    p = eth2_topic_score_params()
    p.FirstMessageDeliveriesCap = 3.0
    p.MeshMessageDeliveriesCap = 4.0
    p.MeshMessageDeliveriesThreshold = 2.0
    p.TopicWeight = 0.5
    e.set_topic_score_params(1, p)
    e.step(3)
    q = eth2_topic_score_params()
    q.TimeInMeshWeight = 0.01
    e.set_topic_score_params(2, q)
    e.step(hops - hops // 2)
    return scenarios.snapshot(e, range(e.n_published))


def test_gpu_set_topic_score_params_matches_oracle(oracle_path):
    bad = scenarios.compare(_retuned(oracle_path), _retuned(PRODUCT_LIB))
    assert bad == [], "\n".join(bad)


def _scored_with_pool_cap(lib, cap, monkeypatch):
    monkeypatch.setenv("GS_DEBUG_POOL_SUB_CAP", str(cap))
    try:
        e, hops = scenarios.SCENARIOS["gossipsub_scored"](lib)
        e.step(hops)
        return scenarios.snapshot(e, range(e.n_published))
    finally:
        monkeypatch.delenv("GS_DEBUG_POOL_SUB_CAP")


def test_gpu_pool_sub_arena_spill(oracle_path, monkeypatch):
    """pool_take (gs_device.h): when a node's sub-arena of the IWANT arena is
    full the allocation spills into the next sub-arena before E_POOL (ADVICE
    r4).  GS_DEBUG_POOL_SUB_CAP caps the 16 sub-arenas of an unpartitioned
    engine and makes every node try sub-arena 0 first: at 256 ids each (4096
    per hop; gossipsub_scored peaks at about 700 request and served ids per
    hop) every busy hop fills sub-arena 0 and spills, and the run still equals
    the oracle; at 4 ids each the hop's ids do not fit at all and the engine
    reports the arena overflow."""
    from pubsub_amd import GossipEngineError, _abi
    ref = scenarios.run(oracle_path, "gossipsub_scored")
    got = _scored_with_pool_cap(PRODUCT_LIB, 256, monkeypatch)
    bad = scenarios.compare(ref, got)
    assert bad == [], "\n".join(bad)
    with pytest.raises(GossipEngineError) as ei:
        _scored_with_pool_cap(PRODUCT_LIB, 4, monkeypatch)
    assert ei.value.code == _abi.GS_ECAPACITY and "arena" in str(ei.value)
