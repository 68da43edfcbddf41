"""The streaming score refresh (k_refresh_rows, gs_kernels.h) at the shapes
where its code takes another path, against the oracle, bit for bit, with a
snapshot after every heartbeat: the decay-to-zero and flag-bit paths play out
over rounds, not only in the final state.

A wave of the refresh owns GS_RG (8) consecutive groups of 1024 / T edges and
streams them through a register ring, so the cases choose edge counts that
leave the last group and the last wave partial and give a wave more groups
than one ring start-up and wind-down cover:

- T = 64, narrow pending counts: the headline instantiation, 16 edges a group;
- T = 16: 64 edges a group, the most for which the score tail's per-edge
  inputs travel in registers (one edge per lane);
- T = 4, wide pending counts, 256 edges a group;
- T = 3 (a lane's topic changes from pair to pair: params from the LDS table)
  and T = 1 (1024 edges a group);
- T = 2 under connection churn: retained and expired score records;
- the life of a mesh failure penalty: the refresh reads mfp only where the
  pair's flag bit says it may be non-zero, so the test first makes sure, on the
  oracle alone, that penalties appear, survive a re-graft and decay to zero.
"""
import functools

import numpy as np
import pytest

import scenarios
from pubsub_amd import (GS_BEHAVE_NO_FORWARD, GS_EV_JOIN, GS_EV_LEAVE, NewGossipSub, PRODUCT_LIB, PeerScoreParams, Second,
                        TopicScoreParams, WithBehaviour, WithGossipSubParams, WithHop, WithMessageWindow,
                        WithPeerScore, WithRecordDeliveries, WithSeed, graphs)
from pubsub_amd.params import GossipSubParams, Millisecond, PeerScoreThresholds

pytestmark = pytest.mark.gpu

BEAT = 10       # hops per heartbeat (HeartbeatInterval 1 s, 100 ms hops)
GROUPS_PER_WAVE = 8  # GS_RG


def _mfp_cycle(lib, n=48, k=8, topics=2, seed=91, beats=16):
    """Where a mesh failure penalty comes from, stays and goes.  The traffic
    keeps an honest mesh peer's delivery counter a little under the threshold
    and every fifth host forwards nothing (a squatter, as in `sinkhole`'s
    family), so once P3 is active (1 s in the mesh) every prune leaves a
    penalty, the deficit squared: the squatters' when their score turns
    negative, and the honest peers' when a host leaves a topic (hops 30-48).
    The host joins again 1.5 s later and grafts peers whose penalty, cut to
    0.3 of itself every second, is still there; the last messages go out at
    hop 95, and by the end the penalties are below DecayToZero."""
    g = graphs.random_regular(n, k, seed)
    tp = TopicScoreParams(TopicWeight=1, TimeInMeshWeight=0.01, TimeInMeshQuantum=Second, TimeInMeshCap=10,
                          FirstMessageDeliveriesWeight=1, FirstMessageDeliveriesDecay=0.9,
                          FirstMessageDeliveriesCap=50, MeshMessageDeliveriesWeight=-0.02,
                          MeshMessageDeliveriesDecay=0.8, MeshMessageDeliveriesCap=30,
                          MeshMessageDeliveriesThreshold=12, MeshMessageDeliveriesWindow=10 * Millisecond,
                          MeshMessageDeliveriesActivation=Second, MeshFailurePenaltyWeight=-0.01,
                          MeshFailurePenaltyDecay=0.3, InvalidMessageDeliveriesDecay=0.5)
    sp = PeerScoreParams(Topics={t: tp for t in range(topics)}, AppSpecificScore=True, AppSpecificWeight=1,
                         DecayInterval=Second, DecayToZero=0.01)
    thr = PeerScoreThresholds(GossipThreshold=-10, PublishThreshold=-100, GraylistThreshold=-10000)
    gp = GossipSubParams(PruneBackoff=Second)
    beh = np.zeros(n, np.uint8)
    beh[::5] = GS_BEHAVE_NO_FORWARD
    e = NewGossipSub(n, topics, g, graphs.all_subscribed(n, topics), WithPeerScore(sp, thr),
                     WithGossipSubParams(gp), WithHop(scenarios.HOP), WithMessageWindow(256), WithBehaviour(beh),
                     WithRecordDeliveries(), WithSeed(seed), app_score=np.ones(n), lib=lib)
    honest = np.flatnonzero(beh == 0)
    rng = np.random.default_rng(seed)
    leavers = rng.choice(honest, 10, replace=False)
    ev = []
    for i, u in enumerate(leavers):
        ev.append((30 + 2 * i, GS_EV_LEAVE, int(u), i % topics))
        ev.append((45 + 2 * i, GS_EV_JOIN, int(u), i % topics))
    ev.sort(key=lambda x: x[0])
    e.schedule_events([x[1] for x in ev], [x[2] for x in ev], [x[3] for x in ev], [x[0] for x in ev])
    msgs = 240
    e.publish(rng.choice(honest, msgs).astype(np.int32), rng.integers(0, topics, msgs).astype(np.int32),
              (5 + np.arange(msgs) * (10 * BEAT - 10) // msgs).astype(np.int64))
    return e, beats * BEAT + 5


def _scored(**kw):
    return lambda lib: scenarios.gossipsub_scored(lib, **kw)


# (the random regular graphs come out a pair short of n * k / 2 connections)
CASES = {
    # 220 edges: 13 full groups of 16 and one of 12; waves of 8 and 6 groups
    "t64_narrow": _scored(n=37, k=6, topics=64, window=64, msgs=300, hb=6, seed=31),
    # 598 edges: 9 full groups of 64 and one of 22; waves of 8 and 2 groups
    "t16_tail_in_registers": _scored(n=100, k=6, topics=16, window=64, msgs=300, hb=6, seed=32),
    # 598 edges: 2 full groups of 256 and one of 86; St = 320 > 254: 32-bit pending counts
    "t4_wide": _scored(n=100, k=6, topics=4, window=320, msgs=300, hb=6, seed=33),
    # 798 edges: 2 full groups of 341 and one of 116
    "t3_topic_per_pair": _scored(n=100, k=8, topics=3, window=128, msgs=300, hb=6, seed=34),
    # 2398 edges: 2 full groups of 1024 and one of 350
    "t1": _scored(n=300, k=8, topics=1, window=512, msgs=300, hb=6, seed=35),
    # 1200 edges: 2 full groups of 512 and one of 176; disconnects, reconnects, leaves and joins
    "t2_churn": lambda lib: scenarios.churn_scored(lib, n=120, k=10, hb=10, msgs=300),
    "mfp_cycle": _mfp_cycle,
}
# edges, edges per group (1024 // T)
SHAPES = {"t64_narrow": (220, 16), "t16_tail_in_registers": (598, 64), "t4_wide": (598, 256),
          "t3_topic_per_pair": (798, 341), "t1": (2398, 1024), "t2_churn": (1200, 512)}


def _snaps(lib, name):
    """The run's snapshot after every heartbeat (deliveries in the last only)."""
    e, hops = CASES[name](lib)
    ids = list(getattr(e, "snapshot_ids", range(e.n_published)))
    out, done = [], 0
    while done < hops:
        step = min(BEAT, hops - done)
        e.step(step)
        done += step
        out.append(scenarios.snapshot(e, ids if done == hops else []))
    out[-1]["edges"] = int(e.edge_range[1] - e.edge_range[0])
    e.close()
    return out


@functools.lru_cache(maxsize=None)
def _oracle_snaps(oracle, name):
    return _snaps(oracle, name)


def _equal(oracle, name):
    ref = _oracle_snaps(oracle, name)
    got = _snaps(PRODUCT_LIB, name)
    assert len(ref) == len(got)
    for beat, (a, b) in enumerate(zip(ref, got)):
        bad = scenarios.compare({k: v for k, v in a.items() if k != "edges"}, b)
        assert bad == [], f"after heartbeat {beat + 1}:\n" + "\n".join(bad)
    return ref


@pytest.mark.parametrize("name", list(SHAPES))
def test_refresh_equals_oracle_every_heartbeat(oracle_path, name):
    ref = _equal(oracle_path, name)
    edges, per_group = SHAPES[name]
    assert ref[-1]["edges"] == edges and edges % per_group != 0
    if name == "t64_narrow":  # a wave's first, middle and last groups, and a second, shorter wave
        assert -(-edges // per_group) >= GROUPS_PER_WAVE + 2
    # the refresh had something to do: counters that decay, P3 switched on nowhere
    # or somewhere, scores that moved
    assert any(np.any(s["ts_fmd"] != 0) for s in ref)
    assert len({np.asarray(s["scores"]).tobytes() for s in ref}) > 1


def test_mfp_life_cycle(oracle_path):
    ref = _oracle_snaps(oracle_path, "mfp_cycle")
    mfp = [np.asarray(s["ts_mfp"]).ravel() for s in ref]
    flags = [np.asarray(s["ts_flags"]).ravel() for s in ref]
    ever = np.zeros(mfp[0].shape, bool)
    for m in mfp:
        ever |= m != 0
    # penalties appear; one is back in the mesh (graft after prune) while it
    # is still there; one has decayed to exactly 0 by the end
    assert ever.any()
    assert any(np.any((m != 0) & ((f & 1) != 0)) for m, f in zip(mfp, flags))
    assert np.any(ever & (mfp[-1] == 0))
    print("pairs with a penalty at some heartbeat:", int(ever.sum()), "back to zero at the end:",
          int((ever & (mfp[-1] == 0)).sum()))
    _equal(oracle_path, "mfp_cycle")
