"""Mesh reach on the device (include/gs_mesh_reach.h) against the reference
(tests/mesh_reach_ref.py) over the oracle stepped in pieces.  Every comparison
is exact.  Each (case, number of sources) runs once on the GPU, as one single
step(hops) with a tick per heartbeat and the depths kept, and every test reads
that run.  tests/test_mesh_reach.py holds the cases' preconditions."""
import ctypes as C
import functools

import numpy as np
import pytest

import inspect_ref
import mesh_health_ref as mhref
import mesh_reach_ref as rref
import scenarios
from pubsub_amd import (PRODUCT_LIB, GossipEngineError, WithMeshHealth, WithMeshReach, WithPartition,
                        WithPeerScoreInspect, _abi)

pytestmark = pytest.mark.gpu
HOP = scenarios.HOP
KS = (1, 64, rref.NUM_SOURCES)  # one source; a full pass; a second pass with one source


def option(sources, mask=None, ticks=64, depths=True, period=rref.PERIOD):
    return WithMeshReach(period * HOP, sources, nodes=mask, ticks=ticks, depths=depths)


def differences(got, want, k, K=None):
    """`want` may hold more sources than `got`: its first K are compared."""
    K = len(got["reached"]) if K is None else K
    return [f"tick {k}: {f} differs at (source, topic, ...) {np.argwhere(got[f] != want[f][:K])[:4].tolist()}"
            for f in rref.ROW if not np.array_equal(got[f], want[f][:K])]


# ---------------------------------------------------------------- 1. the ring's closed form
def _check_ring(e, topics, n):
    """Source 0's rows and depths at every tick taken so far against ring_want."""
    for k in range(e.mesh_reach_ticks()):
        row = e.mesh_reach_row(k)
        assert row["hop"] == (k + 1) * rref.PERIOD
        reached, unreached, ecc, hist, depths = rref.ring_want(k, n)
        for t in range(topics):
            assert (row["reached"][0, t], row["unreached"][0, t], row["ecc"][0, t]) == (reached, unreached, ecc), (k, t)
            assert np.array_equal(row["depth_hist"][0, t], hist), (k, t)
    return depths


def test_ring_closed_form():
    n = mhref.RING_N
    e = mhref.ring_engine(PRODUCT_LIB, (option([0, n // 2], ticks=8),))
    assert e.mesh_reach_ticks() == 0
    e.step(20)
    # before the cut: 100 levels, 25 batches; the bin of the depths >= 63
    row = e.mesh_reach_row(1)
    for f in rref.ROW:
        assert row[f].dtype == np.int64 and row[f].shape == ((2, 2, 64) if f == "depth_hist" else (2, 2))
    assert row["ecc"].tolist() == [[100, 100], [100, 100]] and row["depth_hist"][0, 0].tolist() == [0] + [2] * 62 + [75]
    tick, dep = e.mesh_reach_depths()
    assert tick == 1 and dep.dtype == np.uint8 and dep.shape == (2, n, 2)
    assert np.array_equal(dep[0, :, 0], _check_ring(e, 2, n)) and np.array_equal(dep[0, :, 1], dep[0, :, 0])
    assert np.array_equal(dep[1, :, 0], np.roll(dep[0, :, 0], n // 2))  # the same ring seen from its other side
    ks = e.mesh_reach_kernel_stats()
    assert ks["passes"] == 2 and ks["levels"] == 2 * 101  # 100 levels that set bits and the one that finds none
    e.step(mhref.RING_HOPS - 20)
    assert e.mesh_reach_ticks() == 5
    tick, dep = e.mesh_reach_depths()
    assert tick == 4 and np.array_equal(dep[0, :, 1], _check_ring(e, 2, n))
    row = e.mesh_reach_row(4)  # source 100 is the far end of the other arc: 99 .. 1 at depths 1 .. 99
    assert (row["reached"][1, 0], row["unreached"][1, 0], row["ecc"][1, 0]) == (99, 100, 99)
    assert dep[1, 1:n // 2, 0].tolist() == list(range(99, 0, -1)) and (dep[1, n // 2 + 1:, 0] == 255).all()
    ks = e.mesh_reach_kernel_stats()
    print(f"ring: {ks['levels']} levels in {ks['passes']} passes, {ks['bytes']} bytes")
    assert ks["passes"] == 5 and ks["levels"] == 2 * 101 + 3 * 100 and ks["bytes"] > 0
    e.close()


@pytest.mark.parametrize("topics,n", [(1, 200), (40, 130)])
def test_ring_other_lane_layouts(topics, n):
    """64 hosts per wave (T = 1) and a wave per host with idle lanes (T = 40),
    with a host count that fills no last wave; the closed form, and the
    reference over the engine's own readbacks."""
    e = mhref.ring_engine(PRODUCT_LIB, (option([0]),), topics=topics, n=n)
    e.step(20)
    before = e.mesh_reach_depths()[1]
    assert np.array_equal(before[0, :, topics - 1], _check_ring(e, topics, n))
    e.step(mhref.RING_HOPS - 20)
    row, (tick, dep) = e.mesh_reach_row(4), e.mesh_reach_depths()
    want = rref.of_engine(e, [0])
    assert differences(row, want, 4) == [] and tick == 4 and np.array_equal(dep, want["depths"])
    assert np.array_equal(dep[0, :, 0], _check_ring(e, topics, n))
    e.close()


def test_depth_table_clips_at_254():
    """A ring of 600 hosts: depths up to 300, stored as min(depth, 254); ECC and
    REACHED stay exact."""
    n = 600
    e = mhref.ring_engine(PRODUCT_LIB, (option([0], period=20),), topics=1, n=n)
    e.step(20)
    row, (_, dep) = e.mesh_reach_row(0), e.mesh_reach_depths()
    reached, unreached, ecc, hist, _ = rref.ring_want(0, n)
    assert (row["reached"][0, 0], row["unreached"][0, 0], row["ecc"][0, 0]) == (reached, unreached, ecc) == (599, 0, 300)
    assert np.array_equal(row["depth_hist"][0, 0], hist)
    true = np.minimum(np.arange(n), n - np.arange(n))
    assert np.array_equal(dep[0, :, 0], np.minimum(true, 254)) and (dep == 254).sum() == 2 * 46 + 1
    e.close()


# ---------------------------------------------------------------- 2. scenario parity
class Got:
    """One run on the GPU with mesh reach on over the reference's first K
    sources, every tick read back."""

    def __init__(self, oracle, name, key, K):
        r = rref.ref(oracle, name, key)
        e, hops = scenarios.SCENARIOS[name](PRODUCT_LIB, (option(r.sources[:K], r.mask),))
        assert hops == r.hops
        e.step(hops)
        self.ticks = e.mesh_reach_ticks()
        self.rows = [e.mesh_reach_row(k) for k in range(self.ticks)]
        self.depth_tick, self.depths = e.mesh_reach_depths()
        self.stats = e.mesh_reach_kernel_stats()
        self.final = scenarios.snapshot(e, getattr(e, "snapshot_ids", range(e.n_published)))
        e.close()


@functools.lru_cache(maxsize=None)
def got(oracle, name, key, K):
    return Got(oracle, name, key, K)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name,key", rref.CASES)
def test_rows_and_depths_equal_reference(oracle_path, name, key, K):
    r, g = rref.ref(oracle_path, name, key), got(oracle_path, name, key, K)
    assert g.ticks == r.ticks > 0
    bad = []
    for k in range(r.ticks):
        assert g.rows[k]["hop"] == r.hop(k) and g.rows[k]["reached"].shape == (K, r.T)
        bad += differences(g.rows[k], r.rows[k], k, K)
    assert bad == [], "\n".join(bad[:10])
    assert g.depth_tick == r.ticks - 1
    assert np.array_equal(g.depths, r.depths[:K]), np.argwhere(g.depths != r.depths[:K])[:5].tolist()
    passes = (K + 63) // 64
    print(f"{name} K={K}: {g.stats['levels']} levels in {g.stats['passes']} passes over {g.ticks} ticks")
    assert g.stats["passes"] == g.ticks * passes
    # a pass runs its deepest source's levels and the one that finds nothing
    want_levels = sum(int(r.rows[k]["ecc"][p * 64:min(K, p * 64 + 64)].max()) + 1
                      for k in range(r.ticks) for p in range(passes))
    assert g.stats["levels"] == want_levels


@pytest.mark.parametrize("name,key", rref.CASES)
def test_nothing_else_moves(oracle_path, name, key):
    """The run with mesh reach on ends in the oracle's final state."""
    bad = scenarios.compare(rref.ref(oracle_path, name, key).final, got(oracle_path, name, key, rref.NUM_SOURCES).final)
    assert bad == [], "\n".join(bad)


# ---------------------------------------------------------------- 3. predicted equals actual
def test_predicted_depth_is_the_engines_own_delivery_age():
    """gossipsub_multitopic on the engine, every host a source (four passes, the
    last with 8), a tick at every hop: for every message, the depth table of
    the tick after its publish hop, at its author and topic, is the age of its
    first delivery at every host (255: never delivered)."""
    e, hops = scenarios.SCENARIOS["gossipsub_multitopic"](PRODUCT_LIB, (option(np.arange(200), ticks=2, period=1),))
    assert e.N == 200 and e.n_published == 240
    pub = {}
    for m, h in enumerate(e.msg_hop.tolist()):
        pub.setdefault(h, []).append(m)
    predicted = {}
    for _ in range(hops):
        e.step(1)
        due = pub.get(e.hop - 1, ())
        if due:
            tick, dep = e.mesh_reach_depths()
            assert tick == e.hop - 1
            for m in due:
                predicted[m] = dep[int(e.msg_src[m]), :, int(e.msg_topic[m])].astype(np.int64)
    assert len(predicted) == 240 and e.mesh_reach_kernel_stats()["passes"] == 4 * hops
    differ = 0
    for m in range(240):
        at, _ = e.deliveries(m)
        age = np.where(at >= 0, at.astype(np.int64) - int(e.msg_hop[m]), 255)
        assert age[int(e.msg_src[m])] == 0
        differ += int((age != predicted[m]).sum())
    assert differ == 0
    e.close()


# ---------------------------------------------------------------- 4. ring of ticks and errors
def _raw(period=1, ticks=1, sources=(0,), mask=None, depths=0, num=None):
    src = np.array(sources, dtype=np.int32)
    cfg = _abi.MeshReachConfigC(period, ticks, len(src) if num is None else num,
                                src.ctypes.data_as(C.POINTER(C.c_int32)) if len(src) else None,
                                mask.ctypes.data_as(C.POINTER(C.c_uint8)) if mask is not None else None, depths)
    cfg._keep = (src, mask)
    return cfg


def _err(e):
    return e.lib.gs_last_error().decode()


def test_tick_ring():
    e = mhref.ring_engine(PRODUCT_LIB, (option([0], ticks=2, depths=False),))
    e.step(mhref.RING_HOPS)
    assert e.mesh_reach_ticks() == 5
    for k in (3, 4):
        row = e.mesh_reach_row(k)
        assert row["hop"] == (k + 1) * rref.PERIOD
        assert (row["reached"][0, 0], row["unreached"][0, 0], row["ecc"][0, 0]) == rref.ring_want(k)[:3]
    for k, code in [(0, _abi.GS_ESTATE), (1, _abi.GS_ESTATE), (2, _abi.GS_ESTATE), (5, _abi.GS_EINVAL),
                    (-1, _abi.GS_EINVAL)]:
        with pytest.raises(GossipEngineError) as ei:
            e.mesh_reach_row(k)
        assert ei.value.code == code, (k, str(ei.value))
    with pytest.raises(GossipEngineError) as ei:  # depths = 0: no depth table
        e.mesh_reach_depths()
    assert ei.value.code == _abi.GS_ESTATE
    e.close()


def test_refusals():
    opt = WithMeshReach(HOP, [0, 3])
    for name in ("floodsub_dense", "randomsub_100"):
        with pytest.raises(GossipEngineError) as ei:
            scenarios.SCENARIOS[name](PRODUCT_LIB, (opt,))
        assert ei.value.code == _abi.GS_EUNSUPPORTED and "pubsub router is not gossipsub" in str(ei.value)
    # scoring is not needed
    e, _ = scenarios.SCENARIOS["gossipsub_dense"](PRODUCT_LIB, (WithMeshReach(HOP, [0, 3], depths=True),))
    # a second call
    assert e.lib.gs_set_mesh_reach(e.h, C.byref(_raw())) == _abi.GS_ESTATE
    assert _err(e) == "duplicate mesh reach inspector"
    # before the first tick
    assert e.mesh_reach_ticks() == 0
    for call in (lambda: e.mesh_reach_row(0), e.mesh_reach_depths):
        with pytest.raises(GossipEngineError) as ei:
            call()
        assert ei.value.code == _abi.GS_EINVAL
    e.step(2)
    assert e.mesh_reach_ticks() == 2 and e.mesh_reach_row(1)["hop"] == 2 and e.mesh_reach_depths()[0] == 1
    e.close()
    # bad arguments, each with a text of its own; nothing is set by a refused call
    e, _ = scenarios.SCENARIOS["gossipsub_multitopic"](PRODUCT_LIB)
    texts = set()
    for cfg in (_raw(period=0), _raw(period=-3), _raw(ticks=0), _raw(sources=()), _raw(num=0),
                _raw(num=_abi.GS_REACH_MAX_SOURCES + 1), _raw(sources=(0, e.N)), _raw(sources=(-1,)),
                _raw(sources=(4, 9, 4)), _raw(sources=(), num=3)):
        assert e.lib.gs_set_mesh_reach(e.h, C.byref(cfg)) == _abi.GS_EINVAL
        texts.add(_err(e))
    assert len(texts) == 6 and "mesh reach: source 4 is given twice" in texts
    assert e.lib.gs_set_mesh_reach(e.h, None) == _abi.GS_EINVAL
    # mesh reach off: every read is refused, before and after the start
    for _ in range(2):
        for call in (e.mesh_reach_ticks, e.mesh_reach_depths, e.mesh_reach_kernel_stats, lambda: e.mesh_reach_row(0)):
            with pytest.raises(GossipEngineError) as ei:
                call()
            assert ei.value.code == _abi.GS_ESTATE
        e.step(1)
    # after the first step
    assert e.lib.gs_set_mesh_reach(e.h, C.byref(_raw())) == _abi.GS_ESTATE
    assert "before the first step" in _err(e)
    e.close()
    # the cap itself is accepted
    e, _ = scenarios.SCENARIOS["gossipsub_scored"](PRODUCT_LIB, (WithMeshReach(HOP, np.arange(256)),))
    e.close()


def test_nothing_is_launched_before_a_tick_is_due():
    e, _ = scenarios.SCENARIOS["gossipsub_dense"](PRODUCT_LIB, (WithMeshReach(100 * HOP, [0]),))
    e.set_profiling(True)
    e.step(99)
    ks = e.mesh_reach_kernel_stats()
    assert e.mesh_reach_ticks() == 0 and all(ks[name] == (0.0, 0) for name in _abi.REACH_KERNEL_NAMES)
    assert (ks["passes"], ks["levels"], ks["bytes"]) == (0, 0, 0)
    e.step(1)
    ks = e.mesh_reach_kernel_stats()
    assert e.mesh_reach_ticks() == 1 and ks["passes"] == 1 and ks["reach_members"][1] == 1
    assert ks["reach_init"][1] == ks["reach_finish"][1] == 1 and ks["levels"] <= ks["reach_level"][1] <= ks["levels"] + 3
    e.close()


class _NoTransport:
    """Stands in for a transport record: the refusal comes before it is read."""
    c = _abi.TransportC()


def test_partitioned_engine_is_refused():
    words = "mesh reach: not on a partitioned engine"
    # the option first: gs_set_partition refuses
    with pytest.raises(GossipEngineError) as ei:
        scenarios.SCENARIOS["gossipsub_multitopic"](PRODUCT_LIB, (WithMeshReach(HOP, [0]), WithPartition(0, 2, _NoTransport())))
    assert ei.value.code == _abi.GS_EUNSUPPORTED and words in str(ei.value)
    # the partition first: gs_set_mesh_reach refuses
    e, _ = scenarios.SCENARIOS["gossipsub_multitopic"](PRODUCT_LIB)
    tr = _abi.TransportC(None, _abi.ALLGATHER_I64(lambda *a: 0), _abi.ALLGATHER(lambda *a: 0),
                         _abi.ALLTOALLV(lambda *a: 0))  # never called: the engine does not start
    assert e.lib.gs_set_partition(e.h, 0, 2, C.byref(tr)) == _abi.GS_OK
    assert e.lib.gs_set_mesh_reach(e.h, C.byref(_raw())) == _abi.GS_EUNSUPPORTED and _err(e) == words
    e.close()
    # world = 1 is no partition
    e, _ = scenarios.SCENARIOS["gossipsub_multitopic"](PRODUCT_LIB, (WithMeshReach(HOP, [0]),))
    assert e.lib.gs_set_partition(e.h, 0, 1, None) == _abi.GS_OK
    e.close()


# ---------------------------------------------------------------- 5. all three inspectors
def test_three_inspectors_together(oracle_path):
    """Score inspection, mesh health and mesh reach on one engine at period 1:
    each gives the rows it gives alone (the reference's, over the oracle's mesh
    at every hop for the first two; for mesh reach, which also reads the fanout,
    the rows of an engine that runs it alone)."""
    name = "gossipsub_scored"
    r = inspect_ref.ref(oracle_path, name)  # period 1: a tick of all three at every hop
    sources = [7, 0, 150]
    reach = option(sources, ticks=r.ticks, period=r.period)
    e, hops = inspect_ref.builder(name)(PRODUCT_LIB, (reach,))
    e.step(hops)
    alone = [e.mesh_reach_row(k) for k in range(r.ticks)]
    alone_depths = e.mesh_reach_depths()[1]
    e.close()
    opts = (WithPeerScoreInspect(None, r.period * HOP, bounds=r.bounds, ticks=r.ticks),
            WithMeshHealth(r.period * HOP, ticks=r.ticks, labels=True), reach)
    e, hops = inspect_ref.builder(name)(PRODUCT_LIB, opts)
    e.step(hops)
    assert e.inspect_ticks() == e.mesh_health_ticks() == e.mesh_reach_ticks() == r.ticks
    bad = []
    for k in range(r.ticks):
        row = e.inspect_row(k)
        if not (np.array_equal(row["score_hist"], r.score_hist(k)) and np.array_equal(row["mesh_deg"], r.mesh_deg(k))):
            bad.append(f"tick {k}: the score inspector's row differs")
        want = mhref.health(r.rowptr, r.col, r.mesh[k], e.subs, r.T)
        got_row = e.mesh_health_row(k)
        bad += [f"tick {k}: mesh health's {f} differs" for f in mhref.FIELDS + ("comp_hist",)
                if not np.array_equal(got_row[f], want[f])]
        mine = e.mesh_reach_row(k)
        assert mine["hop"] == r.hop(k) == row["hop"] == got_row["hop"] == alone[k]["hop"]
        bad += differences(mine, alone[k], k)
    assert bad == [], "\n".join(bad[:10])
    assert np.array_equal(e.mesh_labels()[1], want["labels"])
    assert np.array_equal(e.mesh_reach_depths()[1], alone_depths)
    # the last tick against the reference over this engine's own readbacks
    assert differences(mine, rref.of_engine(e, sources), r.ticks - 1) == []
    e.close()
