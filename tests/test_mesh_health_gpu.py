"""Mesh health on the device (include/gs_mesh_health.h) against the reference
(tests/mesh_health_ref.py) over the oracle stepped in pieces.  Every comparison
is exact.  Each case runs once on the GPU, as one single step(hops) with a tick
per heartbeat and the labels kept, and every test reads that run.
tests/test_mesh_health.py holds the cases' preconditions."""
import ctypes as C
import functools

import numpy as np
import pytest

import inspect_ref
import mesh_health_ref as mref
import scenarios
from pubsub_amd import PRODUCT_LIB, GossipEngineError, WithMeshHealth, WithPartition, WithPeerScoreInspect, _abi

pytestmark = pytest.mark.gpu
HOP = scenarios.HOP
ROW = mref.FIELDS + ("comp_hist",)


def option(mask=None, ticks=64, labels=True, period=mref.PERIOD):
    return WithMeshHealth(period * HOP, nodes=mask, ticks=ticks, labels=labels)


def differences(got, want, k):
    return [f"tick {k}: {f} {np.asarray(got[f]).tolist()} != {np.asarray(want[f]).tolist()}" for f in ROW
            if not np.array_equal(got[f], want[f])]


# ---------------------------------------------------------------- 1. the ring's closed form
def test_ring_closed_form():
    e = mref.ring_engine(PRODUCT_LIB, (option(ticks=8),))
    assert e.mesh_health_ticks() == 0
    e.step(mref.RING_HOPS)
    assert e.mesh_health_ticks() == 5
    for k in range(5):
        row = e.mesh_health_row(k)
        assert row["hop"] == (k + 1) * mref.PERIOD
        for f in ROW:
            assert row[f].dtype == np.int64 and row[f].shape == ((2, 32) if f == "comp_hist" else (2,))
        for t in range(2):
            assert tuple(int(row[f][t]) for f in mref.FIELDS[:5]) == mref.ring_want(k), (k, t)
            assert int(row["outside"][t]) == 0 and int(row["eclipsed"][t]) == 0
            sizes = np.zeros(32, dtype=np.int64)
            sizes[7 if k < 2 else 6] = 1 if k < 2 else 2  # one component of 200, then two of 100
            assert np.array_equal(row["comp_hist"][t], sizes)
    tick, lab = e.mesh_labels()
    assert tick == 4 and lab.dtype == np.int32 and np.array_equal(lab, mref.ring_labels())
    ks = e.mesh_health_kernel_stats()
    # an arc's diameter is 99: without shortening and hooking the three ticks after the cut alone
    # would take 3 x 99 iterations
    print(f"ring: {ks['iterations']} label iterations over 5 ticks, {ks['bytes']} bytes")
    assert 5 <= ks["iterations"] < mref.RING_N
    e.close()


@pytest.mark.parametrize("topics,n", [(1, 200), (40, 130)])
def test_ring_other_lane_layouts(topics, n):
    """64 hosts per wave (T = 1) and a wave per host with idle lanes (T = 40),
    with a host count that fills no last wave; against the reference over the
    engine's own mesh readback."""
    e = mref.ring_engine(PRODUCT_LIB, (option(),), topics=topics, n=n)
    e.step(mref.RING_HOPS)
    row = e.mesh_health_row(4)
    want = mref.of_engine(e)
    assert differences(row, want, 4) == []
    for t in range(topics):
        assert tuple(int(row[f][t]) for f in mref.FIELDS[:5]) == mref.ring_want(4, n)
    assert np.array_equal(e.mesh_labels()[1], mref.ring_labels(topics, n))
    e.close()


# ---------------------------------------------------------------- 2. scenario parity
class Got:
    """One run on the GPU with mesh health on, every tick read back."""

    def __init__(self, oracle, name, key):
        r = mref.ref(oracle, name, key)
        e, hops = scenarios.SCENARIOS[name](PRODUCT_LIB, (option(r.mask),))
        assert hops == r.hops
        e.step(hops)
        self.ticks = e.mesh_health_ticks()
        self.rows = [e.mesh_health_row(k) for k in range(self.ticks)]
        self.label_tick, self.labels = e.mesh_labels()
        self.stats = e.mesh_health_kernel_stats()
        self.final = scenarios.snapshot(e, getattr(e, "snapshot_ids", range(e.n_published)))
        e.close()


@functools.lru_cache(maxsize=None)
def got(oracle, name, key):
    return Got(oracle, name, key)


@pytest.mark.parametrize("name,key", mref.CASES)
def test_rows_and_labels_equal_reference(oracle_path, name, key):
    r, g = mref.ref(oracle_path, name, key), got(oracle_path, name, key)
    assert g.ticks == r.ticks > 0
    bad = []
    for k in range(r.ticks):
        assert g.rows[k]["hop"] == r.hop(k)
        bad += differences(g.rows[k], r.rows[k], k)
    assert bad == [], "\n".join(bad[:10])
    assert g.label_tick == r.ticks - 1
    assert np.array_equal(g.labels, r.labels), np.argwhere(g.labels != r.labels)[:5].tolist()
    print(f"{name}: {g.stats['iterations']} label iterations over {g.ticks} ticks")
    assert g.ticks <= g.stats["iterations"] < g.ticks * r.N


@pytest.mark.parametrize("name,key", mref.CASES)
def test_nothing_else_moves(oracle_path, name, key):
    """The run with mesh health on ends in the oracle's final state."""
    bad = scenarios.compare(mref.ref(oracle_path, name, key).final, got(oracle_path, name, key).final)
    assert bad == [], "\n".join(bad)


# ---------------------------------------------------------------- 3. ring of ticks and errors
def _raw(period=1, ticks=1, mask=None, labels=0):
    cfg = _abi.MeshHealthConfigC(period, ticks, mask.ctypes.data_as(C.POINTER(C.c_uint8)) if mask is not None else None,
                                 labels)
    cfg._keep = mask
    return cfg


def _err(e):
    return e.lib.gs_last_error().decode()


def test_tick_ring():
    e = mref.ring_engine(PRODUCT_LIB, (option(ticks=2, labels=False),))
    e.step(mref.RING_HOPS)
    assert e.mesh_health_ticks() == 5
    for k in (3, 4):
        row = e.mesh_health_row(k)
        assert row["hop"] == (k + 1) * mref.PERIOD
        assert tuple(int(row[f][0]) for f in mref.FIELDS[:5]) == mref.ring_want(k)
    for k, code in [(0, _abi.GS_ESTATE), (1, _abi.GS_ESTATE), (2, _abi.GS_ESTATE), (5, _abi.GS_EINVAL),
                    (-1, _abi.GS_EINVAL)]:
        with pytest.raises(GossipEngineError) as ei:
            e.mesh_health_row(k)
        assert ei.value.code == code, (k, str(ei.value))
    with pytest.raises(GossipEngineError) as ei:  # labels = 0: no label table
        e.mesh_labels()
    assert ei.value.code == _abi.GS_ESTATE
    e.close()


def test_refusals():
    opt = WithMeshHealth(HOP)
    for name in ("floodsub_dense", "randomsub_100"):
        with pytest.raises(GossipEngineError) as ei:
            scenarios.SCENARIOS[name](PRODUCT_LIB, (opt,))
        assert ei.value.code == _abi.GS_EUNSUPPORTED and "pubsub router is not gossipsub" in str(ei.value)
    # scoring is not needed
    e, _ = scenarios.SCENARIOS["gossipsub_dense"](PRODUCT_LIB, (opt,))
    # a second call
    assert e.lib.gs_set_mesh_health(e.h, C.byref(_raw())) == _abi.GS_ESTATE
    assert _err(e) == "duplicate mesh health inspector"
    # before the first tick
    assert e.mesh_health_ticks() == 0
    with pytest.raises(GossipEngineError) as ei:
        e.mesh_health_row(0)
    assert ei.value.code == _abi.GS_EINVAL
    e.step(2)
    assert e.mesh_health_ticks() == 2 and e.mesh_health_row(1)["hop"] == 2
    e.close()
    # bad arguments, each with a text of its own; nothing is set by a refused call
    e, _ = scenarios.SCENARIOS["gossipsub_multitopic"](PRODUCT_LIB)
    texts = set()
    for cfg in (_raw(period=0), _raw(period=-3), _raw(ticks=0)):
        assert e.lib.gs_set_mesh_health(e.h, C.byref(cfg)) == _abi.GS_EINVAL
        texts.add(_err(e))
    assert len(texts) == 2
    assert e.lib.gs_set_mesh_health(e.h, None) == _abi.GS_EINVAL
    # mesh health off: every read is refused, before and after the start
    for _ in range(2):
        for call in (e.mesh_health_ticks, e.mesh_labels, e.mesh_health_kernel_stats, lambda: e.mesh_health_row(0)):
            with pytest.raises(GossipEngineError) as ei:
                call()
            assert ei.value.code == _abi.GS_ESTATE
        e.step(1)
    # after the first step
    assert e.lib.gs_set_mesh_health(e.h, C.byref(_raw())) == _abi.GS_ESTATE
    assert "before the first step" in _err(e)
    e.close()


class _NoTransport:
    """Stands in for a transport record: the refusal comes before it is read."""
    c = _abi.TransportC()


def test_partitioned_engine_is_refused():
    words = "mesh health: not on a partitioned engine"
    # the option first: gs_set_partition refuses
    with pytest.raises(GossipEngineError) as ei:
        scenarios.SCENARIOS["gossipsub_multitopic"](PRODUCT_LIB, (WithMeshHealth(HOP), WithPartition(0, 2, _NoTransport())))
    assert ei.value.code == _abi.GS_EUNSUPPORTED and words in str(ei.value)
    # the partition first: gs_set_mesh_health refuses
    e, _ = scenarios.SCENARIOS["gossipsub_multitopic"](PRODUCT_LIB)
    tr = _abi.TransportC(None, _abi.ALLGATHER_I64(lambda *a: 0), _abi.ALLGATHER(lambda *a: 0),
                         _abi.ALLTOALLV(lambda *a: 0))  # never called: the engine does not start
    assert e.lib.gs_set_partition(e.h, 0, 2, C.byref(tr)) == _abi.GS_OK
    assert e.lib.gs_set_mesh_health(e.h, C.byref(_raw())) == _abi.GS_EUNSUPPORTED and _err(e) == words
    e.close()
    # world = 1 is no partition
    e, _ = scenarios.SCENARIOS["gossipsub_multitopic"](PRODUCT_LIB, (WithMeshHealth(HOP),))
    assert e.lib.gs_set_partition(e.h, 0, 1, None) == _abi.GS_OK
    e.close()


# ---------------------------------------------------------------- 4. both inspectors
def test_two_inspectors_together(oracle_path):
    name = "gossipsub_scored"
    r = inspect_ref.ref(oracle_path, name)  # period 1: a tick of both at every hop
    opts = (WithPeerScoreInspect(None, r.period * HOP, bounds=r.bounds, ticks=r.ticks),
            option(ticks=r.ticks, period=r.period))
    e, hops = inspect_ref.builder(name)(PRODUCT_LIB, opts)
    e.step(hops)
    assert e.inspect_ticks() == e.mesh_health_ticks() == r.ticks
    bad = []
    for k in range(r.ticks):
        row = e.inspect_row(k)
        if not (np.array_equal(row["score_hist"], r.score_hist(k)) and np.array_equal(row["mesh_deg"], r.mesh_deg(k))):
            bad.append(f"tick {k}: the score inspector's row differs")
        want = mref.health(r.rowptr, r.col, r.mesh[k], e.subs, r.T)
        got_row = e.mesh_health_row(k)
        assert got_row["hop"] == r.hop(k) == row["hop"]
        bad += differences(got_row, want, k)
    assert bad == [], "\n".join(bad[:10])
    assert np.array_equal(e.mesh_labels()[1], want["labels"])
    e.close()
