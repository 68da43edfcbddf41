"""Bandwidth statistics on the device (include/gs_bandwidth.h) against the
reference (tests/bandwidth_ref.py) over the oracle stepped in pieces.  Every
comparison is exact.  Each scenario runs once on the GPU, as one single
step(hops) with the observers of inspect_ref.observers_of sampled, and every
test reads that run.  tests/test_bandwidth.py holds the scenarios'
preconditions."""
import ctypes as C
import functools

import numpy as np
import pytest

import bandwidth_ref as bref
import scenarios
from pubsub_amd import PRODUCT_LIB, GossipEngineError, WithBandwidthStats, WithPartition, _abi

pytestmark = pytest.mark.gpu
HOP = scenarios.HOP
ALL, EAGER, PULLED, OVERHEAD = bref.ALL, bref.EAGER, bref.PULLED, bref.OVERHEAD


def option(r, ticks=None, nodes=True):
    return WithBandwidthStats(r.period * HOP, bounds=r.bounds, nodes=r.observers if nodes else None,
                              ticks=max(64, r.ticks) if ticks is None else ticks)


class Got:
    """One run on the GPU with the statistics on, every tick read back."""

    def __init__(self, r):
        e, hops = bref.builder(r.name)(PRODUCT_LIB, (option(r),))
        assert hops == r.hops
        assert e.bandwidth_ticks() == 0
        e.step(hops)
        self.ticks = e.bandwidth_ticks()
        self.nodes = e.bandwidth_nodes()
        self.rows = [e.bandwidth_row(k) for k in range(self.ticks)]
        self.sampled = [e.bandwidth_sampled(k) for k in range(self.ticks)]
        self.final = scenarios.snapshot(e, getattr(e, "snapshot_ids", range(e.n_published)))
        e.close()


@functools.lru_cache(maxsize=None)
def got(oracle, name, classes=True, period=None):
    return Got(bref.ref(oracle, name, classes, period))


def check_shapes(r, g):
    assert g.ticks == r.ticks > 0
    assert g.nodes.dtype == np.int32 and g.nodes.tolist() == r.observers
    nb = len(r.bounds)
    for k in range(r.ticks):
        row = g.rows[k]
        assert row["hop"] == r.hop(k)
        assert row["total"].dtype == np.int64 and row["total"].shape == (4,)
        assert row["hist"].dtype == np.int64 and row["hist"].shape == (2, 4, nb + 1)
        assert row["max"].shape == row["argmax"].shape == (2, 4)
        # the identities: every histogram row holds every node; the classes add up
        assert (row["hist"].sum(axis=2) == r.N).all(), f"tick {k}"
        assert row["total"][ALL] == row["total"][1:].sum() and row["total"].min() >= 0
        assert (row["argmax"] >= 0).tolist() == (row["max"] > 0).tolist(), f"tick {k}"
        b, n = g.sampled[k]
        assert b.shape == (len(r.observers), 2, 4) and n.shape == (len(r.observers), 2) and b.min() >= 0
        assert np.array_equal(b[:, :, ALL], b[:, :, 1:].sum(axis=2))
        assert (b[:, :, ALL].max(axis=0) <= row["max"][:, ALL]).all()


# ---------------------------------------------------------------- 1. scenario parity
@pytest.mark.parametrize("name", bref.CASES + ["acct_odd_203"])
def test_rows_and_sampled_equal_reference(oracle_path, name):
    r, g = bref.ref(oracle_path, name), got(oracle_path, name)
    check_shapes(r, g)
    bad = []
    for k in range(r.ticks):
        bad += bref.differences(g.rows[k], r.row(k), k)
        wb, wn = r.sampled(k)
        if not np.array_equal(g.sampled[k][0], wb):
            bad.append(f"tick {k}: sampled bytes differ at (node, dir, class) "
                       f"{np.argwhere(g.sampled[k][0] != wb)[:5].tolist()}")
        if not np.array_equal(g.sampled[k][1], wn):
            bad.append(f"tick {k}: sampled RPC counts differ")
    assert bad == [], "\n".join(bad[:10])


def test_values_above_2_to_the_32(oracle_path):
    """1 GiB messages over floodsub and bounds above 2^32: totals, maxima and
    bins are 64-bit all the way."""
    name = "acct_floodsub_1gib"
    r, g = bref.ref(oracle_path, name), got(oracle_path, name)
    check_shapes(r, g)
    bad = []
    for k in range(r.ticks):
        bad += bref.differences(g.rows[k], r.row(k), k)
        if not (np.array_equal(g.sampled[k][0], r.sampled(k)[0]) and np.array_equal(g.sampled[k][1], r.sampled(k)[1])):
            bad.append(f"tick {k}: sampled nodes differ")
    assert bad == [], "\n".join(bad[:10])
    assert max(int(row["max"][0, ALL]) for row in g.rows) > 1 << 36
    assert sum(int(row["hist"][0, ALL, 2:].sum()) for row in g.rows) > 0


def test_more_nodes_than_one_pass_of_the_grid(oracle_path):
    """gossipsub_scored(n=20011, k=6): k_bw_tick's grid covers 8 workgroups x 4
    nodes per CU in a pass (8,192 nodes on 256 CUs), so the node loop runs three
    times with a ragged end.  `all` and the RPC counts against the oracle
    (without its trace), the classes by their identities."""
    r, g = bref.ref(oracle_path, bref.BIG, False, bref.BIG_PERIOD), got(oracle_path, bref.BIG, False, bref.BIG_PERIOD)
    assert r.N == 20011 > 2 * 8 * 4 * 256
    check_shapes(r, g)
    bad = []
    pulled = 0
    for k in range(r.ticks):
        row, want = g.rows[k], r.row(k)
        pulled += int(row["total"][PULLED])
        if row["total"][ALL] != want["total"][ALL] or row["total_rpcs"] != want["total_rpcs"]:
            bad.append(f"tick {k}: totals {row['total'][ALL]}, {row['total_rpcs']} != "
                       f"{want['total'][ALL]}, {want['total_rpcs']}")
        for f in ("hist", "max", "argmax"):
            if not np.array_equal(row[f][:, ALL], want[f][:, ALL]):
                bad.append(f"tick {k}: {f} of `all` differs")
        wb, wn = r.sampled(k)
        if not (np.array_equal(g.sampled[k][0][:, :, ALL], wb[:, :, ALL]) and np.array_equal(g.sampled[k][1], wn)):
            bad.append(f"tick {k}: sampled nodes differ")
    assert bad == [], "\n".join(bad[:10])
    # degree 6 = D: every peer is in the mesh, nothing is left to gossip to, nothing is pulled
    # (the oracle's trace of this scenario holds no served message either)
    assert pulled == 0 and max(int(row["total"][EAGER]) for row in g.rows) > 0


def test_ladder_equals_own_rpc_bytes_differences(oracle_path):
    """The ticks against rpc_bytes() of a second engine without the statistics,
    stepped a period at a time: tells a statistics error from a disagreement of
    the accounting with the oracle."""
    name = "acct_ladder_multitopic"
    r, g = bref.ref(oracle_path, name), got(oracle_path, name)
    e, _ = bref.builder(name)(PRODUCT_LIB)
    pb, pn = np.zeros(r.E, dtype=np.int64), np.zeros(r.E, dtype=np.int64)
    obs = np.array(r.observers)
    for k in range(r.ticks):
        e.step(r.period)
        b, n = e.rpc_bytes()
        vb, vn = bref.per_node(r.rowptr, r.col, b - pb), bref.per_node(r.rowptr, r.col, n - pn)
        pb, pn = b, n
        row = g.rows[k]
        assert row["total"][ALL] == vb[0].sum() and row["total_rpcs"] == vn[0].sum(), f"tick {k}"
        assert np.array_equal(row["max"][:, ALL], vb.max(axis=1)), f"tick {k}"
        assert np.array_equal(row["argmax"][:, ALL], np.where(vb.max(axis=1) > 0, vb.argmax(axis=1), -1)), f"tick {k}"
        for dr in range(2):
            want = np.bincount(np.searchsorted(r.bounds, vb[dr], side="right"), minlength=len(r.bounds) + 1)
            assert np.array_equal(row["hist"][dr, ALL], want), f"tick {k}"
        assert np.array_equal(g.sampled[k][0][:, :, ALL], vb[:, obs].T), f"tick {k}"
        assert np.array_equal(g.sampled[k][1], vn[:, obs].T), f"tick {k}"
    e.close()


# ---------------------------------------------------------------- 2. ring of ticks and errors
def test_ring_and_read_codes(oracle_path):
    name = "acct_multitopic"
    r = bref.ref(oracle_path, name)
    assert r.ticks == 12
    e, hops = bref.builder(name)(PRODUCT_LIB, (option(r, ticks=4),))
    e.set_profiling(True)
    e.step(hops)
    assert e.bandwidth_ticks() == 12
    for k in range(8, 12):
        row = e.bandwidth_row(k)
        assert row["hop"] == r.hop(k) and bref.differences(row, r.row(k), k) == []
        assert np.array_equal(e.bandwidth_sampled(k)[0], r.sampled(k)[0])
    for k, code in [(j, _abi.GS_ESTATE) for j in range(8)] + [(12, _abi.GS_EINVAL), (-1, _abi.GS_EINVAL)]:
        for call in (e.bandwidth_row, e.bandwidth_sampled):
            with pytest.raises(GossipEngineError) as ei:
                call(k)
            assert ei.value.code == code, (k, str(ei.value))
    ks = e.bandwidth_kernel_stats()
    assert [ks[n][1] for n in _abi.BANDWIDTH_KERNEL_NAMES] == [12, 12, 12] and all(v[0] > 0 for v in ks.values())
    e.close()
    # no sampled nodes: valid, and nothing to gather
    e, hops = bref.builder(name)(PRODUCT_LIB, (option(r, nodes=False),))
    e.step(2 * r.period)
    assert e.bandwidth_ticks() == 2 and len(e.bandwidth_nodes()) == 0 and e.bandwidth_sampled(1)[0].shape == (0, 2, 4)
    assert bref.differences(e.bandwidth_row(1), r.row(1), 1) == []
    e.close()


def _raw(period=1, ticks=1, bounds=(1,), mask=None):
    b = np.array(bounds, dtype=np.int64)
    cfg = _abi.BandwidthConfigC(period, ticks, len(b), b.ctypes.data_as(C.POINTER(C.c_int64)),
                                mask.ctypes.data_as(C.POINTER(C.c_uint8)) if mask is not None else None)
    cfg._keep = (b, mask)
    return cfg


def _err(e):
    return e.lib.gs_last_error().decode()


def test_refusals():
    opt = WithBandwidthStats(HOP)
    # without the accounting
    with pytest.raises(GossipEngineError) as ei:
        scenarios.SCENARIOS["gossipsub_multitopic"](PRODUCT_LIB, (opt,))
    assert ei.value.code == _abi.GS_ESTATE and "RPC accounting is off" in str(ei.value)
    # a second call
    e, _ = scenarios.SCENARIOS["acct_floodsub"](PRODUCT_LIB, (opt,))
    assert e.lib.gs_set_bandwidth_stats(e.h, C.byref(_raw())) == _abi.GS_ESTATE
    assert _err(e) == "duplicate bandwidth statistics"
    # before the first tick
    assert e.bandwidth_ticks() == 0
    with pytest.raises(GossipEngineError) as ei:
        e.bandwidth_row(0)
    assert ei.value.code == _abi.GS_EINVAL
    e.step(2)
    assert e.bandwidth_ticks() == 2 and e.bandwidth_row(1)["hop"] == 2 == e.hop
    e.close()
    # bad arguments, each with a text of its own; nothing is set by a refused call
    e, _ = scenarios.SCENARIOS["acct_floodsub"](PRODUCT_LIB)
    texts = set()
    for cfg in (_raw(period=0), _raw(period=-3), _raw(ticks=0), _raw(bounds=list(range(1, 65))), _raw(bounds=[0, 5]),
                _raw(bounds=[-4]), _raw(bounds=[5, 5]), _raw(bounds=[9, 3])):
        assert e.lib.gs_set_bandwidth_stats(e.h, C.byref(cfg)) == _abi.GS_EINVAL
        texts.add(_err(e))
    assert len(texts) == 4
    assert e.lib.gs_set_bandwidth_stats(e.h, None) == _abi.GS_EINVAL
    # the statistics off: every read is refused, before and after the start
    for _ in range(2):
        for call in (e.bandwidth_ticks, e.bandwidth_nodes, e.bandwidth_kernel_stats, lambda: e.bandwidth_row(0),
                     lambda: e.bandwidth_sampled(0)):
            with pytest.raises(GossipEngineError) as ei:
                call()
            assert ei.value.code == _abi.GS_ESTATE
        e.step(1)
    # after the first step
    assert e.lib.gs_set_bandwidth_stats(e.h, C.byref(_raw())) == _abi.GS_ESTATE
    assert "before the first step" in _err(e)
    e.close()
    # 63 bounds: valid
    b63 = [1 << k for k in range(63)]
    e, _ = scenarios.SCENARIOS["acct_floodsub"](PRODUCT_LIB, (WithBandwidthStats(2 * HOP, bounds=b63),))
    e.step(4)
    row = e.bandwidth_row(1)
    assert e.bandwidth_ticks() == 2 and row["hop"] == 4 and row["hist"].shape == (2, 4, 64)
    assert (row["hist"].sum(axis=2) == e.N).all()
    e.close()


class _NoTransport:
    """Stands in for a transport record: the refusal comes before it is read."""
    c = _abi.TransportC()


def test_partitioned_engine_is_refused():
    words = "bandwidth statistics: not on a partitioned engine"
    # the option first: gs_set_partition refuses
    with pytest.raises(GossipEngineError) as ei:
        scenarios.SCENARIOS["acct_floodsub"](PRODUCT_LIB, (WithBandwidthStats(HOP), WithPartition(0, 2, _NoTransport())))
    assert ei.value.code == _abi.GS_EUNSUPPORTED and words in str(ei.value)
    # the partition first: gs_set_bandwidth_stats refuses
    e, _ = scenarios.SCENARIOS["acct_floodsub"](PRODUCT_LIB)
    tr = _abi.TransportC(None, _abi.ALLGATHER_I64(lambda *a: 0), _abi.ALLGATHER(lambda *a: 0),
                         _abi.ALLTOALLV(lambda *a: 0))  # never called: the engine does not start
    assert e.lib.gs_set_partition(e.h, 0, 2, C.byref(tr)) == _abi.GS_OK
    assert e.lib.gs_set_bandwidth_stats(e.h, C.byref(_raw())) == _abi.GS_EUNSUPPORTED and _err(e) == words
    e.close()
    # world = 1 is no partition
    e, _ = scenarios.SCENARIOS["acct_floodsub"](PRODUCT_LIB, (WithBandwidthStats(HOP),))
    assert e.lib.gs_set_partition(e.h, 0, 1, None) == _abi.GS_OK
    e.close()


# ---------------------------------------------------------------- 3. nothing else moves
@pytest.mark.parametrize("name", ["acct_adversarial", "acct_churn", "acct_ladder_multitopic"])
def test_nothing_else_moves(oracle_path, name):
    """The run with the statistics on ends in the state of the run without
    them, the final rpc_bytes included."""
    e, hops = scenarios.SCENARIOS[name](PRODUCT_LIB)
    e.step(hops)
    plain = scenarios.snapshot(e, getattr(e, "snapshot_ids", range(e.n_published)))
    e.close()
    assert "rpc_bytes" in plain and plain["rpc_bytes"].sum() > 0
    bad = scenarios.compare(plain, got(oracle_path, name).final)
    assert bad == [], "\n".join(bad)
