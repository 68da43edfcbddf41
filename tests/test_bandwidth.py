"""Bandwidth statistics (include/gs_bandwidth.h) without a GPU: the Python
option's own checks, the ABI struct against the header, the reference
(tests/bandwidth_ref.py) and its identities, and the preconditions of
tests/test_bandwidth_gpu.py on the oracle alone, so that a pass on the GPU
cannot be vacuous."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bandwidth_ref as bref
import scenarios
from pubsub_amd import (Millisecond, WithBandwidthStats, WithRPCAccounting, _abi, bandwidth_quantiles,
                        default_bandwidth_bounds)

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gs_bandwidth.h")
ALL, EAGER, PULLED, OVERHEAD = bref.ALL, bref.EAGER, bref.PULLED, bref.OVERHEAD
ROWS = bref.CASES + ["acct_odd_203", "acct_floodsub_1gib"]


# ---------------------------------------------------------------- (a) pure Python
def test_option_arguments(oracle_path):
    hop = 100 * Millisecond
    assert default_bandwidth_bounds() == [1] + [4 ** k for k in range(5, 18)]
    assert default_bandwidth_bounds()[1] == 1 << 10 and default_bandwidth_bounds()[-1] == 16 << 30
    key, val = WithBandwidthStats(3 * hop, nodes=[1, 5])
    assert key == "bandwidth" and val["ticks"] == 64 and val["period"] == 3 * hop
    assert val["bounds"].dtype == np.int64 and val["bounds"].tolist() == default_bandwidth_bounds()
    assert WithBandwidthStats(hop, bounds=[])[1]["bounds"].tolist() == []
    for bad in (dict(ticks=0), dict(bounds=[0, 5]), dict(bounds=[-1]), dict(bounds=[5, 5]), dict(bounds=[9, 3]),
                dict(bounds=[1.5, 2.5]), dict(bounds=list(range(1, 65))), dict(bounds=[[1, 2]]),
                dict(bounds=[1, 1 << 63])):
        with pytest.raises(ValueError, match="WithBandwidthStats"):
            WithBandwidthStats(hop, **bad)
    assert len(WithBandwidthStats(hop, bounds=list(range(1, 64)))[1]["bounds"]) == 63
    build = scenarios.SCENARIOS["acct_floodsub"]
    for period in (150 * Millisecond, 0, -hop):
        with pytest.raises(ValueError, match="WithBandwidthStats: period .* multiple of the hop"):
            build(oracle_path, (WithBandwidthStats(period),))
    with pytest.raises(ValueError, match="one entry per host"):
        build(oracle_path, (WithBandwidthStats(hop, nodes=[True, False]),))
    with pytest.raises(ValueError, match="outside 0 .. 19"):
        build(oracle_path, (WithBandwidthStats(hop, nodes=[3, 20]),))
    # valid arguments get as far as the library: the oracle does not export gs_bandwidth.h
    with pytest.raises(ValueError, match="product library only"):
        build(oracle_path, (WithBandwidthStats(hop, nodes=[3, 19]),))


def test_quantiles():
    bounds = [1, 1024, 4096]
    hist = np.array([[10, 0, 0, 0], [1, 1, 1, 1], [0, 0, 0, 0], [0, 50, 49, 1]])
    q = bandwidth_quantiles(hist, bounds, [0.5, 0.99, 1])
    assert q.dtype == np.int64 and q.tolist() == [[1, 1, 1], [1024, -1, -1], [-1, -1, -1], [1024, 4096, -1]]
    with pytest.raises(ValueError):
        bandwidth_quantiles(hist[:, :3], bounds, [0.5])


def test_abi_against_header():
    S = _abi.BandwidthConfigC
    assert C.sizeof(S) == 32
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [
        ("period_hops", 0), ("ticks", 8), ("num_bounds", 12), ("bounds", 16), ("node_mask", 24)]
    text = open(HEADER).read()
    struct = re.search(r"typedef struct gs_bandwidth_config \{(.*?)\} gs_bandwidth_config;", text, re.S).group(1)
    fields = re.findall(r"^\s*(?:const )?(\w+)\*? (\w+);", struct, re.M)
    assert [n for _, n in fields] == [n for n, _ in S._fields_]
    assert [t for t, _ in fields] == ["int64_t", "int32_t", "int32_t", "int64_t", "uint8_t"]
    assert int(re.search(r"#define GS_BW_MAX_BOUNDS (\d+)", text).group(1)) == _abi.GS_BW_MAX_BOUNDS
    # every function of the header is bound, with as many arguments as it declares
    decl = {m.group(1): m.group(2) for m in re.finditer(r"^int(?:64_t)? (gs_\w+)\((.*?)\);", text, re.M | re.S)}
    assert sorted(decl) == sorted(n for n, _, _ in _abi.BANDWIDTH_FUNCTIONS)
    for name, _, args in _abi.BANDWIDTH_FUNCTIONS:
        assert len(args) == decl[name].count(",") + 1, name
    enum = lambda first: re.search(r"enum \{\s*" + first + r"(.*?)\};", text, re.S).group(0)
    assert len(_abi.BW_DIRS) == enum("GS_BW_EGRESS").count(",") and len(_abi.BW_CLASSES) == enum("GS_BW_ALL").count(",")
    assert len(_abi.BANDWIDTH_KERNEL_NAMES) == len(re.findall(r"GS_BW_K_\w+", enum("GS_BW_K_TICK")))


# ---------------------------------------------------------------- (b) the reference by hand
def test_ref_by_hand():
    """Three hosts on a path 0 - 1 - 2; edges in CSR order 0>1, 1>0, 1>2, 2>1."""
    rowptr, col = np.array([0, 1, 3, 4]), np.array([1, 0, 2, 1])
    pn = bref.per_node(rowptr, col, np.array([10, 1024, 5, 0], dtype=np.int64))
    assert pn.tolist() == [[10, 1029, 0], [1024, 10, 5]]
    split = np.zeros((2, 2, 3), dtype=np.int64)
    split[0, 0, 1], split[0, 1, 0] = 1000, 1000  # host 1 pushed 1000 bytes to host 0
    v = bref.with_classes(pn, split)
    assert v[0, OVERHEAD].tolist() == [10, 29, 0] and v[1, OVERHEAD].tolist() == [24, 10, 5]
    row = bref.row_of(v, bref.per_node(rowptr, col, np.array([1, 3, 1, 0], dtype=np.int64)), np.array([1, 10, 1024]))
    assert row["total"].tolist() == [1039, 1000, 0, 39] and row["total_rpcs"] == 5
    # a value equal to a bound goes to the upper bin; bin 0 holds the silent host
    assert row["hist"][0, ALL].tolist() == [1, 0, 1, 1] and row["hist"][1, ALL].tolist() == [0, 1, 1, 1]
    assert row["hist"][0, PULLED].tolist() == [3, 0, 0, 0] and (row["hist"].sum(axis=2) == 3).all()
    assert row["max"].tolist() == [[1029, 1000, 0, 29], [1024, 1000, 0, 24]]
    assert row["argmax"].tolist() == [[1, 1, -1, 1], [0, 0, -1, 0]]


def test_pb_field_is_the_size_model():
    assert [bref.pb_field(n) for n in (0, 127, 128, 16383, 16384, 1 << 30)] == [2, 129, 131, 16386, 16388, (1 << 30) + 6]


# ---------------------------------------------------------------- (c) the oracle alone
@pytest.mark.parametrize("name", ROWS)
def test_reference_identities(oracle_path, name):
    r = bref.ref(oracle_path, name)
    assert r.ticks >= 7
    v = np.array(r.values)  # [ticks, 2, 4, N]
    n = np.array(r.rpcs)    # [ticks, 2, N]
    tot = v.sum(axis=3)
    assert np.array_equal(tot[:, bref.EGRESS], tot[:, bref.INGRESS])  # per class
    assert np.array_equal(n[:, 0].sum(axis=1), n[:, 1].sum(axis=1))
    assert v.min() >= 0 and n.min() >= 0  # overhead = all - eager - pulled included
    # the ticks sum to the final cumulative totals
    cum = bref.per_node(r.rowptr, r.col, r.cum_bytes)
    assert np.array_equal(v[:, :, ALL].sum(axis=0), cum)
    assert np.array_equal(n.sum(axis=0), bref.per_node(r.rowptr, r.col, r.cum_rpcs))
    assert tot[:, 0, ALL].sum() == r.cum_bytes.sum() and tot[:, 0, EAGER].sum() > 0
    # every RPC is traced except the hello packets, which exist at tick 0
    hello = n[:, 0].sum(axis=1) - r.sends
    assert (hello >= 0).all() and hello[0] > 0
    for k in range(r.ticks):
        row = r.row(k)
        assert (row["hist"].sum(axis=2) == r.N).all()
        assert (row["argmax"] >= 0).tolist() == (row["max"] > 0).tolist()


@pytest.mark.parametrize("name", ROWS)
def test_preconditions(oracle_path, name):
    r = bref.ref(oracle_path, name)
    v = np.array(r.values)
    # at least three bins populated in each direction for `all`, at some tick
    pop = np.array([(r.row(k)["hist"][:, ALL] > 0).sum(axis=1) for k in range(r.ticks)])
    assert (pop.max(axis=0) >= 3).all(), pop.tolist()
    # overhead at some tick, and payload pulled through IWANT where the router has gossip
    assert v[:, 0, OVERHEAD].sum(axis=1).max() > 0
    gossip = "floodsub" not in name and "randomsub" not in name
    assert (v[:, 0, PULLED].sum() > 0) == gossip
    # one bound equals a per-node value that occurs: the upper-bin rule
    mid = r.values[r.ticks // 2][bref.EGRESS, ALL]
    assert all(b in r.bounds and (mid == b).any() for b in r.exact_bounds) and len(r.exact_bounds) >= 1
    k = int(np.searchsorted(r.bounds, r.exact_bounds[0]))
    assert r.row(r.ticks // 2)["hist"][0, ALL, k + 1] >= 1
    assert len(r.bounds) <= _abi.GS_BW_MAX_BOUNDS and len(r.observers) >= 5


def test_ladder_samples_every_kind_of_row(oracle_path):
    r = bref.ref(oracle_path, "acct_ladder_multitopic")
    deg = np.diff(r.rowptr)[r.observers]
    assert 64 in deg and 1 in deg and 0 in deg
    b = np.array([r.sampled(k)[0] for k in range(r.ticks)])  # [ticks, nS, 2, 4]
    silent = r.observers[int(np.flatnonzero(deg == 0)[0])]
    # (nothing is sent in the last period: the run's tail past the last heartbeat)
    assert silent == 158 and not b[:, deg == 0].any() and b[:-1, deg == 64, :, ALL].min() > 0
    assert r.period == 7 and r.ticks == 17


def test_churn_has_hello_packets_after_tick_0(oracle_path):
    r = bref.ref(oracle_path, "acct_churn")
    hello = np.array(r.rpcs)[:, 0].sum(axis=1) - r.sends
    assert hello[0] == r.E and (hello[1:] > 0).any()
    # the static scenarios: tick 0 only
    s = bref.ref(oracle_path, "acct_ladder_multitopic")
    hello = np.array(s.rpcs)[:, 0].sum(axis=1) - s.sends
    assert hello[0] == s.E and not hello[1:].any()


def test_1gib_messages_pass_2_to_the_32(oracle_path):
    r = bref.ref(oracle_path, "acct_floodsub_1gib")
    v = np.array(r.values)
    assert v[:, :, ALL].max() > 1 << 36 and (r.bounds[1:] >= 1 << 32).all()
    assert min(r.exact_bounds) > 1 << 32
    hist = np.array([r.row(k)["hist"][:, ALL] for k in range(r.ticks)])
    assert hist[:, :, 2:].sum() > 0 and r.row(r.ticks // 2)["total"][EAGER] > 1 << 40


def test_big_case_needs_more_than_one_pass(oracle_path):
    """k_bw_tick's grid is capped at 8 workgroups of 4 nodes per CU: 8,192
    nodes per pass on a 256-CU device."""
    probe, hops = bref.builder(bref.BIG)(oracle_path)
    assert probe.N == 20011 > 2 * 8 * 4 * 256 and hops // bref.BIG_PERIOD == 25
    probe.close()


def test_option_order_does_not_matter(oracle_path):
    """The option applies itself after WithRPCAccounting wherever it stands:
    both orders get as far as the library."""
    acct = WithRPCAccounting(100)
    for extra in ((acct, WithBandwidthStats(100 * Millisecond)), (WithBandwidthStats(100 * Millisecond), acct)):
        with pytest.raises(ValueError, match="product library only"):
            scenarios.SCENARIOS["gossipsub_dense"](oracle_path, extra)
