"""Latency statistics (include/gs_latency.h), the parts that need no GPU: the
product-only boundary, latency_quantiles, and, on the oracle alone, the
preconditions of tests/test_latency_gpu.py: the reference built from the
oracle's per-message deliveries (tests/latency_ref.py) counts exactly what
gs_counters.deliveries counts, and every scenario still has the size and the
largest first-delivery age it was chosen for."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import latency_ref
from pubsub_amd import PRODUCT_LIB, WithLatencyStats, _abi, latency_quantiles

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_product_exports_latency_header():
    """include/gs_latency.h is product-only and bound through _abi.LATENCY_FUNCTIONS."""
    if not os.path.exists(PRODUCT_LIB):
        pytest.skip("product library not built")
    src = open(os.path.join(REPO, "include", "gs_latency.h")).read()
    names = set(re.findall(r"^[a-z_0-9 \*]+?\b(gs_[a-z_0-9]+)\(", src, re.M))
    assert {"gs_set_latency_stats", "gs_latency_bins", "gs_read_latency_hist", "gs_reset_latency_stats",
            "gs_read_message_latency"} <= names
    assert names == {n for n, _, _ in _abi.LATENCY_FUNCTIONS}
    lib = C.CDLL(PRODUCT_LIB)
    for name in names:
        assert hasattr(lib, name), f"product library does not export {name}"
    # gossip_engine.h (what the oracle must export too) does not declare them
    assert not names & {n for n, _, _ in _abi.ABI_FUNCTIONS}


def test_oracle_refuses_the_option(oracle_path):
    with pytest.raises(ValueError, match="product library only"):
        latency_ref.builder("gossipsub_dense")(oracle_path, (WithLatencyStats(),))


def test_latency_quantiles():
    qs = (0.5, 0.95, 1.0)
    rows = np.array([
        [0, 0, 0, 0, 0],    # empty
        [0, 0, 7, 0, 0],    # a single bin
        [0, 5, 5, 0, 0],    # a tie exactly at q = 0.5: age 1 has reached it
        [0, 5, 4, 1, 0],    # 0.95 x 10 = 9.5 -> the 10th delivery
        [0, 19, 0, 0, 1],   # 0.95 x 20 = 19, reached exactly at age 1
    ], dtype=np.int64)
    got = latency_quantiles(rows, qs)
    assert got.dtype == np.int64 and got.shape == (5, 3)
    assert got.tolist() == [[-1, -1, -1], [2, 2, 2], [1, 2, 2], [1, 3, 3], [1, 1, 4]]
    assert latency_quantiles(rows[3], qs).tolist() == [1, 3, 3]           # one row
    assert latency_quantiles(rows.astype(np.uint32), (0.5,)).tolist() == [[-1], [2], [1], [1], [1]]
    # counts past 2^53: q x total stays exact
    big = np.array([0, (1 << 60) + 1, (1 << 60) - 1], dtype=np.int64)
    assert latency_quantiles(big, (0.5,)).tolist() == [1]
    big = np.array([0, (1 << 60) - 1, (1 << 60) + 1], dtype=np.int64)
    assert latency_quantiles(big, (0.5,)).tolist() == [2]


@pytest.mark.parametrize("name", sorted(latency_ref.TABLE))
def test_reference_preconditions(oracle_path, name):
    nodes, topics, deliveries, max_age = latency_ref.TABLE[name]
    r = latency_ref.ref(oracle_path, name)
    assert (r.N, r.T) == (nodes, topics)
    assert r.max_age == max_age
    assert int((r.age == 0).sum()) == 0  # no delivery within the publish hop
    h = r.hist(max_age + 1)
    assert h.sum() == r.counters["deliveries"] == deliveries
    assert h[:, 0].sum() == 0 and h[:, max_age].sum() > 0
    rows = r.message_rows(range(len(r.msg_hop)), max_age + 1)
    assert rows.sum() == deliveries
    for t in range(topics):
        assert np.array_equal(rows[r.msg_topic == t].sum(axis=0), h[t])
    # a partition's tables add up to the whole graph's
    cut = nodes // 3
    assert np.array_equal(r.hist(max_age + 1, (0, cut)) + r.hist(max_age + 1, (cut, nodes)), h)


@pytest.mark.parametrize("name", latency_ref.WINDOWS)
def test_window_families_reuse_slot_zero(oracle_path, name):
    """The GPU tests read id 0 as refused (its slot has a new owner) and the
    last bin as reached: both must hold on the schedule."""
    from test_window import family_window
    r = latency_ref.ref(oracle_path, name)
    assert r.max_age == family_window(name)[0]
    assert 0 not in r.live_ids and len(r.live_ids) < len(r.msg_hop)
