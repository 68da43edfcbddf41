"""The latency statistics and the four periodic inspectors (score inspection,
mesh health, mesh reach, bandwidth statistics) on one engine, against engines
that each carry one of them alone.  acct_multitopic, a tick of every inspector
at every hop into rings of 4, 12 hops with profiling on; every comparison is
exact.  Each engine runs once and every test reads that run."""
import functools

import numpy as np
import pytest

import scenarios
from pubsub_amd import (PRODUCT_LIB, GossipEngineError, WithBandwidthStats, WithLatencyStats, WithMeshHealth,
                        WithMeshReach, WithPeerScoreInspect, WithPeertxCapacity, _abi)

pytestmark = pytest.mark.gpu
HOP = scenarios.HOP
NAME, HOPS, TICKS = "acct_multitopic", 12, 4
OBSERVERS, SOURCES = [3, 60, 199], [150, 7]
KEPT = range(HOPS - TICKS, HOPS)  # the ticks still in the rings
OPTIONS = {
    "latency": lambda: WithLatencyStats(),
    "inspect": lambda: WithPeerScoreInspect(None, HOP, nodes=OBSERVERS, ticks=TICKS, extended=True),
    "mesh_health": lambda: WithMeshHealth(HOP, ticks=TICKS, labels=True),
    "mesh_reach": lambda: WithMeshReach(HOP, SOURCES, ticks=TICKS, depths=True),
    "bandwidth": lambda: WithBandwidthStats(HOP, nodes=OBSERVERS, ticks=TICKS),
}
ROW_READS = {"inspect": ("inspect_row", "inspect_scores", "inspect_snapshot"), "mesh_health": ("mesh_health_row",),
             "mesh_reach": ("mesh_reach_row",), "bandwidth": ("bandwidth_row", "bandwidth_sampled")}
NEWEST_READS = {"latency": ("latency_hist",), "inspect": ("inspect_edges",), "mesh_health": ("mesh_labels",),
                "mesh_reach": ("mesh_reach_depths",), "bandwidth": ("bandwidth_nodes",)}


def _flat(prefix, v, out):
    """Every array or number under `v` (dicts and tuples walked), by name."""
    if isinstance(v, dict):
        for k in v:
            _flat(f"{prefix}.{k}", v[k], out)
    elif isinstance(v, tuple):
        for i, x in enumerate(v):
            _flat(f"{prefix}[{i}]", x, out)
    else:
        out[prefix] = np.asarray(v)


def read(e, features):
    """{feature: {name: array}}: the kept ticks and the newest-tick tables."""
    got = {}
    for f in features:
        out = {}
        assert f == "latency" or getattr(e, f + "_ticks")() == HOPS
        for call in ROW_READS.get(f, ()):
            for k in KEPT:
                _flat(f"{call}({k})", getattr(e, call)(k), out)
        for call in NEWEST_READS[f]:
            _flat(call, getattr(e, call)(), out)
        got[f] = out
    return got


MESH_BATCH = 4  # GS_MESH_BATCH (csrc/gs_kernels_mesh.h): label launches per read of the flags
TIMING = ("mesh_label", "iterations", "bytes")  # of mesh health: see same_launches


def launches(e, f):
    """The launch counts of feature f's kernels and the counters kept with them."""
    return {k: v[1] if isinstance(v, tuple) else v for k, v in getattr(e, f + "_kernel_stats")().items()}


def same_launches(f, got, want):
    """Equal counts.  Mesh health's label launches, iterations and bytes alone
    may differ between two runs of one engine: how far a label iteration gets
    depends on the order of its workgroups, by at most one iteration a tick
    (DESIGN.md §6o), so by at most one batch of launches a tick; the launches
    come in whole batches, at least one a tick."""
    if f != "mesh_health":
        return got == want
    for ks in (got, want):
        assert ks["mesh_label"] % MESH_BATCH == 0 and ks["mesh_label"] >= MESH_BATCH * HOPS, ks
        assert ks["mesh_label"] >= ks["iterations"] >= HOPS and ks["bytes"] > 0, ks
    return ({k: v for k, v in got.items() if k not in TIMING} == {k: v for k, v in want.items() if k not in TIMING}
            and abs(got["iterations"] - want["iterations"]) <= HOPS
            and abs(got["mesh_label"] - want["mesh_label"]) <= MESH_BATCH * HOPS)


class Ran:
    def __init__(self, features, extra=()):
        e, _ = scenarios.SCENARIOS[NAME](PRODUCT_LIB, tuple(OPTIONS[f]() for f in features) + tuple(extra))
        self.e, self.features = e, features

    def step(self):
        e = self.e
        e.set_profiling(True)
        e.step(HOPS)
        self.got = read(e, self.features)
        self.launches = {f: launches(e, f) for f in self.features}
        self.public = {k: v[1] for k, v in e.kernel_stats().items()}
        self.final = scenarios.snapshot(e, range(e.n_published))
        return self


@functools.lru_cache(maxsize=None)
def ran(*features):
    r = Ran(features).step()
    r.e.close()
    return r


def differences(got, want, f):
    assert got.keys() == want.keys() and len(got) > 0
    return [f"{f}: {k} differs" for k in want if not np.array_equal(scenarios._bits(got[k]), scenarios._bits(want[k]))]


def test_all_five_equal_each_alone():
    both = ran(*OPTIONS)
    bad = []
    for f in OPTIONS:
        bad += differences(both.got[f], ran(f).got[f], f)
    assert bad == [], "\n".join(bad[:10])
    # something was there to compare: hosts in the mesh, sources that reach, bytes sent, deliveries
    assert both.got["mesh_health"][f"mesh_health_row({HOPS - 1}).members"].sum() > 0
    assert both.got["mesh_reach"][f"mesh_reach_row({HOPS - 1}).reached"].sum() > 0
    assert both.got["bandwidth"][f"bandwidth_row({HOPS - 1}).total"][0] > 0
    assert both.got["latency"]["latency_hist"].sum() > 0 and len(both.got["inspect"]["inspect_edges"]) > 0
    for f in ROW_READS:
        assert both.got[f][f"{ROW_READS[f][0]}({HOPS - 1}).hop"] == HOPS


def test_nothing_else_moves():
    bad = scenarios.compare(ran().final, ran(*OPTIONS).final)
    assert bad == [], "\n".join(bad)


def test_kernel_stat_ranges_do_not_overlap():
    """A feature's launch counts on the engine with all five are its counts
    alone; the public kernels' are the plain run's."""
    both = ran(*OPTIONS)
    for f in OPTIONS:
        assert same_launches(f, both.launches[f], ran(f).launches[f]), (f, both.launches[f], ran(f).launches[f])
        assert sum(both.launches[f].values()) > 0, f
    assert both.public == ran().public and sum(both.public.values()) > 0
    assert [both.launches["inspect"][k] for k in _abi.INSPECT_KERNEL_NAMES] == [HOPS] * 3
    assert [both.launches["bandwidth"][k] for k in _abi.BANDWIDTH_KERNEL_NAMES] == [HOPS] * 3
    assert both.launches["mesh_health"]["mesh_init"] == both.launches["mesh_reach"]["reach_members"] == HOPS
    assert both.launches["mesh_reach"]["passes"] == HOPS


def test_ring_window_of_every_inspector():
    """Tick k reads while taken - ticks <= k < taken, with one pair of codes."""
    e, _ = scenarios.SCENARIOS[NAME](PRODUCT_LIB, tuple(OPTIONS[f]() for f in ROW_READS))
    e.step(HOPS)
    for f, calls in ROW_READS.items():
        for call in calls:
            for k, code in [(HOPS - TICKS - 1, _abi.GS_ESTATE), (0, _abi.GS_ESTATE), (HOPS, _abi.GS_EINVAL),
                            (-1, _abi.GS_EINVAL)]:
                with pytest.raises(GossipEngineError) as ei:
                    getattr(e, call)(k)
                assert ei.value.code == code, (call, k, str(ei.value))
            getattr(e, call)(HOPS - TICKS)
    e.close()


def test_restart_after_a_refused_start():
    """A first step refused while the device state is built (a peertx row the
    LDS cannot hold): the same engine, corrected, starts and ticks as the engine
    that started at once.  The refusal comes before the observers' own tables
    are allocated (no later refusal is made on the host), so release() gives
    back the core state only: the observers' configuration surviving it and
    their start after it are what this pins, not the reset of their `dev`
    records."""
    r = Ran(tuple(OPTIONS), (WithPeertxCapacity(16, 16),))
    e = r.e
    for _ in range(2):
        with pytest.raises(GossipEngineError) as ei:
            e.step(1)
        assert ei.value.code == _abi.GS_ECAPACITY and "lower home_bits" in str(ei.value)
        assert e.hop == 0 and [getattr(e, f + "_ticks")() for f in ROW_READS] == [0] * 4
    assert e.lib.gs_set_peertx_capacity(e.h, 10, 16) == _abi.GS_OK  # the default row
    r.step()
    e.close()
    want = ran(*OPTIONS)
    bad = scenarios.compare(want.final, r.final)
    for f in OPTIONS:
        bad += differences(r.got[f], want.got[f], f)
        assert same_launches(f, r.launches[f], want.launches[f]), (f, r.launches[f], want.launches[f])
    assert bad == [], "\n".join(bad[:10])
