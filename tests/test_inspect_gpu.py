"""WithPeerScoreInspect on the device (include/gs_inspect.h) against the oracle
stepped in pieces (tests/inspect_ref.py).  Every comparison is exact.  Each
scenario runs once on the GPU, as one single step(hops) with the observers of
inspect_ref.observers_of sampled and the extended fields kept, and every test
reads that run.  tests/test_inspect.py holds the scenarios' preconditions."""
import ctypes as C
import functools
import multiprocessing as mp
import os
import sys

import numpy as np
import pytest

import inspect_ref
import scenarios
from pubsub_amd import PRODUCT_LIB, GossipEngineError, PeerScoreSnapshot, WithPeerScoreInspect, _abi
from test_partition_gpu import _free_port

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
HOP = scenarios.HOP
ROW_CASES = ["gossipsub_scored", "gossipsub_multitopic", "gossipsub_negative_app", "adversarial_mix", "churn_scored",
             "p6_churn_heavy", "mixed_scored", "ladder_64t", "ladder32_64t", "ladder_wide_mesh_4t",
             "ladder_wide_mesh_64t"]
SAMPLED = ["ladder_64t", "adversarial_mix", "churn_scored"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def option(r, inspect=None, ticks=None, extended=True, nodes=True):
    return WithPeerScoreInspect(inspect, r.period * HOP, bounds=r.bounds, nodes=r.observers if nodes else None,
                                ticks=max(64, r.ticks) if ticks is None else ticks, extended=extended)


class Got:
    """One run on the GPU with inspection on, every tick read back."""

    def __init__(self, oracle, name):
        r = inspect_ref.ref(oracle, name)
        e, hops = inspect_ref.builder(name)(PRODUCT_LIB, (option(r),))
        assert hops == r.hops
        assert e.inspect_ticks() == 0
        e.step(hops)
        self.ticks = e.inspect_ticks()
        self.edges = e.inspect_edges()
        self.rows = [e.inspect_row(k) for k in range(self.ticks)]
        self.scores = [e.inspect_scores(k) for k in range(self.ticks)]
        self.snaps = [e.inspect_snapshot(k) for k in range(self.ticks)]
        self.final_scores, self.final_mesh = e.scores(), e.mesh()
        e.close()


@functools.lru_cache(maxsize=None)
def got(oracle, name):
    return Got(oracle, name)


@pytest.mark.parametrize("name", ROW_CASES)
def test_rows_equal_oracle(oracle_path, name):
    r, g = inspect_ref.ref(oracle_path, name), got(oracle_path, name)
    assert g.ticks == r.ticks > 0
    bad = []
    for k in range(r.ticks):
        row = g.rows[k]
        assert row["hop"] == r.hop(k)
        assert row["score_hist"].dtype == np.int64 and row["score_hist"].shape == (len(r.bounds) + 1,)
        assert row["mesh_deg"].dtype == np.int64 and row["mesh_deg"].shape == (r.T, 65)
        assert row["score_hist"].sum() == r.E and (row["mesh_deg"].sum(axis=1) == r.N).all()
        if not np.array_equal(row["score_hist"], r.score_hist(k)):
            bad.append(f"tick {k}: score_hist {row['score_hist'].tolist()} != {r.score_hist(k).tolist()}")
        want = r.mesh_deg(k)
        if not np.array_equal(row["mesh_deg"], want):
            bad.append(f"tick {k}: mesh_deg differs at (t, d) {np.argwhere(row['mesh_deg'] != want)[:5].tolist()}")
    assert bad == [], "\n".join(bad[:10])
    # the run itself ends where the oracle's does
    assert np.array_equal(_bits(g.final_scores), _bits(r.final_scores)) and np.array_equal(g.final_mesh, r.final_mesh)


@pytest.mark.parametrize("T", [4, 64])
def test_wide_mesh_rows_equal_own_readbacks(oracle_path, T):
    """The ticks against the engine's own gs_read_scores / gs_read_mesh of a
    second engine without inspection, stepped 3 hops at a time: tells an
    inspection error from a disagreement of the existing kernels with the
    oracle under these unusual mesh parameters."""
    name = f"ladder_wide_mesh_{T}t"
    r, g = inspect_ref.ref(oracle_path, name), got(oracle_path, name)
    e, _ = inspect_ref.builder(name)(PRODUCT_LIB)
    differs = 0
    for k in range(r.ticks):
        e.step(r.period)
        s, m = e.scores(), e.mesh()
        assert np.array_equal(g.rows[k]["score_hist"], inspect_ref.score_hist(r.bounds, s)), f"tick {k}"
        assert np.array_equal(g.rows[k]["mesh_deg"], inspect_ref.mesh_deg(r.rowptr, m, T)), f"tick {k}"
        assert np.array_equal(_bits(g.scores[k]), _bits(s[g.edges])), f"tick {k}"
        differs += int(not (np.array_equal(_bits(s), _bits(r.scores[k])) and np.array_equal(m, r.mesh[k])))
    e.close()
    print(f"{name}: ticks at which the engine without inspection differs from the oracle: {differs} of {r.ticks}")
    assert max(int(row["mesh_deg"][:, 64].sum()) for row in g.rows) > 0


@pytest.mark.parametrize("name", SAMPLED)
def test_sampled_scores_and_snapshots(oracle_path, name):
    r, g = inspect_ref.ref(oracle_path, name), got(oracle_path, name)
    assert np.array_equal(g.edges, r.edges) and len(r.edges) > 64
    app_want = r.app[r.col[r.edges]]
    for k in range(r.ticks):
        st, sn = r.stats[k], g.snaps[k]
        assert np.array_equal(_bits(g.scores[k]), _bits(r.scores[k][r.edges])), f"tick {k}: scores"
        in_mesh = (st["flags"] & 1) != 0
        assert np.array_equal(sn["time_in_mesh"], np.where(in_mesh, st["mesh_time"], 0)), f"tick {k}: time_in_mesh"
        assert not sn["time_in_mesh"][~in_mesh].any()
        for f in ("fmd", "mmd", "imd"):
            assert np.array_equal(_bits(sn[f]), _bits(st[f])), f"tick {k}: {f}"
        assert np.array_equal(_bits(sn["behaviour_penalty"]), _bits(r.bp[k])), f"tick {k}: behaviour penalty"
        if name == "churn_scored":
            # an edge without a record reads 0 (the reference's map has no entry for it); every
            # edge the oracle holds anything for has one
            live = (st["fmd"] != 0).any(axis=1) | (st["mesh_time"] != 0).any(axis=1) | (r.bp[k] != 0) | \
                (r.scores[k][r.edges] != 0)
            assert np.array_equal(sn["app"][live], app_want[live]), f"tick {k}: app"
            assert ((sn["app"] == app_want) | (sn["app"] == 0)).all()
        else:
            assert np.array_equal(sn["app"], app_want), f"tick {k}: app"
    assert any(sn["time_in_mesh"].any() for sn in g.snaps) and any(sn["fmd"].any() for sn in g.snaps)


def test_ip_colocation_factor(oracle_path):
    """p6_static_dense: the surplus of the observer's peers on the peer's IP
    over the threshold, squared (score.go:335-379), recounted with numpy."""
    r, g = inspect_ref.ref(oracle_path, "p6_static_dense"), got(oracle_path, "p6_static_dense")
    thr = r.score_params.IPColocationFactorThreshold
    obs = np.searchsorted(r.rowptr, r.edges, side="right") - 1
    want = np.zeros(len(r.edges))
    for i, (u, e) in enumerate(zip(obs, r.edges)):
        peers = r.col[r.rowptr[u]:r.rowptr[u + 1]]
        surplus = int((r.ipv4[peers] == r.ipv4[r.col[e]]).sum()) - thr
        want[i] = float(surplus * surplus) if surplus > 0 else 0.0
    assert want.max() > 0 and (want == 0).any()
    for k in range(r.ticks):
        assert np.array_equal(g.snaps[k]["ip_colocation"], want), f"tick {k}"
        assert np.array_equal(_bits(g.scores[k]), _bits(r.scores[k][r.edges])), f"tick {k}"


@pytest.mark.parametrize("name", SAMPLED + ["p6_static_dense"])
def test_score_recomputed_from_snapshot_parts(oracle_path, name):
    """score() (score.go:256-333) from the snapshot's own parts, with the two
    inputs a PeerScoreSnapshot does not carry (MeshFailurePenalty and the
    in-mesh / P3-active flags) from the reference, gives the snapshot's Score."""
    r, g = inspect_ref.ref(oracle_path, name), got(oracle_path, name)
    for k in (0, r.ticks // 2, r.ticks - 1):
        st, sn = r.stats[k], g.snaps[k]
        calc = np.array([inspect_ref.score_from_parts(
            r.score_params, r.T, sn["time_in_mesh"][i], sn["fmd"][i], sn["mmd"][i], sn["imd"][i], st["mfp"][i],
            st["flags"][i], sn["app"][i], sn["ip_colocation"][i], sn["behaviour_penalty"][i])
            for i in range(len(r.edges))])
        assert np.array_equal(calc, g.scores[k]), f"tick {k}: first at {np.flatnonzero(calc != g.scores[k])[:5]}"


def test_ring_and_callback(oracle_path):
    name = "gossipsub_negative_app"
    r, g = inspect_ref.ref(oracle_path, name), got(oracle_path, name)
    assert r.ticks == 12
    e, hops = inspect_ref.builder(name)(PRODUCT_LIB, (option(r, ticks=4, extended=False),))
    e.set_profiling(True)
    e.step(hops)
    assert e.inspect_ticks() == 12
    for k in range(8, 12):
        row = e.inspect_row(k)
        assert row["hop"] == r.hop(k)
        assert np.array_equal(row["score_hist"], r.score_hist(k)) and np.array_equal(row["mesh_deg"], r.mesh_deg(k))
        assert np.array_equal(_bits(e.inspect_scores(k)), _bits(r.scores[k][r.edges]))
    for k, code in [(j, _abi.GS_ESTATE) for j in range(8)] + [(12, _abi.GS_EINVAL), (-1, _abi.GS_EINVAL)]:
        for call in (e.inspect_row, e.inspect_scores):
            with pytest.raises(GossipEngineError) as ei:
                call(k)
            assert ei.value.code == code, (k, str(ei.value))
    with pytest.raises(GossipEngineError) as ei:  # extended = 0: no snapshot fields
        e.inspect_snapshot(11)
    assert ei.value.code == _abi.GS_ESTATE
    ks = e.inspect_kernel_stats()
    assert [ks[n][1] for n in _abi.INSPECT_KERNEL_NAMES] == [12, 12, 12] and all(v[0] > 0 for v in ks.values())
    e.close()

    # the callback form with the same small ring still delivers every tick, in order
    for extended in (False, True):
        seen = []
        holder = {}

        def inspect(hop, scores):
            seen.append((hop, scores, holder["e"].inspect_row(hop // r.period - 1)))

        e, hops = inspect_ref.builder(name)(PRODUCT_LIB, (option(r, inspect=inspect, ticks=4, extended=extended),))
        holder["e"] = e
        e.step(hops)
        e.close()
        assert [h for h, _, _ in seen] == [r.hop(k) for k in range(12)]
        with_edges = [u for u in r.observers if r.rowptr[u + 1] > r.rowptr[u]]
        for k, (hop, scores, row) in enumerate(seen):
            assert row["hop"] == hop
            assert np.array_equal(row["score_hist"], g.rows[k]["score_hist"])
            assert np.array_equal(row["mesh_deg"], g.rows[k]["mesh_deg"])
            assert sorted(scores) == r.observers and all(scores[u] for u in with_edges)
            for u in with_edges:
                for e_ in range(int(r.rowptr[u]), int(r.rowptr[u + 1])):
                    val = scores[u][int(r.col[e_])]
                    want = r.scores[k][e_]
                    if not extended:
                        assert isinstance(val, float) and _bits(val) == _bits(want)
                        continue
                    i = int(np.searchsorted(r.edges, e_))
                    assert isinstance(val, PeerScoreSnapshot) and _bits(val.Score) == _bits(want)
                    assert val.AppSpecificScore == r.app[r.col[e_]] and val.BehaviourPenalty == r.bp[k][i]
                    assert sorted(val.Topics) == list(range(r.T))
                    for t, ts in val.Topics.items():
                        st = r.stats[k]
                        assert ts.FirstMessageDeliveries == st["fmd"][i, t]
                        assert ts.MeshMessageDeliveries == st["mmd"][i, t]
                        assert ts.InvalidMessageDeliveries == st["imd"][i, t]
                        assert ts.TimeInMesh == (st["mesh_time"][i, t] if st["flags"][i, t] & 1 else 0)


@pytest.mark.parametrize("name", ["gossipsub_scored", "adversarial_mix", "ladder_64t"])
def test_nothing_else_moves(oracle_path, name):
    r = inspect_ref.ref(oracle_path, name)
    snaps = []
    for extra in ((), (option(r),)):
        e, hops = scenarios.SCENARIOS[name](PRODUCT_LIB, extra)
        e.step(hops)
        snaps.append(scenarios.snapshot(e, getattr(e, "snapshot_ids", range(e.n_published))))
        e.close()
    bad = scenarios.compare(*snaps)
    assert bad == [], "\n".join(bad)


def _raw(period=1, ticks=1, bounds=(), mask=None, extended=0):
    b = np.array(bounds, dtype=np.float64)
    cfg = _abi.InspectConfigC(period, ticks, len(b), b.ctypes.data_as(C.POINTER(C.c_double)),
                              mask.ctypes.data_as(C.POINTER(C.c_uint8)) if mask is not None else None, extended)
    cfg._keep = b
    return cfg


def _err(e):
    return e.lib.gs_last_error().decode()


def test_refusals():
    opt = WithPeerScoreInspect(None, HOP)
    for name, text in (("floodsub_dense", "pubsub router is not gossipsub"),
                       ("randomsub_100", "pubsub router is not gossipsub"),
                       ("gossipsub_dense", "peer scoring is not enabled")):
        with pytest.raises(GossipEngineError) as ei:
            scenarios.SCENARIOS[name](PRODUCT_LIB, (opt,))
        assert ei.value.code == _abi.GS_EUNSUPPORTED and text in str(ei.value)
    # a second call
    e, _ = scenarios.SCENARIOS["gossipsub_multitopic"](PRODUCT_LIB, (opt,))
    assert e.lib.gs_set_score_inspect(e.h, C.byref(_raw())) == _abi.GS_ESTATE
    assert _err(e) == "duplicate peer score inspector"
    e.close()
    # bad arguments, each with a text of its own; nothing is set by a refused call
    e, _ = scenarios.SCENARIOS["gossipsub_multitopic"](PRODUCT_LIB)
    texts = set()
    for cfg in (_raw(period=0), _raw(period=-3), _raw(ticks=0), _raw(bounds=list(range(64))),
                _raw(bounds=[0.0, 0.0]), _raw(bounds=[1.0, 0.0]), _raw(bounds=[float("nan")]),
                _raw(bounds=[0.0, float("inf")])):
        assert e.lib.gs_set_score_inspect(e.h, C.byref(cfg)) == _abi.GS_EINVAL
        texts.add(_err(e))
    assert len(texts) == 4
    assert e.lib.gs_set_score_inspect(e.h, None) == _abi.GS_EINVAL
    # inspection off: every read is refused, before and after the start
    for _ in range(2):
        for call in (e.inspect_ticks, e.inspect_edges, e.inspect_kernel_stats, lambda: e.inspect_row(0),
                     lambda: e.inspect_scores(0), lambda: e.inspect_snapshot(0)):
            with pytest.raises(GossipEngineError) as ei:
                call()
            assert ei.value.code == _abi.GS_ESTATE
        e.step(1)
    # after the first step
    assert e.lib.gs_set_score_inspect(e.h, C.byref(_raw())) == _abi.GS_ESTATE
    assert "before the first step" in _err(e)
    e.close()
    # 63 bounds, no sampled nodes: valid
    e, _ = scenarios.SCENARIOS["gossipsub_multitopic"](
        PRODUCT_LIB, (WithPeerScoreInspect(None, 2 * HOP, bounds=np.arange(63) - 31.0),))
    e.step(4)
    assert e.inspect_ticks() == 2 and len(e.inspect_edges()) == 0 and len(e.inspect_scores(1)) == 0
    row = e.inspect_row(1)
    assert row["hop"] == 4 == e.hop and row["score_hist"].shape == (64,) and row["score_hist"].sum() == e.E
    assert np.array_equal(row["score_hist"], inspect_ref.score_hist(np.arange(63) - 31.0, e.scores()))
    e.close()


# ---------------------------------------------------------------- partitioned
def _worker(rank, world, port, name, oracle, q):
    try:
        sys.path.insert(0, HERE)
        sys.path.insert(0, os.path.join(os.path.dirname(HERE), "go-libp2p-pubsub_amd"))
        import torch
        import torch.distributed as dist

        import inspect_ref
        from pubsub_amd import PRODUCT_LIB, WithPartition
        from pubsub_amd.transport import TorchTransport
        from test_inspect_gpu import _bits, option
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
        tr = TorchTransport(memory="device")
        r = inspect_ref.ref(oracle, name)
        e, hops = inspect_ref.builder(name)(PRODUCT_LIB, (WithPartition(rank, world, tr), option(r)))
        e.step(hops)
        own = e.node_range
        bad = []
        if e.inspect_ticks() != r.ticks:
            bad.append(f"rank {rank}: {e.inspect_ticks()} ticks, not {r.ticks}")
        edges = e.inspect_edges()
        if not np.array_equal(edges, inspect_ref.edges_of(r.rowptr, r.observers, own)):
            bad.append(f"rank {rank} {own}: sampled edges are not its own observers' edges")
        at = np.searchsorted(r.edges, edges)
        for k in range(r.ticks):
            row = e.inspect_row(k)
            if row["hop"] != r.hop(k) or not np.array_equal(row["score_hist"], r.score_hist(k, own)):
                bad.append(f"rank {rank} {own} tick {k}: score_hist differs")
            if not np.array_equal(row["mesh_deg"], r.mesh_deg(k, own)):
                bad.append(f"rank {rank} {own} tick {k}: mesh_deg differs")
            if not np.array_equal(_bits(e.inspect_scores(k)), _bits(r.scores[k][edges])):
                bad.append(f"rank {rank} {own} tick {k}: sampled scores differ")
            sn = e.inspect_snapshot(k)
            if not np.array_equal(_bits(sn["fmd"]), _bits(r.stats[k]["fmd"][at])):
                bad.append(f"rank {rank} {own} tick {k}: sampled fmd differs")
            total = torch.from_numpy(np.concatenate([row["score_hist"], row["mesh_deg"].ravel()]))
            dist.all_reduce(total)
            if not np.array_equal(total.numpy(), np.concatenate([r.score_hist(k), r.mesh_deg(k).ravel()])):
                bad.append(f"tick {k}: the ranks' rows do not add up to the whole graph's")
        q.put((rank, bad[:8], own, len(edges)))
        e.close()
        dist.destroy_process_group()
    except Exception as ex:  # report instead of hanging the parent
        import traceback
        q.put((rank, [f"worker raised: {ex!r}\n{traceback.format_exc()}"], None, 0))


@pytest.mark.parametrize("world,name", [(2, "gossipsub_multitopic"), (2, "adversarial_mix"), (3, "ladder_64t")])
def test_partitioned_rank_counts_its_own(oracle_path, world, name):
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
    for rank, bad, own, n in res:
        assert bad == [], "\n".join(bad)
    r = inspect_ref.ref(oracle_path, name)
    assert res[0][2][0] == 0 and res[-1][2][1] == r.N
    assert sum(x[3] for x in res) == len(r.edges)  # every sampled edge on its owner rank only
