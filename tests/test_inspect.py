"""WithPeerScoreInspect (include/gs_inspect.h) without a GPU: the Python
option's own checks, the ABI struct's layout, and the preconditions of
tests/test_inspect_gpu.py on the oracle alone (tests/inspect_ref.py), so that a
pass on the GPU cannot be vacuous."""
import ctypes as C

import numpy as np
import pytest

import inspect_ref
import scenarios
from pubsub_amd import (Millisecond, PeerScoreSnapshot, TopicScoreSnapshot, WithPeerScoreInspect, _abi,
                        default_inspect_bounds, eth2_thresholds)


# ---------------------------------------------------------------- (a) pure Python
def test_period_must_be_a_multiple_of_the_hop(oracle_path):
    for period in (150 * Millisecond, 0, -100 * Millisecond, 1):
        with pytest.raises(ValueError, match="multiple of the hop"):
            scenarios.SCENARIOS["gossipsub_dense"](oracle_path, (WithPeerScoreInspect(None, period),))
    # a valid period gets as far as the library: the oracle does not export gs_inspect.h
    with pytest.raises(ValueError, match="product library only"):
        scenarios.SCENARIOS["gossipsub_dense"](oracle_path, (WithPeerScoreInspect(None, 300 * Millisecond),))


@pytest.mark.parametrize("bounds", [[0.0, -1.0], [1.0, 1.0], [0.0, float("inf")], [float("nan")],
                                    list(range(64))])
def test_bad_bounds_are_refused(bounds):
    with pytest.raises(ValueError):
        WithPeerScoreInspect(None, 100 * Millisecond, bounds=bounds)


def test_option_arguments():
    with pytest.raises(ValueError):
        WithPeerScoreInspect(None, 100 * Millisecond, ticks=0)
    with pytest.raises(ValueError):
        WithPeerScoreInspect("not callable", 100 * Millisecond)
    key, val = WithPeerScoreInspect(None, 100 * Millisecond, bounds=list(range(63)), nodes=[1, 2], extended=True)
    assert key == "score_inspect" and val["ticks"] == 64 and val["extended"] and len(val["bounds"]) == 63


def test_default_bounds():
    assert default_inspect_bounds(eth2_thresholds()) == [-300.0, -200.0, -100.0, 0.0, 5e-324, 1.0]
    b = np.array(default_inspect_bounds(eth2_thresholds()))
    # "exactly 0" has a bin of its own
    assert np.searchsorted(b, [-0.0, 0.0, 5e-324, -5e-324], side="right").tolist() == [4, 4, 5, 3]


def test_abi_struct_layout():
    S = _abi.InspectConfigC
    assert C.sizeof(S) == 40
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [
        ("period_hops", 0), ("ticks", 8), ("num_bounds", 12), ("bounds", 16), ("node_mask", 24), ("extended", 32)]
    assert _abi.GS_INSPECT_MAX_BOUNDS == 63 and _abi.GS_INSPECT_DEG_BINS == 65
    assert [n for n, _, _ in _abi.INSPECT_FUNCTIONS] == [
        "gs_set_score_inspect", "gs_inspect_ticks", "gs_inspect_num_edges", "gs_inspect_edges",
        "gs_read_inspect_row", "gs_read_inspect_scores", "gs_read_inspect_snapshot",
        "gs_read_inspect_kernel_stats"]


def test_snapshot_dataclasses():
    s = PeerScoreSnapshot(Score=1.5, Topics={0: TopicScoreSnapshot(TimeInMesh=3)})
    assert (s.AppSpecificScore, s.IPColocationFactor, s.BehaviourPenalty) == (0.0, 0.0, 0.0)
    t = s.Topics[0]
    assert (t.TimeInMesh, t.FirstMessageDeliveries, t.MeshMessageDeliveries, t.InvalidMessageDeliveries) == (3, 0, 0, 0)


# ---------------------------------------------------------------- (b) the oracle alone
def test_ref_binning():
    b = np.array([-1.0, 0.0, 2.0])
    assert inspect_ref.score_hist(b, np.array([-5.0, -1.0, -0.5, 0.0, 0.0, 1.0, 2.0, 9.0])).tolist() == [1, 2, 3, 2]
    rowptr = np.array([0, 2, 3, 3])
    mesh = np.array([1, 3, 2], dtype=np.uint64)
    d = inspect_ref.mesh_deg(rowptr, mesh, 2)
    assert d[0, :3].tolist() == [2, 0, 1] and d[1, :3].tolist() == [1, 2, 0] and d.sum(axis=1).tolist() == [3, 3]


@pytest.mark.parametrize("name", ["gossipsub_negative_app", "adversarial_mix", "churn_scored", "ladder_64t",
                                  "p6_churn_heavy"])
def test_stepping_in_pieces_changes_nothing(oracle_path, name):
    """Reads between pieces leave the oracle's state alone: scores and meshes
    after the pieces equal those of one whole step, on the bit patterns."""
    r = inspect_ref.ref(oracle_path, name)
    e, hops = inspect_ref.builder(name)(oracle_path)
    e.step(hops)
    assert np.array_equal(e.scores().view(np.uint64), r.final_scores.view(np.uint64))
    assert np.array_equal(e.mesh(), r.final_mesh)
    e.close()


def test_adversarial_mix_fills_every_bin(oracle_path):
    r = inspect_ref.ref(oracle_path, "adversarial_mix")
    assert r.period == 10 and r.E == 6400 and len(r.bounds) == 6
    rows = np.stack([r.score_hist(k) for k in range(r.ticks)])
    assert (rows.sum(axis=1) == r.E).all()
    assert (rows.max(axis=0) > 0).all(), rows.max(axis=0)
    h = rows[5]
    assert np.cumsum(h)[:4].tolist() == [293, 453, 455, 748] and h[4] == 2236


def test_p6_churn_heavy_graylists(oracle_path):
    r = inspect_ref.ref(oracle_path, "p6_churn_heavy")
    assert max(r.score_hist(k)[0] for k in range(r.ticks)) > 200


def test_negative_app_scores_on_the_bounds(oracle_path):
    r = inspect_ref.ref(oracle_path, "gossipsub_negative_app")
    assert r.bounds.tolist() == [-300.0, -150.0, 0.0, 1.0]
    on150 = sum(int((s == -150.0).sum()) for s in r.scores)
    on0 = sum(int((s == 0.0).sum()) for s in r.scores)
    assert on150 > 0 and on0 > 0
    # on-the-bound scores go to the upper bin
    k = next(k for k in range(r.ticks) if (r.scores[k] == -150.0).any())
    assert r.score_hist(k)[2] >= (r.scores[k] == -150.0).sum()


def test_churn_scored_has_edges_without_records(oracle_path):
    r = inspect_ref.ref(oracle_path, "churn_scored")
    # a sampled edge whose every field is zero at some tick and not at another
    seen = np.zeros(len(r.edges), dtype=bool)
    blank = np.zeros(len(r.edges), dtype=bool)
    for k in range(r.ticks):
        live = (r.stats[k]["fmd"] != 0).any(axis=1) | (r.stats[k]["mesh_time"] != 0).any(axis=1)
        seen |= live
        blank |= ~live & (r.scores[k][r.edges] == 0)
    assert (seen & blank).any()


def test_mixed_scored_has_hosts_without_scores(oracle_path):
    r = inspect_ref.ref(oracle_path, "mixed_scored")
    e, _ = inspect_ref.builder("mixed_scored")(oracle_path)
    other = np.flatnonzero(e.routers < _abi.GS_ROUTER_GOSSIPSUB)
    e.close()
    assert len(other) > 10
    for u in other:
        sl = slice(int(r.rowptr[u]), int(r.rowptr[u + 1]))
        assert not r.scores[-1][sl].any() and not r.mesh[-1][sl].any()


def test_ladder_64t_degrees(oracle_path):
    r = inspect_ref.ref(oracle_path, "ladder_64t")
    d = r.mesh_deg(r.ticks - 1)
    assert (d.sum(axis=1) == r.N).all()
    assert d[:, 0].min() > 0 and d[:, 12].sum() > 0
    assert set(np.diff(r.rowptr)[r.observers]) >= {64, 1, 0}


@pytest.mark.parametrize("T,at64,over32", [(4, 8, 32), (64, 120, 512)])
def test_ladder_wide_mesh_reaches_the_last_bin(oracle_path, T, at64, over32):
    r = inspect_ref.ref(oracle_path, f"ladder_wide_mesh_{T}t")
    assert r.T == T and r.period == 3
    best64 = max(int(r.mesh_deg(k)[:, 64].sum()) for k in range(r.ticks))
    best33 = max(int(r.mesh_deg(k)[:, 33:].sum()) for k in range(r.ticks))
    assert best64 > 0 and best33 >= 32
    assert (best64, best33) == (at64, over32)
    # lane 63 and bit 63: a degree-64 row whose last edge is in the mesh
    hub = int(np.argmax(np.diff(r.rowptr)))
    assert any(r.mesh[k][r.rowptr[hub] + 63] != 0 for k in range(r.ticks))


def test_p6_static_dense_has_surplus(oracle_path):
    r = inspect_ref.ref(oracle_path, "p6_static_dense")
    assert r.ipv4 is not None and r.score_params.IPColocationFactorThreshold == 10
    assert max(np.bincount(r.ipv4[r.col[r.rowptr[u]:r.rowptr[u + 1]]] & 0xFF).max() for u in r.observers) > 10
