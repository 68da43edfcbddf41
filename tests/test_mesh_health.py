"""Mesh health (include/gs_mesh_health.h) without a GPU: the Python option's own
checks, the ABI struct's layout, the reference (tests/mesh_health_ref.py) on
hand-made graphs, and the preconditions of tests/test_mesh_health_gpu.py on the
oracle alone, so that a pass on the GPU cannot be vacuous."""
import ctypes as C

import numpy as np
import pytest

import mesh_health_ref as mref
import scenarios
from pubsub_amd import GS_EV_JOIN, GS_EV_LEAVE, Millisecond, WithMeshHealth, _abi


# ---------------------------------------------------------------- (a) pure Python
def test_option_arguments(oracle_path):
    with pytest.raises(ValueError):
        WithMeshHealth(100 * Millisecond, ticks=0)
    key, val = WithMeshHealth(300 * Millisecond, nodes=[True, False], labels=True)
    assert key == "mesh_health" and val["ticks"] == 64 and val["labels"] and val["period"] == 300 * Millisecond
    for period in (150 * Millisecond, 0, -100 * Millisecond):
        with pytest.raises(ValueError, match="WithMeshHealth: period .* multiple of the hop"):
            scenarios.SCENARIOS["gossipsub_dense"](oracle_path, (WithMeshHealth(period),))
    with pytest.raises(ValueError, match="one entry per host"):
        scenarios.SCENARIOS["gossipsub_dense"](oracle_path, (WithMeshHealth(100 * Millisecond, nodes=[1, 0]),))
    # valid arguments get as far as the library: the oracle does not export gs_mesh_health.h
    with pytest.raises(ValueError, match="product library only"):
        scenarios.SCENARIOS["gossipsub_dense"](oracle_path, (WithMeshHealth(300 * Millisecond),))


def test_abi_struct_layout():
    S = _abi.MeshHealthConfigC
    assert C.sizeof(S) == 32
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [
        ("period_hops", 0), ("ticks", 8), ("include", 16), ("labels", 24)]
    assert _abi.GS_MESH_SIZE_BINS == 32 and _abi.MESH_ROW_FIELDS == list(mref.FIELDS)
    assert [n for n, _, _ in _abi.MESH_HEALTH_FUNCTIONS] == [
        "gs_set_mesh_health", "gs_mesh_health_ticks", "gs_read_mesh_health_row", "gs_read_mesh_labels",
        "gs_read_mesh_health_kernel_stats"]


# ---------------------------------------------------------------- (b) the reference by hand
def _csr(n, pairs):
    adj = [[] for _ in range(n)]
    for a, b in pairs:
        adj[a].append(b)
        adj[b].append(a)
    rowptr = np.concatenate([[0], np.cumsum([len(x) for x in adj])]).astype(np.int64)
    col = np.array([v for x in adj for v in sorted(x)], dtype=np.int32)
    return rowptr, col


def test_ref_by_hand():
    """Six hosts, one topic: 0 - 1 - 2 a path, 3 - 4 one-sided (3 holds 4 only),
    5 holds only 4, which is excluded in the second reading."""
    rowptr, col = _csr(6, [(0, 1), (1, 2), (3, 4), (4, 5)])
    # edges in CSR order: 0>1, 1>0, 1>2, 2>1, 3>4, 4>3, 4>5, 5>4
    mesh = np.array([1, 1, 1, 1, 1, 0, 0, 1], dtype=np.uint64)
    subs = np.ones(6, dtype=np.uint64)
    h = mref.health(rowptr, col, mesh, subs, 1)
    got = [int(h[f][0]) for f in mref.FIELDS]
    assert got == [6, 4, 3, 3, 2, 0, 0]  # components {0, 1, 2}, {3}, {4}, {5}
    assert h["comp_hist"][0, :3].tolist() == [3, 1, 0] and h["labels"][:, 0].tolist() == [0, 0, 0, 3, 4, 5]
    inc = np.array([1, 1, 1, 1, 0, 1], dtype=np.uint8)
    h = mref.health(rowptr, col, mesh, subs, 1, include=inc)
    got = [int(h[f][0]) for f in mref.FIELDS]
    assert got == [5, 3, 3, 2, 0, 2, 2] and h["labels"][:, 0].tolist() == [0, 0, 0, 3, -1, 5]
    # host 1 not joined: the path falls apart, its own mesh entries count for nothing
    subs[1] = 0
    h = mref.health(rowptr, col, mesh, subs, 1)
    assert [int(h[f][0]) for f in mref.FIELDS][:4] == [5, 5, 1, 5] and h["labels"][1, 0] == -1
    # a floodsub host is no member either
    routers = np.full(6, _abi.GS_ROUTER_GOSSIPSUB, dtype=np.uint8)
    routers[0] = _abi.GS_ROUTER_FLOODSUB
    routers[2] = _abi.GS_ROUTER_GOSSIPSUB_V10
    h = mref.health(rowptr, col, mesh, np.ones(6, dtype=np.uint64), 1, routers=routers)
    assert int(h["members"][0]) == 5 and h["labels"][:3, 0].tolist() == [-1, 1, 1]


def test_ref_long_path_with_shuffled_ids():
    """A path of 300 hosts numbered at random: one component labelled 0."""
    order = np.random.default_rng(3).permutation(300)
    rowptr, col = _csr(300, [(int(order[i]), int(order[i + 1])) for i in range(299)])
    h = mref.health(rowptr, col, np.ones(len(col), dtype=np.uint64), np.ones(300, dtype=np.uint64), 1)
    assert [int(h[f][0]) for f in mref.FIELDS] == [300, 1, 300, 0, 0, 0, 0]
    assert not h["labels"].any() and h["comp_hist"][0, 8] == 1


def test_subs_at_applies_the_events_of_earlier_hops():
    subs = np.array([1, 1, 0], dtype=np.uint64)
    ev = [(5, GS_EV_LEAVE, 0, 0), (7, GS_EV_JOIN, 0, 0), (7, GS_EV_JOIN, 2, 0), (7, GS_EV_LEAVE, 2, 0),
          (9, GS_EV_LEAVE, 1, 0)]
    assert mref.subs_at(subs, ev, 5).tolist() == [1, 1, 0]  # the hop counter 5: hops 0 .. 4 ran
    assert mref.subs_at(subs, ev, 6).tolist() == [0, 1, 0]
    assert mref.subs_at(subs, ev, 8).tolist() == [1, 1, 1]  # a hop's leaves come before its joins
    assert mref.subs_at(subs, ev, 10).tolist() == [1, 0, 1]


# ---------------------------------------------------------------- (c) the oracle alone
def test_ring_closed_form(oracle_path):
    e = mref.ring_engine(oracle_path)
    for k in range(mref.RING_HOPS // mref.PERIOD):
        e.step(mref.PERIOD)
        h = mref.of_engine(e)
        for t in range(2):
            assert tuple(int(h[f][t]) for f in mref.FIELDS[:5]) == mref.ring_want(k), (k, t)
    assert [mref.ring_want(k)[1] for k in range(5)] == [1, 1, 2, 2, 2]
    assert np.array_equal(h["labels"], mref.ring_labels())
    e.close()


def test_adversarial_mix_falls_apart_around_the_sybils(oracle_path):
    r = mref.ref(oracle_path, "adversarial_mix")
    comp = r.series("components")[:, 0]
    assert r.ticks == 10 and comp[0] == 1 and comp[9] > 40
    assert r.series("one_sided").max() > 0
    h = mref.ref(oracle_path, "adversarial_mix", "honest")
    assert int(h.mask.sum()) == 309
    assert (h.series("components") == 1).all() and (h.series("largest") == 309).all()
    assert (h.series("members") == 309).all() and h.series("outside").max() > 0


def test_squatters_hold_honest_mesh_slots(oracle_path):
    r = mref.ref(oracle_path, "squatters", "honest")
    assert int(r.mask.sum()) == 10 and r.ticks == 28
    assert (r.series("components") == 1).all() and (r.series("largest") == 10).all()
    assert (r.series("outside") > 0).any()


def test_churn_scored_one_sided_entries_move(oracle_path):
    r = mref.ref(oracle_path, "churn_scored")
    one = r.series("one_sided")
    assert r.T == 2 and all(len(set(one[:, t].tolist())) >= 2 for t in range(2))
    # the members follow the JOIN / LEAVE events: some tick has a host out of each topic
    assert (r.series("members").min(axis=0) < r.N).all()


def test_mixed_scored_has_hosts_that_are_no_members(oracle_path):
    r = mref.ref(oracle_path, "mixed_scored")
    e, _ = scenarios.SCENARIOS["mixed_scored"](oracle_path)
    other = np.flatnonzero(e.routers < _abi.GS_ROUTER_GOSSIPSUB)
    subscribed = [int(((e.subs >> np.uint64(t)) & np.uint64(1)).sum()) for t in range(r.T)]
    e.close()
    assert len(other) > 10 and (r.labels[other] == -1).all()
    assert (r.series("members")[-1] < np.array(subscribed)).all()


@pytest.mark.parametrize("name,T", [("ladder_64t_sub", 64), ("ladder_multitopic", 3)])
def test_ladder_cases_have_partial_subscriptions(oracle_path, name, T):
    r = mref.ref(oracle_path, name)
    assert r.T == T and r.ticks >= 8
    assert (r.series("members") > 0).all() and (r.series("members") < r.N).all()
    # the ladder's isolated and pendant hosts: singletons at every tick
    assert (r.series("isolated") > 0).all() and (r.series("components") > 1).all()
