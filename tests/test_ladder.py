"""Preconditions of the degree-ladder scenarios (scenarios.LADDER), on the
oracle alone: the graphs hold every degree class the one-wave-per-node kernels
branch on, every first delivery stays inside the engine's message window (so a
late-delivery error from the GPU on these scenarios is a parity failure, not
the documented limit), every schedule has authors of degree 64, 1 and 0, and
the runs reach the branches they are there for (Dhi pruning on the hubs,
randomsub's selection at degree > 32, k_push's region overflow)."""
import functools
import math

import numpy as np
import pytest

import scenarios
from pubsub_amd import WithEventTracer, _abi, graphs
from pubsub_amd.params import GossipSubParams
from test_trace_rpc import ITEM, SEND, blocks

FULL = sorted(n for n in scenarios.LADDER if not n.startswith("ladder32_"))
CAP32 = sorted(n for n in scenarios.LADDER if n.startswith("ladder32_"))
# the adversarial model (validation drops, the gater, spam) delivers late by
# design and runs with the 11-heartbeat window (gs_engine.h setWindow)
ADVERSARIAL = {"ladder_adversarial", "ladder_px_adversarial"}
# message window of the engine in hops: 3 heartbeats; 11 once events are scheduled
WINDOW = {name: 30 for name in scenarios.LADDER if name not in ADVERSARIAL}
WINDOW["ladder_churn"] = 110
HUB0, PENDANT, ISOLATED = scenarios.LADDER_AUTHORS


@functools.lru_cache(maxsize=None)
def ran(oracle, name):
    """The oracle's engine after the scenario's run (shared, read only)."""
    e, hops = scenarios.SCENARIOS[name](oracle)
    e.step(hops)
    return e


def _readable(e):
    return getattr(e, "snapshot_ids", range(e.n_published))


# ---------------------------------------------------------------- the builder
def test_degree_ladder_builder():
    n = scenarios.LADDER_N
    rowptr, col, outbound = graphs.degree_ladder(n, 97)
    deg = np.diff(rowptr)
    hubs = graphs.LADDER_HUBS
    assert deg[:len(hubs)].tolist() == list(hubs)
    assert (deg[n - 2:] == 0).all() and (deg[n - 6:n - 2] == 1).all()
    body = np.arange(len(hubs), n - 6)
    assert deg[body].min() >= 3 and deg[body].max() <= 64
    src = np.repeat(np.arange(n), deg)
    # symmetric, rows strictly ascending, no self loops, one dialer per pair
    und = {(int(u), int(v)): int(o) for u, v, o in zip(src, col, outbound)}
    assert len(und) == len(col) and all(u != v for u, v in und)
    assert all(und[(v, u)] == 1 - o for (u, v), o in und.items())
    assert all(np.all(np.diff(col[rowptr[u]:rowptr[u + 1]]) > 0) for u in range(n))
    assert 0 < outbound[rowptr[0]:rowptr[1]].sum() < 64  # the dialer is drawn per pair
    # hub neighbours are body nodes, but for the 0 - 1 connection; pendants hang on the body
    for h in range(len(hubs)):
        nb = set(col[rowptr[h]:rowptr[h + 1]].tolist())
        assert nb - set(body.tolist()) == ({1} if h == 0 else {0} if h == 1 else set())
    assert all(col[rowptr[p]] in body for p in range(n - 6, n - 2))
    # same seed, same graph; another seed, another graph
    again = graphs.degree_ladder(n, 97)
    assert all(np.array_equal(a, b) for a, b in zip((rowptr, col, outbound), again))
    assert not np.array_equal(col, graphs.degree_ladder(n, 98)[1])


def test_degree_ladder_refuses_what_it_cannot_build():
    with pytest.raises(ValueError, match="hub 0 cannot reach degree 64"):
        graphs.degree_ladder(60, 1)  # a body of 42 nodes
    with pytest.raises(ValueError, match="> 32"):
        graphs.degree_ladder(160, 1, max_degree=32)
    deg = np.diff(graphs.degree_ladder(160, 1, hubs=graphs.LADDER32_HUBS, max_degree=32)[0])
    assert deg.max() == 32 and deg[:5].tolist() == list(graphs.LADDER32_HUBS)


# ---------------------------------------------------------------- degree sets
@pytest.mark.parametrize("name", FULL)
def test_full_ladder_degrees(oracle_path, name):
    e, _ = scenarios.SCENARIOS[name](oracle_path)
    deg = np.diff(e.rowptr)
    assert e.N == scenarios.LADDER_N and deg.max() == 64
    assert {0, 1, 31, 32, 33, 63, 64} <= set(deg.tolist())
    assert deg[0] == 64 and deg[1] == 64 and 1 in e.col[e.rowptr[0]:e.rowptr[1]]
    assert deg[HUB0] == 64 and deg[PENDANT] == 1 and deg[ISOLATED] == 0


@pytest.mark.parametrize("name", CAP32)
def test_capped_ladder_degrees(oracle_path, name):
    e, _ = scenarios.SCENARIOS[name](oracle_path)
    deg = np.diff(e.rowptr)
    assert deg.max() == 32 and {0, 1, 32} <= set(deg.tolist())
    assert 1 in e.col[e.rowptr[0]:e.rowptr[1]]


# ---------------------------------------------------------------- delivery age
def max_age(e):
    age = -1
    for i in _readable(e):
        hop, _ = e.deliveries(i)
        if (hop >= 0).any():
            age = max(age, int(hop.max() - e.sched_hops[i]))
    return age


@pytest.mark.parametrize("name", sorted(WINDOW))
def test_first_deliveries_well_inside_the_window(oracle_path, name):
    """The oldest first delivery of the oracle's run is at least 10 hops inside
    the engine's message window: 20 hops of the 30 everywhere but ladder_churn,
    whose scheduled events give the engine the 110-hop window."""
    age = max_age(ran(oracle_path, name))
    print(name, "max delivery age", age)
    assert 0 <= age <= WINDOW[name] - 10


# ---------------------------------------------------------------- authors
@pytest.mark.parametrize("name", sorted(scenarios.LADDER))
def test_authors_of_degree_64_1_and_0(oracle_path, name):
    e = ran(oracle_path, name)
    deg = np.diff(e.rowptr)
    seen = set()
    for i in _readable(e):
        a = int(e.sched_src[i])
        if a not in scenarios.LADDER_AUTHORS or (name in ADVERSARIAL and e.sybil[a]):
            continue
        hop, frm = e.deliveries(i)
        if hop[a] != e.sched_hops[i] or frm[a] >= 0:
            continue  # (an invalid or phantom message: not delivered to its author)
        seen.add(a)
        if deg[a] == 0:  # an isolated author delivers to itself only
            assert np.flatnonzero(hop >= 0).tolist() == [a]
    assert seen == set(scenarios.LADDER_AUTHORS)
    assert deg[HUB0] == deg.max() and deg[PENDANT] == 1 and deg[ISOLATED] == 0


# ---------------------------------------------------------------- not vacuous
@pytest.mark.parametrize("name", ["ladder_scored", "ladder_64t"])
def test_hubs_are_pruned_into_the_mesh_bounds(oracle_path, name):
    e = ran(oracle_path, name)
    gp = GossipSubParams()
    assert e.counters()["prunes_sent"] > 0
    mesh = e.mesh()
    checked = 0
    for h in range(len(graphs.LADDER_HUBS)):
        row = slice(e.rowptr[h], e.rowptr[h + 1])
        for t in range(e.T):
            bit = np.uint64(1) << np.uint64(t)
            if not (e.subs[h] & bit) or ((e.subs[e.col[row]] & bit) != 0).sum() < gp.Dhi:
                continue
            md = int(((mesh[row] & bit) != 0).sum())
            assert gp.Dlo <= md <= gp.Dhi, (h, t, md)
            checked += 1
    assert checked == len(graphs.LADDER_HUBS) * e.T  # all subscribed: every hub, every topic


def test_randomsub_selects_at_degree_over_32(oracle_path):
    """A message first held by a degree-64 hub (its own publish) leaves it in
    exactly max(6, ceil(sqrt(100))) = 10 copies: the selection ran, not the
    send-to-all shortcut for hosts with no more peers than the target."""
    e, hops = scenarios.SCENARIOS["ladder_randomsub_100"](oracle_path, (WithEventTracer([HUB0], rpc=True),))
    e.step(hops)
    ev = e.trace_events()
    own = [i for i in range(e.n_published) if e.sched_src[i] == HUB0]
    assert own and np.diff(e.rowptr)[HUB0] > 32
    copies = {i: 0 for i in own}
    for hd, items in blocks(ev):
        if hd["type"] == SEND and hd["node"] == HUB0:
            for it in items[items["reason"] == _abi.GS_RPC_ITEM_MSG]:
                if int(it["msg"]) in copies:
                    copies[int(it["msg"])] += 1
    assert ITEM in ev["type"]
    assert all(c == max(6, math.ceil(math.sqrt(100))) for c in copies.values()), copies


def test_flood_burst_overflows_the_push_region(oracle_path):
    """ladder_4t_flood: hub 0's burst of 40 flood-published messages reaches its
    64 peers in one hop, more than GS_PUSHR = 2048 copies from one sender."""
    e = ran(oracle_path, "ladder_4t_flood")
    burst = [i for i in range(e.n_published) if e.sched_src[i] == HUB0 and e.sched_hops[i] == 40]
    assert len(burst) >= 40
    copies = 0
    for i in burst:
        hop, frm = e.deliveries(i)
        copies += int(((frm == HUB0) & (hop == 41)).sum())  # first deliveries: a lower bound
    assert copies > 2048


# ---------------------------------------------------------------- degree 0 / 1 state
def test_isolated_and_pendant_rows(oracle_path):
    e = ran(oracle_path, "ladder_scored")
    assert e.rowptr[ISOLATED] == e.rowptr[ISOLATED + 1] and e.rowptr[ISOLATED + 2] == e.E == len(e.mesh())
    assert e.rowptr[PENDANT + 1] - e.rowptr[PENDANT] == 1
    edge = int(e.rowptr[PENDANT])
    peer = int(e.col[edge])
    back = int(e.rowptr[peer]) + e.col[e.rowptr[peer]:e.rowptr[peer + 1]].tolist().index(PENDANT)
    scores = e.scores()
    assert np.isfinite(scores[edge]) and np.isfinite(scores[back])
    assert e.mesh()[edge] == 1 and e.mesh()[back] == 1  # its only peer is its mesh


# ---------------------------------------------------------------- past the limit
def test_oracle_accepts_degree_65(oracle_path):
    """The reference's AddPeer has no bound: the oracle runs the 65-leaf star
    the engine refuses (test_parity_gpu.py): the centre's flood-published
    message reaches all 65 leaves in one hop, a leaf's message the centre."""
    e, hops = scenarios.degree65_star(oracle_path)
    assert np.diff(e.rowptr).max() == 65
    e.step(hops)
    hop, frm = e.deliveries(0)
    assert hop[0] == 12 and (hop[1:] == 13).all() and (frm[1:] == 0).all()
    hop, frm = e.deliveries(1)
    assert hop[7] == 14 and hop[0] == 15 and frm[0] == 7
