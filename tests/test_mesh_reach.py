"""Mesh reach (include/gs_mesh_reach.h) without a GPU: the Python option's own
checks, the ABI struct's layout, the reference (tests/mesh_reach_ref.py) on a
hand-made graph, and the preconditions of tests/test_mesh_reach_gpu.py on the
oracle alone: that the structural depth is what eager push really does, the
ring's closed form, and that the scenarios cover what the GPU tests claim to."""
import ctypes as C

import numpy as np
import pytest

import mesh_health_ref as mhref
import mesh_reach_ref as rref
import scenarios
from pubsub_amd import Millisecond, WithMeshReach, _abi


# ---------------------------------------------------------------- (a) pure Python
def test_option_arguments(oracle_path):
    with pytest.raises(ValueError, match="ticks"):
        WithMeshReach(100 * Millisecond, [0], ticks=0)
    for bad in ([], list(range(_abi.GS_REACH_MAX_SOURCES + 1)), [[0, 1]], [0.5]):
        with pytest.raises(ValueError, match="sources must be"):
            WithMeshReach(100 * Millisecond, bad)
    with pytest.raises(ValueError, match="given twice"):
        WithMeshReach(100 * Millisecond, [3, 4, 3])
    key, val = WithMeshReach(300 * Millisecond, [5, 2], nodes=[True, False], depths=True)
    assert key == "mesh_reach" and val["ticks"] == 64 and val["depths"] and val["period"] == 300 * Millisecond
    assert val["sources"].tolist() == [5, 2]
    for period in (150 * Millisecond, 0, -100 * Millisecond):
        with pytest.raises(ValueError, match="WithMeshReach: period .* multiple of the hop"):
            scenarios.SCENARIOS["gossipsub_dense"](oracle_path, (WithMeshReach(period, [0]),))
    with pytest.raises(ValueError, match="one entry per host"):
        scenarios.SCENARIOS["gossipsub_dense"](oracle_path, (WithMeshReach(100 * Millisecond, [0], nodes=[1, 0]),))
    for src in ([20], [-1, 3]):  # gossipsub_dense has 20 hosts
        with pytest.raises(ValueError, match="a source is outside 0 .. 19"):
            scenarios.SCENARIOS["gossipsub_dense"](oracle_path, (WithMeshReach(100 * Millisecond, src),))
    # valid arguments get as far as the library: the oracle does not export gs_mesh_reach.h
    with pytest.raises(ValueError, match="product library only"):
        scenarios.SCENARIOS["gossipsub_dense"](oracle_path, (WithMeshReach(300 * Millisecond, [0, 19]),))


def test_abi_struct_layout():
    S = _abi.MeshReachConfigC
    assert C.sizeof(S) == 40
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [
        ("period_hops", 0), ("ticks", 8), ("num_sources", 12), ("sources", 16), ("include", 24), ("depths", 32)]
    assert _abi.GS_REACH_DEPTH_BINS == rref.DEPTH_BINS == 64 and _abi.GS_REACH_MAX_SOURCES >= 256
    assert _abi.REACH_ROW_FIELDS == list(rref.FIELDS)
    assert [n for n, _, _ in _abi.MESH_REACH_FUNCTIONS] == [
        "gs_set_mesh_reach", "gs_mesh_reach_ticks", "gs_read_mesh_reach_row", "gs_read_mesh_reach_depths",
        "gs_read_mesh_reach_kernel_stats"]
    assert len(_abi.REACH_STAT_NAMES) == 7


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
    """Seven hosts, one topic.  0 > 1 > 2 one-sided mesh edges, 2 > 3 and 0 > 3
    too (3 at depth 1, not 3), 3 > 4 with 4 excluded in the second reading and
    4 > 5 behind it; 6 is not joined and publishes through a fanout edge to 0."""
    rowptr, col = _csr(7, [(0, 1), (1, 2), (2, 3), (0, 3), (3, 4), (4, 5), (0, 6)])
    # edges in CSR order: 0>1 0>3 0>6 | 1>0 1>2 | 2>1 2>3 | 3>0 3>2 3>4 | 4>3 4>5 | 5>4 | 6>0
    mesh = np.array([1, 1, 0, 0, 1, 0, 1, 0, 0, 1, 0, 1, 0, 0], dtype=np.uint64)
    fanout = np.zeros(14, dtype=np.uint64)
    fanout[13] = 1
    subs = np.array([1, 1, 1, 1, 1, 1, 0], dtype=np.uint64)
    r = rref.reach(rowptr, col, mesh, fanout, subs, 1, [0, 6, 5])
    assert r["depths"][0, :, 0].tolist() == [0, 1, 2, 1, 2, 3, 255]
    assert r["depths"][1, :, 0].tolist() == [1, 2, 3, 2, 3, 4, 0]  # the unjoined publisher's first hop is its fanout
    assert r["depths"][2, :, 0].tolist() == [255] * 5 + [0, 255]  # 5 holds nobody: the edges are directed
    assert r["reached"][:, 0].tolist() == [5, 6, 0] and r["unreached"][:, 0].tolist() == [0, 0, 5]
    assert r["ecc"][:, 0].tolist() == [3, 4, 0]
    assert r["depth_hist"][0, 0, :5].tolist() == [0, 2, 2, 1, 0] and r["depth_hist"][2, 0].sum() == 0
    # 4 excluded: never reached, so it relays nothing and 5 is cut off; as a source it still publishes
    inc = np.array([1, 1, 1, 1, 0, 1, 1], dtype=np.uint8)
    r = rref.reach(rowptr, col, mesh, fanout, subs, 1, [0, 4], include=inc)
    assert r["depths"][0, :, 0].tolist() == [0, 1, 2, 1, 255, 255, 255]
    assert (r["reached"][0, 0], r["unreached"][0, 0], r["ecc"][0, 0]) == (3, 1, 2)
    assert r["depths"][1, :, 0].tolist() == [255, 255, 255, 255, 0, 1, 255]
    assert (r["reached"][1, 0], r["unreached"][1, 0]) == (1, 4)  # five members, none of them the source
    # a floodsub host is no target
    routers = np.full(7, _abi.GS_ROUTER_GOSSIPSUB, dtype=np.uint8)
    routers[1] = _abi.GS_ROUTER_FLOODSUB
    r = rref.reach(rowptr, col, mesh, fanout, subs, 1, [0], routers=routers)
    assert r["depths"][0, :, 0].tolist() == [0, 255, 255, 1, 2, 3, 255]


def test_ref_depth_bins_and_clip():
    """A directed path of 300 hosts: bin 63 holds the depths 63 .. 299, the
    depth table clips at 254."""
    rowptr, col = _csr(300, [(i, i + 1) for i in range(299)])
    src = np.repeat(np.arange(300), np.diff(rowptr))
    mesh = (col > src).astype(np.uint64)
    r = rref.reach(rowptr, col, mesh, np.zeros_like(mesh), np.ones(300, dtype=np.uint64), 1, [0])
    assert (r["reached"][0, 0], r["unreached"][0, 0], r["ecc"][0, 0]) == (299, 0, 299)
    assert r["depth_hist"][0, 0].tolist() == [0] + [1] * 62 + [237]
    assert r["depths"][0, :, 0].tolist() == list(range(255)) + [254] * 45


def test_ref_side_by_side_equals_one_at_a_time(oracle_path):
    """reach()'s searches on whole arrays against the plain queue, on a mesh
    with one-sided edges, fanout, partial subscriptions and a mask."""
    e, _ = scenarios.SCENARIOS["ladder_multitopic"](oracle_path)
    e.step(37)
    mask = np.arange(e.N) % 3 != 0
    sources = rref.sources_of(e, mask, count=12)
    r = rref.of_engine(e, sources, mask)
    mem = rref.members(mhref.subs_at(e.subs, e.events, e.hop), e.T, mask, e.routers)
    adj = rref.eager_lists(e.rowptr, e.col, e.mesh(), e.fanout(), e.T)
    assert e.fanout().any() and (r["depths"] == 255).any() and r["ecc"].max() >= 3
    for t in range(e.T):
        for k, s in enumerate(sources):
            d = rref.depth_from(adj[t], mem[:, t], int(s))
            want = np.where(d < 0, 255, np.minimum(d, 254))
            assert np.array_equal(r["depths"][k, :, t], want), (k, t)
            assert r["reached"][k, t] == (d > 0).sum() and r["ecc"][k, t] == d.max()
    e.close()


# ---------------------------------------------------------------- (c) the oracle alone
def _depth_equals_delivery_age(oracle_path, name):
    """Steps the oracle hop by hop; for every message, the reference depth from
    its author on its topic at the tick after its publish hop against the
    first-delivery age at every host.  Returns (messages, pairs compared, pairs
    that differ, pairs that differ with the snapshot before the publish hop,
    topics that have an unjoined author)."""
    e, hops = scenarios.SCENARIOS[name](oracle_path)
    pub = {}
    for m, h in enumerate(e.msg_hop.tolist()):
        pub.setdefault(h, []).append(m)
    depth, before = {}, {}

    def take(into, hop):
        subs = mhref.subs_at(e.subs, e.events, e.hop)
        mem = rref.members(subs, e.T, None, e.routers)
        adj = rref.eager_lists(e.rowptr, e.col, e.mesh(), e.fanout(), e.T)
        for m in pub.get(hop, ()):
            t = int(e.msg_topic[m])
            into[m] = rref.depth_from(adj[t], mem[:, t], int(e.msg_src[m]))

    for _ in range(hops):
        take(before, e.hop)  # the hop counter is h: hop h has not run
        e.step(1)
        take(depth, e.hop - 1)  # the hop counter has become h + 1
    assert len(depth) == e.n_published == len(before)
    pairs = differ = differ_before = 0
    unjoined = set()
    for m in range(e.n_published):
        s, t, h = int(e.msg_src[m]), int(e.msg_topic[m]), int(e.msg_hop[m])
        if not (int(e.subs[s]) >> t) & 1:
            unjoined.add(t)
        at, _ = e.deliveries(m)
        age = np.where(at >= 0, at.astype(np.int64) - h, -1)  # a host the message never came to: not reached
        assert age[s] == 0 and depth[m][s] == 0
        pairs += e.N
        differ += int((age != depth[m]).sum())
        differ_before += int((age != before[m]).sum())
    T = e.T
    e.close()
    return e.n_published, pairs, differ, differ_before, unjoined, T


def test_depth_is_first_delivery_age_multitopic(oracle_path):
    msgs, pairs, differ, differ_before, unjoined, T = _depth_equals_delivery_age(oracle_path, "gossipsub_multitopic")
    assert (msgs, pairs) == (240, 48000)
    assert differ == 0
    assert differ_before > 0  # the fanout is made by the publish: the tick is taken after the hop
    assert unjoined == set(range(T))  # every topic has an author that publishes through fanout


def test_depth_is_first_delivery_age_dense(oracle_path):
    msgs, pairs, differ, _, _, _ = _depth_equals_delivery_age(oracle_path, "gossipsub_dense")
    assert (msgs, pairs) == (100, 2000) and differ == 0


def test_ring_closed_form(oracle_path):
    e = mhref.ring_engine(oracle_path)
    n = mhref.RING_N
    for k in range(mhref.RING_HOPS // rref.PERIOD):
        e.step(rref.PERIOD)
        r = rref.of_engine(e, [0])
        reached, unreached, ecc, hist, depths = rref.ring_want(k)
        for t in range(2):
            assert (r["reached"][0, t], r["unreached"][0, t], r["ecc"][0, t]) == (reached, unreached, ecc), (k, t)
            assert np.array_equal(r["depth_hist"][0, t], hist) and np.array_equal(r["depths"][0, :, t], depths)
    # before the cut: two hosts at each depth 1 .. 99, one at 100; bins 1 .. 62 hold 2 each, bin 63 holds 75
    reached, unreached, ecc, hist, _ = rref.ring_want(1)
    assert (reached, unreached, ecc) == (n - 1, 0, 100)
    assert hist.tolist() == [0] + [2] * 62 + [75]
    # after it: 199, 198, ..., 101 at depths 1 .. 99, and 100 targets unreached
    reached, unreached, ecc, hist, depths = rref.ring_want(4)
    assert (reached, unreached, ecc) == (99, 100, 99) and hist.tolist() == [0] + [1] * 62 + [37]
    assert depths[101:].tolist() == list(range(99, 0, -1)) and (depths[1:101] == 255).all()
    e.close()


@pytest.mark.parametrize("name,key", rref.CASES)
def test_cases_have_unreached_targets(oracle_path, name, key):
    r = rref.ref(oracle_path, name, key)
    assert r.ticks >= 8 and len(r.sources) == rref.NUM_SOURCES == len(set(r.sources.tolist()))
    assert r.series("unreached").max() > 0 and r.series("reached").max() > 0
    assert r.series("ecc").max() >= 2


def test_cases_cover_the_sources_that_matter(oracle_path):
    lad = rref.ref(oracle_path, "ladder_64t_sub")
    deg = lad.degree[lad.sources]
    assert lad.T == 64 and deg.min() == 0 and deg.max() == 64
    k0 = int(np.argmin(deg))  # a source without connections reaches nobody, at any tick
    assert (lad.series("reached")[:, k0] == 0).all() and (lad.series("unreached")[:, k0] > 0).all()
    adv = rref.ref(oracle_path, "adversarial_mix", "honest")
    outside = np.flatnonzero(~adv.mask[adv.sources])
    assert len(outside) >= 1 and int(adv.mask.sum()) == 309
    # an excluded source is no target of the others: its rows in their tables stay 255
    others = np.setdiff1d(np.arange(len(adv.sources)), outside)
    assert (adv.depths[others][:, adv.sources[outside]] == 255).all()
    churn = rref.ref(oracle_path, "churn_scored")
    m = churn.series("reached") + churn.series("unreached")  # the targets follow the JOIN / LEAVE events
    assert len(np.unique(m[:, 0, 0])) >= 2
