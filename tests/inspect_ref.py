"""Reference for WithPeerScoreInspect (include/gs_inspect.h), oracle only: the
scenario on the CPU oracle, stepped `period` hops at a time; after each piece
scores() and mesh() are read, and for the sampled edges topic_stats_at() and
behaviour_penalty().  The rows are binned with numpy exactly as the header
defines them.  Stepping the oracle in pieces with reads in between ends in
the same scores and meshes, bit for bit, as one whole step
(tests/test_inspect.py checks it), so it is a valid yardstick for ticks taken
inside one gs_step."""
import functools

import numpy as np

import scenarios
from pubsub_amd import GossipSubParams, default_inspect_bounds, eth2_thresholds

DEG_BINS = 65


def _wide_params():
    return GossipSubParams(D=48, Dlo=40, Dhi=64, Dout=2, Dscore=4)


def ladder_wide_mesh(T):
    """The ladder with meshes as wide as a row: D = 48, Dlo = 40, Dhi = 64, so
    the degree-64 hubs keep every peer in the mesh (mesh_deg's last bin, lane
    63 and bit 63 of the transposed masks)."""
    return lambda lib, x=(): scenarios.gossipsub_scored(
        lib, graph=scenarios.ladder_graph(), authors=scenarios.LADDER_AUTHORS, topics=T, seed=39, msgs=300, hb=6,
        window=256, params=_wide_params(), extra=x)


LOCAL = {"ladder_wide_mesh_4t": ladder_wide_mesh(4), "ladder_wide_mesh_64t": ladder_wide_mesh(64)}
# scenario: period in hops
PERIOD = {
    "gossipsub_scored": 1,
    "gossipsub_multitopic": 7,
    "gossipsub_negative_app": 10,
    "adversarial_mix": 10,
    "churn_scored": 10,
    "p6_churn_heavy": 10,
    "mixed_scored": 10,
    "ladder_64t": 7,
    "ladder32_64t": 10,
    "ladder_wide_mesh_4t": 3,
    "ladder_wide_mesh_64t": 3,
    "p6_static_dense": 10,
}
# bounds other than the default: a score of exactly -150 (the app score times
# its weight 1 of a peer that delivered nothing) and of exactly 0 against the
# bounds -150 and 0
BOUNDS = {"gossipsub_negative_app": [-300.0, -150.0, 0.0, 1.0]}


def builder(name):
    return LOCAL[name] if name in LOCAL else scenarios.SCENARIOS[name]


def bounds_of(name):
    return np.array(BOUNDS.get(name, default_inspect_bounds(eth2_thresholds())), dtype=np.float64)


def observers_of(rowptr, seed=5):
    """A node of the largest degree (a degree-64 hub on the ladder), one of
    degree 1 (a pendant node) and one of degree 0 (an isolated node) where the
    graph has them, and five random nodes."""
    deg = np.diff(rowptr)
    pick = {int(np.argmax(deg))}
    for d in (1, 0):
        if (deg == d).any():
            pick.add(int(np.flatnonzero(deg == d)[0]))
    pick.update(int(u) for u in np.random.default_rng(seed).choice(len(deg), 5, replace=False))
    return sorted(pick)


def edges_of(rowptr, nodes, node_range=None):
    n0, n1 = node_range if node_range is not None else (0, len(rowptr) - 1)
    own = [u for u in nodes if n0 <= u < n1]
    return np.array([e for u in own for e in range(int(rowptr[u]), int(rowptr[u + 1]))], dtype=np.int64)


def score_hist(bounds, scores):
    return np.bincount(np.searchsorted(bounds, scores, side="right"), minlength=len(bounds) + 1).astype(np.int64)


def mesh_deg(rowptr, mesh, T, node_range=None):
    """int64 [T, 65]: nodes of [n0, n1) by the number of their edges whose mesh word holds topic t."""
    n0, n1 = node_range if node_range is not None else (0, len(rowptr) - 1)
    src = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    out = np.zeros((T, DEG_BINS), dtype=np.int64)
    for t in range(T):
        deg = np.bincount(src, weights=((mesh >> np.uint64(t)) & np.uint64(1)).astype(np.float64),
                          minlength=len(rowptr) - 1).astype(np.int64)
        out[t] = np.bincount(deg[n0:n1], minlength=DEG_BINS)
    return out


class Ref:
    """An oracle run read every `period` hops: scores[k] and mesh[k] of every
    edge at tick k, and stats[k] (topic_stats_at), bp[k] of the sampled edges."""

    def __init__(self, oracle, name):
        e, hops = builder(name)(oracle)
        self.name, self.hops, self.period = name, hops, PERIOD[name]
        self.N, self.T, self.E = e.N, e.T, e.E
        self.rowptr, self.col = e.rowptr.copy(), e.col.copy()
        self.bounds = bounds_of(name)
        self.observers = observers_of(self.rowptr)
        self.edges = edges_of(self.rowptr, self.observers)
        self.app = e.app_attr.copy() if e.app_attr is not None else np.zeros(e.N)
        self.ipv4 = e.ipv4_attr.copy() if e.ipv4_attr is not None else None
        self.score_params = e.score_params
        self.ticks = hops // self.period
        self.scores, self.mesh, self.stats, self.bp = [], [], [], []
        for _ in range(self.ticks):
            e.step(self.period)
            self.scores.append(e.scores())
            self.mesh.append(e.mesh())
            self.stats.append(e.topic_stats_at(self.edges))
            self.bp.append(e.behaviour_penalty()[self.edges])
        e.step(hops - self.ticks * self.period)
        self.final_scores, self.final_mesh = e.scores(), e.mesh()
        e.close()
        for a in self.scores + self.mesh + self.bp + [self.final_scores, self.final_mesh]:
            a.setflags(write=False)

    def hop(self, k):
        return (k + 1) * self.period

    def score_hist(self, k, node_range=None):
        n0, n1 = node_range if node_range is not None else (0, self.N)
        return score_hist(self.bounds, self.scores[k][self.rowptr[n0]:self.rowptr[n1]])

    def mesh_deg(self, k, node_range=None):
        return mesh_deg(self.rowptr, self.mesh[k], self.T, node_range)


@functools.lru_cache(maxsize=None)
def ref(oracle, name):
    """The oracle's run of a PERIOD scenario (shared, read only)."""
    return Ref(oracle, name)


def score_from_parts(sp, T, tim, fmd, mmd, imd, mfp, flags, app, ipc, bp):
    """peerScore.score (score.go:256-333) of one peer from a PeerScoreSnapshot's
    parts (tim .. imd per topic, app, ipc, bp) and the two things a snapshot
    does not carry: MeshFailurePenalty and the in-mesh / P3-active flags.  Plain
    Python floats: the reference's operations in the reference's order."""
    score = 0.0
    for t in range(T):
        tp = sp.Topics.get(t)
        if tp is None:
            continue
        ts = 0.0
        if flags[t] & 1:
            p1 = float(int(tim[t]) // tp.TimeInMeshQuantum)
            if p1 > tp.TimeInMeshCap:
                p1 = tp.TimeInMeshCap
            ts += p1 * tp.TimeInMeshWeight
        ts += float(fmd[t]) * tp.FirstMessageDeliveriesWeight
        if flags[t] & 2 and float(mmd[t]) < tp.MeshMessageDeliveriesThreshold:
            deficit = tp.MeshMessageDeliveriesThreshold - float(mmd[t])
            ts += (deficit * deficit) * tp.MeshMessageDeliveriesWeight
        ts += float(mfp[t]) * tp.MeshFailurePenaltyWeight
        ts += (float(imd[t]) * float(imd[t])) * tp.InvalidMessageDeliveriesWeight
        score += ts * tp.TopicWeight
    if sp.TopicScoreCap > 0 and score > sp.TopicScoreCap:
        score = sp.TopicScoreCap
    score += float(app) * sp.AppSpecificWeight
    score += float(ipc) * sp.IPColocationFactorWeight
    if float(bp) > sp.BehaviourPenaltyThreshold:
        excess = float(bp) - sp.BehaviourPenaltyThreshold
        score += (excess * excess) * sp.BehaviourPenaltyWeight
    return score
