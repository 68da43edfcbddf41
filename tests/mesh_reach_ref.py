"""Reference for mesh reach (include/gs_mesh_reach.h): the definitions of the
header in numpy over rowptr, col, a mesh and a fanout readback, the include
mask, the routers and the subscription words (mesh_health_ref.subs_at).  It
reads nothing but what the oracle's or the engine's existing readbacks return.

depth_from() is one plain breadth-first search for a (source, topic): a queue
of hosts that hold the message, each handing it over its eager edges to the
targets that do not hold it yet.  reach() runs that search for every source
and topic (depths_from(): a topic's searches side by side on whole arrays, which
tests/test_mesh_reach.py holds against depth_from()) and counts the header's row
from the depths.

Ref runs a scenario on the CPU oracle stepped `PERIOD` hops at a time (a tick
per heartbeat) with the scenario's SOURCES and keeps every tick's rows, the
last tick's depths and the final snapshot.  The searches from different sources
do not touch each other, so the rows of the first K sources are the rows of a
run with those K sources alone."""
import collections
import functools

import numpy as np

import mesh_health_ref as mhref
import scenarios
from pubsub_amd import GS_ROUTER_GOSSIPSUB, GS_ROUTER_GOSSIPSUB_V10

FIELDS = ("reached", "unreached", "ecc")
ROW = FIELDS + ("depth_hist",)
DEPTH_BINS = 64
PERIOD = mhref.PERIOD
NUM_SOURCES = 65  # a full pass and a second pass with one source
# (scenario, mask): the scenarios of tests/test_mesh_reach_gpu.py
# c4shape's hosts all subscribe to every topic and its meshes reach everybody:
# with every other host left out, a host whose mesh in-neighbours are all
# outside is a target that is not reached
CASES = [("ladder_64t_sub", None), ("ladder_multitopic", None), ("adversarial_mix", "honest"), ("churn_scored", None),
         ("c4shape", "even")]


def mask_of(e, key):
    if key == "even":
        return np.arange(e.N) % 2 == 0
    return mhref.mask_of(e, key)


def members(subs, T, include=None, routers=None):
    """bool [N, T]: the hosts that can be targets of each topic."""
    n = len(subs)
    inc = np.ones(n, dtype=bool) if include is None else np.asarray(include) != 0
    gossip = np.ones(n, dtype=bool)
    if routers is not None:
        gossip = (np.asarray(routers) == GS_ROUTER_GOSSIPSUB) | (np.asarray(routers) == GS_ROUTER_GOSSIPSUB_V10)
    bits = ((np.asarray(subs, dtype=np.uint64)[:, None] >> np.arange(T, dtype=np.uint64)[None, :]) & np.uint64(1)) != 0
    return bits & (inc & gossip)[:, None]


def eager_lists(rowptr, col, mesh, fanout, T):
    """out[t][u]: the peers v of u with bit t in (mesh | fanout)[u -> v]."""
    n = len(rowptr) - 1
    both = np.asarray(mesh, dtype=np.uint64) | np.asarray(fanout, dtype=np.uint64)
    src = np.repeat(np.arange(n), np.diff(rowptr))
    out = []
    for t in range(T):
        adj = [[] for _ in range(n)]
        on = np.flatnonzero((both >> np.uint64(t)) & np.uint64(1))
        for u, v in zip(src[on].tolist(), np.asarray(col)[on].tolist()):
            adj[u].append(v)
        out.append(adj)
    return out


def depth_from(adj, member, s):
    """int64 [N]: the depth of every host from source s over adj (one topic's
    eager lists) through the hosts of `member` (bool [N]); 0 at s, -1 where the
    message does not arrive."""
    depth = np.full(len(adj), -1, dtype=np.int64)
    depth[s] = 0
    queue = collections.deque([s])
    while queue:
        u = queue.popleft()
        for v in adj[u]:
            if depth[v] < 0 and member[v]:
                depth[v] = depth[u] + 1
                queue.append(v)
    return depth


def depths_from(src, col, eager, member, sources):
    """int64 [K, N]: depth_from() for every source of one topic, the K searches
    side by side, one row of the tables each (they share nothing but the edge
    arrays): level by level, a host that does not hold the message yet takes it
    if any of its eager in-neighbours held it at the level before.  eager: bool
    [E], the topic's eager edges."""
    n, K = len(member), len(sources)
    on = eager & member[col]
    order = np.argsort(col[on], kind="stable")
    eu, ev = src[on][order], col[on][order]
    starts = np.flatnonzero(np.r_[True, ev[1:] != ev[:-1]]) if len(ev) else np.zeros(0, dtype=np.int64)
    depth = np.full((K, n), -1, dtype=np.int64)
    depth[np.arange(K), sources] = 0
    front, level = depth == 0, 0
    while len(ev) and front.any():
        level += 1
        arrive = np.zeros((K, n), dtype=bool)
        arrive[:, ev[starts]] = np.logical_or.reduceat(front[:, eu], starts, axis=1)
        front = arrive & (depth < 0)
        depth[front] = level
    return depth


def reach(rowptr, col, mesh, fanout, subs, T, sources, include=None, routers=None):
    """dict of reached, unreached, ecc int64 [K, T], depth_hist int64 [K, T, 64]
    and depths uint8 [K, N, T] by the header's definitions."""
    n, K = len(rowptr) - 1, len(sources)
    mem = members(subs, T, include, routers)
    both = np.asarray(mesh, dtype=np.uint64) | np.asarray(fanout, dtype=np.uint64)
    src, col = np.repeat(np.arange(n), np.diff(rowptr)), np.asarray(col, dtype=np.int64)
    sources = np.asarray(sources, dtype=np.int64)
    out = {f: np.zeros((K, T), dtype=np.int64) for f in FIELDS}
    out["depth_hist"] = np.zeros((K, T, DEPTH_BINS), dtype=np.int64)
    out["depths"] = np.full((K, n, T), 255, dtype=np.uint8)
    for t in range(T):
        m = mem[:, t]
        all_d = depths_from(src, col, ((both >> np.uint64(t)) & np.uint64(1)) != 0, m, sources)
        got = all_d > 0  # (the source's own depth is 0: no target)
        out["reached"][:, t] = got.sum(axis=1)
        out["unreached"][:, t] = m.sum() - m[sources] - got.sum(axis=1)
        out["ecc"][:, t] = all_d.max(axis=1)
        k_of, _ = np.nonzero(got)
        out["depth_hist"][:, t] = np.bincount(k_of * DEPTH_BINS + np.minimum(all_d[got], DEPTH_BINS - 1),
                                              minlength=K * DEPTH_BINS).reshape(K, DEPTH_BINS)
        out["depths"][:, :, t] = np.where(all_d < 0, 255, np.minimum(all_d, 254))
    return out


def of_engine(e, sources, include=None, hop=None):
    """reach() of an engine's (or the oracle's) state as it stands."""
    return reach(e.rowptr, e.col, e.mesh(), e.fanout(), mhref.subs_at(e.subs, e.events, e.hop if hop is None else hop),
                 e.T, sources, include, e.routers)


def sources_of(e, mask, count=NUM_SOURCES, seed=5):
    """`count` distinct hosts: a random one first (the run with one source), then
    a host of the smallest and one of the largest degree, a host outside the
    mask if there is one, and random ones."""
    deg = np.diff(e.rowptr)
    first = np.random.default_rng(seed).permutation(e.N).tolist()
    picked = [first[0], int(np.argmin(deg)), int(np.argmax(deg))]
    if mask is not None and not np.asarray(mask).all():
        picked.append(int(np.flatnonzero(~np.asarray(mask, dtype=bool))[0]))
    out = list(dict.fromkeys(picked + first))[:count]
    return np.array(out, dtype=np.int32)


class Ref:
    """An oracle run read every PERIOD hops: rows[k] (reach() without the
    depths) of tick k over SOURCES, the last tick's depths, the final snapshot."""

    def __init__(self, oracle, name, key):
        e, hops = scenarios.SCENARIOS[name](oracle)
        self.name, self.hops, self.N, self.T = name, hops, e.N, e.T
        self.mask = mask_of(e, key)
        self.sources = sources_of(e, self.mask)
        self.degree = np.diff(e.rowptr)
        self.ticks = hops // PERIOD
        self.rows, self.depths = [], None
        for _ in range(self.ticks):
            e.step(PERIOD)
            row = of_engine(e, self.sources, self.mask)
            self.depths = row.pop("depths")
            self.rows.append(row)
        e.step(hops - self.ticks * PERIOD)
        self.final = scenarios.snapshot(e, getattr(e, "snapshot_ids", range(e.n_published)))
        e.close()
        for row in self.rows:
            for a in row.values():
                a.setflags(write=False)
        self.depths.setflags(write=False)
        self.sources.setflags(write=False)

    def hop(self, k):
        return (k + 1) * PERIOD

    def series(self, field):
        """int64 [ticks, K, T]"""
        return np.stack([row[field] for row in self.rows])


@functools.lru_cache(maxsize=None)
def ref(oracle, name, key=None):
    """The oracle's run of a CASES scenario (shared, read only)."""
    return Ref(oracle, name, key)


# ---------------------------------------------------------------- the ring of the closed form
# mesh_health_ref.ring_engine: n hosts on a cycle, every host's mesh its two
# neighbours; the connections (0, 1) and (n / 2, n / 2 + 1) close at hop 25,
# which leaves host 0 at one end of the arc n / 2 + 1 .. n - 1, 0.
def ring_want(k, n=mhref.RING_N):
    """(reached, unreached, ecc, depth_hist [64], depths [n]) from source 0 of
    any topic at tick k."""
    depth = np.full(n, -1, dtype=np.int64)
    depth[0] = 0
    if (k + 1) * PERIOD < mhref.RING_CUT_HOP:  # two hosts at each depth 1 .. n / 2 - 1, one at n / 2
        for v in range(1, n):
            depth[v] = min(v, n - v)
    else:  # n - 1, n - 2, ... at depths 1, 2, ...
        for v in range(n // 2 + 1, n):
            depth[v] = n - v
    got = depth > 0
    hist = np.bincount(np.minimum(depth[got], DEPTH_BINS - 1), minlength=DEPTH_BINS)
    table = np.where(depth < 0, 255, np.minimum(depth, 254)).astype(np.uint8)
    return int(got.sum()), int(n - 1 - got.sum()), int(depth[got].max()), hist, table
