"""Reference for mesh health (include/gs_mesh_health.h): the definitions of the
header in numpy over rowptr, col, a mesh readback, the include mask, the
routers and the subscription words -- the initial subscriptions plus the
scheduled JOIN / LEAVE events up to the tick.  It reads nothing but what the
oracle's or the engine's existing readbacks return.

Components by union to the smaller label with path halving, on whole arrays:
every mutual edge lowers its source's label to its target's, then every label
to its label's label, until nothing changes; the fixed point is the smallest
node id of the component.

Ref runs a scenario on the CPU oracle stepped `PERIOD` hops at a time (a tick
per heartbeat) and keeps every tick's rows, the last tick's labels and the
final snapshot."""
import functools

import numpy as np

import scenarios
from pubsub_amd import GS_EV_JOIN, GS_EV_LEAVE, GS_ROUTER_GOSSIPSUB, GS_ROUTER_GOSSIPSUB_V10

FIELDS = ("members", "components", "largest", "isolated", "one_sided", "outside", "eclipsed")
SIZE_BINS = 32
PERIOD = 10  # HeartbeatInterval 1 s over hops of 100 ms
# (scenario, mask): the scenarios of tests/test_mesh_health_gpu.py
CASES = [("ladder_64t_sub", None), ("ladder_multitopic", None), ("adversarial_mix", None),
         ("adversarial_mix", "honest"), ("squatters", "honest"), ("churn_scored", None), ("mixed_scored", None),
         ("c4shape", None)]


def subs_at(subs, events, hop):
    """The hosts' subscription words when the hop counter is `hop`: the events
    of the hops <= hop - 1 have been applied, each hop's leaves before its joins."""
    out = np.array(subs, dtype=np.uint64)
    evs = [(h, 0 if kind == GS_EV_LEAVE else 1, a, b) for h, kind, a, b in events
           if kind in (GS_EV_LEAVE, GS_EV_JOIN) and h <= hop - 1]
    for _, join, a, b in sorted(evs, key=lambda x: (x[0], x[1])):
        bit = np.uint64(1) << np.uint64(b)
        out[a] = (out[a] | bit) if join else (out[a] & ~bit)
    return out


def reverse_edges(rowptr, col):
    n = len(rowptr) - 1
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    key = src * n + col  # ascending: rows in order, columns sorted within a row
    assert (np.diff(key) > 0).all()
    return src, np.searchsorted(key, col.astype(np.int64) * n + src)


def health(rowptr, col, mesh, subs, T, include=None, routers=None):
    """dict of the seven int64 [T] counts, comp_hist int64 [T, 32] and labels
    int32 [N, T] (-1: not a member) by the header's definitions."""
    n = len(rowptr) - 1
    src, rev = reverse_edges(rowptr, col)
    inc = np.ones(n, dtype=bool) if include is None else np.asarray(include) != 0
    gossip = np.ones(n, dtype=bool)
    if routers is not None:
        gossip = (np.asarray(routers) == GS_ROUTER_GOSSIPSUB) | (np.asarray(routers) == GS_ROUTER_GOSSIPSUB_V10)
    out = {f: np.zeros(T, dtype=np.int64) for f in FIELDS}
    out["comp_hist"] = np.zeros((T, SIZE_BINS), dtype=np.int64)
    out["labels"] = np.full((n, T), -1, dtype=np.int32)
    ids = np.arange(n, dtype=np.int64)
    for t in range(T):
        member = inc & gossip & (((subs >> np.uint64(t)) & np.uint64(1)) != 0)
        bit = ((mesh >> np.uint64(t)) & np.uint64(1)) != 0
        mutual = bit & bit[rev] & member[src] & member[col]
        u, v = src[mutual], col[mutual].astype(np.int64)
        lab = ids.copy()
        while True:
            new = lab.copy()
            np.minimum.at(new, u, lab[v])
            new = new[new]
            if np.array_equal(new, lab):
                break
            lab = new
        sizes = np.bincount(lab[member], minlength=n)
        comp = sizes[sizes > 0]
        has_mutual = np.zeros(n, dtype=bool)
        has_mutual[u] = True
        out["members"][t] = member.sum()
        out["components"][t] = len(comp)
        out["largest"][t] = comp.max() if len(comp) else 0
        out["isolated"][t] = (member & ~has_mutual).sum()
        assert out["isolated"][t] == (comp == 1).sum()
        mine = bit & member[src]
        out["one_sided"][t] = (mine & inc[col] & ~bit[rev]).sum()
        out["outside"][t] = (mine & ~inc[col]).sum()
        slots = np.bincount(src[mine], minlength=n)
        inside = np.bincount(src[mine & inc[col]], minlength=n)
        out["eclipsed"][t] = (member & (slots > 0) & (inside == 0)).sum()
        if len(comp):
            out["comp_hist"][t] = np.bincount(np.floor(np.log2(comp)).astype(np.int64), minlength=SIZE_BINS)
        out["labels"][member, t] = lab[member]
    return out


def of_engine(e, include=None, hop=None):
    """health() of an engine's (or the oracle's) state as it stands."""
    return health(e.rowptr, e.col, e.mesh(), subs_at(e.subs, e.events, e.hop if hop is None else hop), e.T,
                  include, e.routers)


def mask_of(e, key):
    if key is None:
        return None
    assert key == "honest"
    return ~e.sybil if hasattr(e, "sybil") else np.arange(e.N) < e.honest


class Ref:
    """An oracle run read every PERIOD hops: rows[k] (health() without the
    labels) of tick k, the last tick's labels, the final snapshot."""

    def __init__(self, oracle, name, key):
        e, hops = scenarios.SCENARIOS[name](oracle)
        self.name, self.hops, self.N, self.T = name, hops, e.N, e.T
        self.mask = mask_of(e, key)
        self.ticks = hops // PERIOD
        self.rows, self.labels = [], None
        for _ in range(self.ticks):
            e.step(PERIOD)
            row = of_engine(e, self.mask)
            self.labels = row.pop("labels")
            self.rows.append(row)
        e.step(hops - self.ticks * PERIOD)
        self.final = scenarios.snapshot(e, getattr(e, "snapshot_ids", range(e.n_published)))
        e.close()
        for row in self.rows:
            for a in row.values():
                a.setflags(write=False)
        self.labels.setflags(write=False)

    def hop(self, k):
        return (k + 1) * PERIOD

    def series(self, field):
        """int64 [ticks, T]"""
        return np.stack([row[field] for row in self.rows])


@functools.lru_cache(maxsize=None)
def ref(oracle, name, key=None):
    """The oracle's run of a CASES scenario (shared, read only)."""
    return Ref(oracle, name, key)


# ---------------------------------------------------------------- the ring of the closed form
RING_N, RING_HOPS, RING_CUT_HOP = 200, 50, 25


def ring_engine(lib, extra=(), topics=2, n=RING_N):
    """n hosts on a cycle, every topic subscribed, default gossipsub params,
    hops of 100 ms; the connections (0, 1) and (n / 2, n / 2 + 1) close at hop
    25, which leaves the arcs 1 .. n / 2 and n / 2 + 1 .. n - 1, 0."""
    from pubsub_amd import GS_EV_DISCONNECT, NewGossipSub, WithHop, WithMessageWindow, graphs
    pairs = np.array([(i, (i + 1) % n) for i in range(n)], dtype=np.int64)
    e = NewGossipSub(n, topics, graphs._to_csr(n, pairs), graphs.all_subscribed(n, topics), WithHop(scenarios.HOP),
                     WithMessageWindow(64), *extra, lib=lib)
    e.schedule_events([GS_EV_DISCONNECT] * 2, [0, n // 2], [1, n // 2 + 1], [RING_CUT_HOP] * 2)
    return e


def ring_want(k, n=RING_N):
    """(members, components, largest, isolated, one_sided) of either topic at tick k."""
    return (n, 1, n, 0, 0) if (k + 1) * PERIOD < RING_CUT_HOP else (n, 2, n // 2, 0, 0)


def ring_labels(topics=2, n=RING_N):
    lab = np.zeros(n, dtype=np.int32)
    lab[1:n // 2 + 1] = 1
    return np.repeat(lab[:, None], topics, axis=1)
