"""Per-hop runs of the P6 scenarios (scenarios.P6) and the count of "sibling"
score changes in them: changes of a score that nothing but a recount of the
IP colocation factor can explain.

An edge's score changes as a sibling at hop h if, between the snapshots after
hops h - 1 and h, its own behaviour penalty and every topic's fmd, mmd, mfp,
imd, flags and mesh time are unchanged, no connection event touches the edge's
own connection at hops h - 1, h or h + 1, and the score is non-zero before and
after (an edge without a record scores 0).  The snapshot after hop h is the
state once hop h has run: its events, its refresh (hops 10, 20, ...) and its
heartbeat."""
import functools

import numpy as np

import scenarios

REFRESH = 10  # hops per DecayInterval
OWN_STATE = ("ts_fmd", "ts_mmd", "ts_mfp", "ts_imd", "ts_flags", "ts_mesh_time")


def hop_snaps(lib, name, extra=()):
    """(engine facts, [snapshot after hop 0, 1, ...]); deliveries only in the last."""
    e, hops = scenarios.SCENARIOS[name](lib, extra)
    ids = list(getattr(e, "snapshot_ids", range(e.n_published)))
    snaps = []
    for h in range(hops):
        e.step(1)
        snaps.append(scenarios.snapshot(e, ids if h == hops - 1 else []))
    facts = dict(rowptr=e.rowptr, col=e.col, N=e.N, T=e.T, E=e.E, n_published=e.n_published,
                 conn_events=list(getattr(e, "conn_events", ())), flip_edges=getattr(e, "flip_edges", None),
                 flip_hop=getattr(e, "flip_hop", None))
    e.close()
    return facts, snaps


@functools.lru_cache(maxsize=None)
def oracle_snaps(oracle, name):
    return hop_snaps(oracle, name)


def first_difference(ref, got):
    """None, or "hop h: <what differs>" for the first hop whose snapshots differ."""
    if len(ref) != len(got):
        return f"{len(ref)} hops vs {len(got)}"
    for h, (a, b) in enumerate(zip(ref, got)):
        bad = scenarios.compare(a, b)
        if bad:
            return f"hop {h}: " + "; ".join(bad)
    return None


def sibling_changes(facts, snaps):
    """[(hop, edge, score before, score after)] by the definition above."""
    src = np.repeat(np.arange(facts["N"]), np.diff(facts["rowptr"]))
    col = facts["col"]
    busy = {}
    for h, a, b in facts["conn_events"]:
        for d in (-1, 0, 1):
            busy.setdefault(h + d, set()).update({(a, b), (b, a)})
    out = []
    for h in range(1, len(snaps)):
        p, q = snaps[h - 1], snaps[h]
        sp, sq = np.asarray(p["scores"]), np.asarray(q["scores"])
        cand = (sp != sq) & (sp != 0) & (sq != 0) & (np.asarray(p["bp"]) == np.asarray(q["bp"]))
        for k in OWN_STATE:
            cand &= (np.asarray(p[k]) == np.asarray(q[k])).all(axis=0)
        hot = busy.get(h, ())
        for e in np.flatnonzero(cand):
            if (int(src[e]), int(col[e])) not in hot:
                out.append((h, int(e), float(sp[e]), float(sq[e])))
    return out


def crossings(changes, thr, refresh, fall=True):
    """The sibling changes that cross `thr` (fall: from >= thr to < thr, else
    the other way) at refresh hops / at the other hops."""
    return [c for c in changes
            if ((c[0] % REFRESH == 0) == refresh) and ((c[2] >= thr > c[3]) if fall else (c[2] < thr <= c[3]))]


def delivered(facts, snap):
    """Deliveries in a final snapshot: (node, message) pairs with a delivery hop."""
    return int(sum((np.asarray(h) >= 0).sum() for h, _ in snap["deliv"]))


def overflow_prunes(facts, snaps, D=6, t=0):
    """[(heartbeat hop, node)] where the heartbeat found more than Dhi mesh
    members.  GRAFTs are taken in during the heartbeat's own hop, so the
    overflow is in no snapshot; what shows is its pruning: across the hop the
    node loses a member whom it scores >= 0 afterwards and whose connection
    no event touched (so neither the prune of negative scores nor a
    disconnect explains the loss; a peer's own PRUNE arrives the hop after a
    heartbeat or a Join, never at a heartbeat hop of a run without Joins) and
    is left with exactly D."""
    src = np.repeat(np.arange(facts["N"]), np.diff(facts["rowptr"]))
    col = facts["col"]
    busy = {}
    for h, a, b in facts["conn_events"]:
        for d in (-1, 0, 1):
            busy.setdefault(h + d, set()).update({(a, b), (b, a)})
    out = []
    for h in range(1, len(snaps)):
        if snaps[h]["counters"]["heartbeats"] == snaps[h - 1]["counters"]["heartbeats"]:
            continue
        was = ((np.asarray(snaps[h - 1]["mesh"]) >> np.uint64(t)) & np.uint64(1)).astype(bool)
        now = ((np.asarray(snaps[h]["mesh"]) >> np.uint64(t)) & np.uint64(1)).astype(bool)
        lost = was & ~now & (np.asarray(snaps[h]["scores"]) >= 0)
        hot = busy.get(h, ())
        for e in np.flatnonzero(lost):
            if (int(src[e]), int(col[e])) in hot:
                lost[e] = False
        n_lost = np.bincount(src, weights=lost, minlength=facts["N"])
        n_now = np.bincount(src, weights=now, minlength=facts["N"])
        out += [(h, int(u)) for u in np.flatnonzero((n_lost >= 1) & (n_now == D))]
    return out


def mesh_medians(facts, snap, t=0):
    """Per node with at least two mesh members of topic t: the score the
    reference's opportunistic grafting calls the median (gossipsub.go:1455-1470:
    ascending, index len / 2)."""
    m = ((np.asarray(snap["mesh"]) >> np.uint64(t)) & np.uint64(1)).astype(bool)
    sc = np.asarray(snap["scores"])
    out = {}
    for u in range(facts["N"]):
        b, f = int(facts["rowptr"][u]), int(facts["rowptr"][u + 1])
        s = np.sort(sc[b:f][m[b:f]])
        if len(s) > 1:
            out[u] = float(s[len(s) // 2])
    return out
