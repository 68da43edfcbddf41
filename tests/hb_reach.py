"""Which steps of the heartbeat's mesh maintenance (gossipsub.go:1331-1503) a
scenario reaches, counted on a traced run stepped hop by hop.

The heartbeat is the last thing in its hop, and an (edge, topic) is grafted or
pruned at most once in it (a pruned peer is in backoff, a Dlo graft fills a
mesh to D <= Dhi only), so with G and P the peers of the heartbeat's Graft and
Prune trace events (phase 4) of host u and topic t at hop h, and `post` the
mesh in the snapshot after h, the heartbeat entered the topic with
pre = (post - G) | P.  K = pre - P are the members it kept.  A step is counted
only on a condition that is sufficient for it:

  neg_prune   P is not empty and |pre| <= Dhi: no Dhi prune is possible (the
              Dlo graft stops at D), and an honest host prunes for nothing else.
  dlo_graft   |pre| <= Dhi (so all of P left for their score, before the Dlo
              test), |pre| - |P| < Dlo and G is not empty.  An opportunistic
              graft's candidates score above a median >= 0, so they are Dlo
              candidates too: the Dlo step took some of G.
  dhi_prune   a pruned peer whom u scores >= 0 after the hop and whom u
              grafted in no topic in this heartbeat.  A prune never raises the
              score (it removes P1 >= 0, and swaps P3 for P3b of the same
              deficit: check_weights), so the peer scored >= 0 going in and
              did not leave for its score.
  dhi_keep    a dhi_prune of which every pruned peer is of that kind (so the
              ranked list is `pre`), with a kept outbound peer q that the
              ranking alone puts at position >= D: at least Dscore members
              score above q (by u's score after the hop, which is exact for
              a peer the heartbeat did not touch and a lower bound for a
              pruned one), so q is in the shuffled tail, and at least D
              members precede q in the tail's shuffle (GS_SITE_DHI_TAIL keys;
              at most Dscore of them are not in the tail).  q stayed, so fewer
              than Dout outbound peers were among the first D and the
              outbound-keep (gossipsub.go:1389-1429) moved q up.
  dout_graft  |K| >= Dlo (no Dlo graft), G is not empty, and the tick is no
              opportunistic one: every graft is the Dout step's.
  opp_graft   an opportunistic tick, |K| >= Dlo and G holds a peer the Dout
              step cannot take: one that is not outbound, or any once K has
              Dout outbound members.
  refresh     P is not empty and u received a message of t one or two
              heartbeat intervals back, which is in its gossip windows
              (HistoryGossip >= 3): emitGossip(t) runs, and the pruned peers
              (topic peers outside the mesh now, never direct) are candidates
              whose live score it computes after the prune.
"""
import collections

import numpy as np

import scenarios
from pubsub_amd import WithEventTracer, _abi

STEPS = ("neg_prune", "dlo_graft", "dhi_prune", "dhi_keep", "dout_graft", "opp_graft", "refresh")
GRAFT, PRUNE = _abi.TRACE_TYPES.index("GRAFT"), _abi.TRACE_TYPES.index("PRUNE")
SITE_DHI_TAIL = 9  # include/gs_rng.h


def check_weights(score_params):
    for tp in score_params.Topics.values():
        assert tp.TopicWeight >= 0 and tp.TimeInMeshWeight >= 0
        assert tp.MeshFailurePenaltyWeight <= tp.MeshMessageDeliveriesWeight <= 0


def reach(lib, olib, name, graph, gp, seed):
    """{step: number of heartbeats in which some host certainly took it} for
    scenario `name` on `lib`; graph, gp (GossipSubParams) and seed are the
    scenario's own (the graph is checked against the engine's)."""
    rowptr, col, outbound = graph
    N = len(rowptr) - 1
    e, hops = scenarios.SCENARIOS[name](lib, (WithEventTracer(np.arange(N)),))
    assert np.array_equal(e.rowptr, rowptr) and np.array_equal(e.col, col)
    check_weights(e.score_params)
    assert gp.HistoryGossip >= 3
    mesh, score, tick, ev = [], [], [], []
    for _ in range(hops):
        e.step(1)
        mesh.append(e.mesh())
        score.append(e.scores())
        tick.append(e.counters()["heartbeats"])
        x = e.trace_events()
        ev.append(x[(x["phase"] == 4) & ((x["type"] == GRAFT) | (x["type"] == PRUNE))])
    ev = np.concatenate(ev)
    ids = list(getattr(e, "snapshot_ids", range(e.n_published)))
    topic_of = getattr(e, "sched_top", np.zeros(e.n_published, np.int32))
    got = collections.defaultdict(set)  # (host, topic) -> hops at which the host got a message of the topic
    for i in ids:
        hop_of, _ = e.deliveries(i)
        for u in np.flatnonzero(hop_of >= 0):
            got[(int(u), int(topic_of[i]))].add(int(hop_of[u]))
    e.close()

    hb = [h for h in range(1, hops) if tick[h] != tick[h - 1]]
    every = hb[1] - hb[0]
    changed = collections.defaultdict(lambda: (set(), set()))  # (hop, host, topic) -> (grafted, pruned) edges
    for x in ev:
        u, p = int(x["node"]), int(x["peer"])
        edge = int(rowptr[u] + np.searchsorted(col[rowptr[u]:rowptr[u + 1]], p))
        assert col[edge] == p
        changed[(int(x["hop"]), u, int(x["topic"]))][0 if x["type"] == GRAFT else 1].add(edge)
    grafted = collections.defaultdict(set)  # (hop, host) -> edges grafted in any topic
    touched = collections.defaultdict(set)  # (hop, host) -> edges grafted or pruned in any topic
    for (h, u, _), (G, P) in changed.items():
        grafted[(h, u)] |= G
        touched[(h, u)] |= G | P

    out = {s: set() for s in STEPS}
    for (h, u, t), (G, P) in changed.items():
        assert h in hb and not (G & P)
        row = np.arange(rowptr[u], rowptr[u + 1])
        post = {int(x) for x in row[(mesh[h][row] >> np.uint64(t)) & np.uint64(1) == 1]}
        assert G <= post and not (P & post)
        pre = (post - G) | P
        K = pre - P
        S = score[h]
        ob = lambda edges: sum(int(outbound[x]) for x in edges)
        opp_tick = tick[h] % gp.OpportunisticGraftTicks == 0
        if P and len(pre) <= gp.Dhi:
            out["neg_prune"].add(h)
            if len(K) < gp.Dlo and G:
                out["dlo_graft"].add(h)
        by_rank = {p for p in P if S[p] >= 0 and p not in grafted[(h, u)]}
        if by_rank:
            out["dhi_prune"].add(h)
        if by_rank and by_rank == P and len(K) == gp.D:
            lower = {m: (S[m] if m in P or m not in touched[(h, u)] else -np.inf) for m in pre}
            k2 = {m: olib.orng_key64(seed, SITE_DHI_TAIL, u, h & 0xFFFFFFFF, int(col[m]), t) for m in pre}
            for q in K:
                if outbound[q] and q not in touched[(h, u)] \
                        and sum(lower[m] > S[q] for m in pre if m != q) >= gp.Dscore \
                        and sum((k2[m], m) < (k2[q], q) for m in pre if m != q) >= gp.D:
                    out["dhi_keep"].add(h)
        if G and len(K) >= gp.Dlo:
            if not opp_tick:
                assert ob(K) < gp.Dout and all(outbound[g] for g in G)
                out["dout_graft"].add(h)
            elif ob(K) >= gp.Dout or not all(outbound[g] for g in G):
                out["opp_graft"].add(h)
        if P and any(h - 2 * every <= d <= h - 1 for d in got[(u, t)]):
            out["refresh"].add(h)
    return {s: len(v) for s, v in out.items()}
