"""Preconditions of the message-window edge scenarios (scenarios.WINDOW_EDGE /
WINDOW_OVER), on the oracle alone.  The engine's seen-set is a fixed window of
message slots with two limits the reference and the oracle do not have
(window() below); the scenarios are worth something only while the oracle's
largest first-delivery age is exactly maxAge (the `_edge` members, which the
engine must reproduce bit for bit) or exactly maxAge + 1 (the `_over` members,
which it must refuse), and while a slot is used again exactly retireHops after
its earlier use.  A change to a graph builder or a schedule that moves either
fails here, not silently on the GPU."""
import functools
import json
import os

import numpy as np
import pytest

import scenarios
from pubsub_amd import graphs
from pubsub_amd.params import GossipSubParams

HERE = os.path.dirname(os.path.abspath(__file__))
FAMILIES = sorted(scenarios.WINDOW_FAMILIES)
# the families whose rings wrap (64 topics x 256 slots at one message per hop
# over all topics would need 64 x 256 hops)
WRAPPING = [f for f in FAMILIES if f != "win_gossip_64t"]
# tails one inside and two past the limit (the GPU tests run them too)
NEAR = ["win_flood", "win_gossip"]


def window(router="gossipsub", params=None, hop_ns=scenarios.HOP, long=False):
    """(maxAge, retireHops) in hops: gs_engine::setWindow(), csrc/gs_engine.h:475.
    long: the adversarial model is on (a validator, the gater, behaviours) or
    connection / subscription events were scheduled before the first publish."""
    gp = params or GossipSubParams()
    gossip = router == "gossipsub"
    H = gp.HeartbeatInterval // hop_ns if gossip else 16  # a nominal 16 for floodsub / randomsub
    max_age = (gp.HistoryLength + gp.HistoryGossip + 3 if long else 3) * H
    return max_age, max_age + ((gp.HistoryLength + 2) * H if gossip else 2)


def family_window(fam):
    kw = scenarios.WINDOW_FAMILIES[fam]
    return window(kw.get("router", "gossipsub"), scenarios._win_params(kw.get("hist")),
                  long=bool(kw.get("validate")) or kw.get("event_at") is not None)


def builder(fam, d=0):
    """The family's run with a tail `d` nodes longer than its _edge member's."""
    return scenarios._win(fam, d)


class Ran:
    """An oracle run of a window scenario: first-delivery hops of every
    message, [message, node], -1 where never delivered."""

    def __init__(self, oracle, fam, d):
        e, hops = builder(fam, d)(oracle)
        e.step(hops)
        self.e, self.hops = e, hops
        self.hop = np.stack([e.deliveries(i)[0] for i in range(e.n_published)]).astype(np.int64)
        self.age = np.where(self.hop >= 0, self.hop - e.sched_hops[:, None], -1)
        self.counters = e.counters()

    @property
    def max_age(self):
        return int(self.age.max())

    def first_hop_of_age(self, age):
        return int(self.hop[self.age == age].min())


@functools.lru_cache(maxsize=None)
def ran(oracle, fam, d=0):
    return Ran(oracle, fam, d)


def first_over_hop(oracle, fam, d=1):
    """The first hop at which the oracle makes a first delivery older than
    the family's maxAge, in the run whose tail is d nodes past the _edge one."""
    r = ran(oracle, fam, d)
    return int(r.hop[r.age > family_window(fam)[0]].min())


# ---------------------------------------------------------------- the builder
def test_tailed_builder():
    nb, k, tail = 24, 6, 9
    rowptr, col, outbound = graphs.tailed(nb, k, tail, 5)
    n = nb + tail
    deg = np.diff(rowptr)
    assert len(rowptr) == n + 1 and len(col) == len(outbound) == rowptr[-1]
    src = np.repeat(np.arange(n), deg)
    und = {(int(u), int(v)): int(o) for u, v, o in zip(src, col, outbound)}
    # symmetric, rows strictly ascending, no self loops, one dialer per pair
    assert len(und) == len(col) and all(u != v for u, v in und)
    assert all(und[(v, u)] == 1 - o for (u, v), o in und.items())
    assert all(np.all(np.diff(col[rowptr[u]:rowptr[u + 1]]) > 0) for u in range(n))
    # the tail: degree 2 along it, 1 at the tip, hung on body node 0
    assert (deg[nb:n - 1] == 2).all() and deg[n - 1] == 1
    assert col[rowptr[nb]:rowptr[nb + 1]].tolist() == [0, nb + 1]
    assert all(col[rowptr[u]:rowptr[u + 1]].tolist() == [u - 1, u + 1] for u in range(nb + 1, n - 1))
    assert col[rowptr[n - 1]] == n - 2
    # the body is random_regular's, edges and dialers, with the one tail edge on node 0
    br, bc, bo = graphs.random_regular(nb, k, 5)
    assert deg[0] == br[1] - br[0] + 1 and np.array_equal(deg[1:nb], np.diff(br)[1:])
    for u in range(nb):
        keep = col[rowptr[u]:rowptr[u + 1]] < nb
        assert np.array_equal(col[rowptr[u]:rowptr[u + 1]][keep], bc[br[u]:br[u + 1]])
        assert np.array_equal(outbound[rowptr[u]:rowptr[u + 1]][keep], bo[br[u]:br[u + 1]])
    # same seed, same graph; a longer tail keeps the shorter one's dialers; another seed differs
    again = graphs.tailed(nb, k, tail, 5)
    assert all(np.array_equal(a, b) for a, b in zip((rowptr, col, outbound), again))
    longer = graphs.tailed(nb, k, tail + 1, 5)
    assert np.array_equal(longer[2][:rowptr[n - 1]], outbound[:rowptr[n - 1]])
    assert not np.array_equal(col, graphs.tailed(nb, k, tail, 6)[1])
    with pytest.raises(ValueError, match="at least one node"):
        graphs.tailed(nb, k, 0, 5)


# ---------------------------------------------------------------- the schedules
@pytest.mark.parametrize("fam", FAMILIES)
def test_schedule_sits_on_the_publish_guard(fam):
    """`reuse` is the formula's retireHops, `slots` the smallest multiple of 64
    that holds it (64 topics: the layout's 256), every hop of at least
    maxAge + 70 has a message by the body author or the tip in turn, and a slot
    is used again exactly retireHops after its earlier use, never sooner."""
    kw = scenarios.WINDOW_FAMILIES[fam]
    max_age, retire = family_window(fam)
    assert kw["reuse"] == retire
    assert kw["slots"] == (256 if kw["topics"] == 64 else -(-retire // 64) * 64)
    assert kw["count"] >= max_age + 70 and kw["tail"] + scenarios.WIN_BODY < 200
    src, top, hops = scenarios.window_schedule(**kw)
    tip = scenarios.WIN_BODY + kw["tail"] - 1
    assert set(src.tolist()) == {scenarios.WIN_AUTHOR, tip}
    assert set(np.unique(hops).tolist()) == set(range(kw["start"], kw["start"] + kw["count"]))
    dist = []
    for t in range(kw["topics"]):
        h = hops[top == t]
        dist += (h[kw["slots"]:] - h[:len(h) - kw["slots"]]).tolist()
    if fam in WRAPPING:
        assert dist and min(dist) == retire
    else:
        assert not dist


@pytest.mark.parametrize("fam", FAMILIES)
def test_young_and_old_slots_share_words(fam):
    """At some hop a 64-bit word of the seen-set holds a slot whose message is
    young (age <= maxAge) beside one whose message is older, and (more than
    one word per topic, one message per hop and topic) a topic's young slots
    lie in two words."""
    kw = scenarios.WINDOW_FAMILIES[fam]
    max_age, _ = family_window(fam)
    _, top, hops = scenarios.window_schedule(**kw)
    slot = np.zeros(len(hops), np.int64)
    for t in range(kw["topics"]):
        idx = np.flatnonzero(top == t)
        slot[idx] = t * kw["slots"] + np.arange(len(idx)) % kw["slots"]
    mixed = straddle = False
    for h in range(int(hops[0]), int(hops[-1]) + 1):
        owner = {}
        for i in np.flatnonzero(hops <= h):  # (the latest message of every slot)
            owner[int(slot[i])] = int(hops[i])
        young = {s for s, p in owner.items() if h - p <= max_age}
        old = set(owner) - young
        mixed |= bool({s >> 6 for s in young} & {s >> 6 for s in old})
        straddle |= any(len({s >> 6 for s in young if s // kw["slots"] == t}) > 1 for t in range(kw["topics"]))
    assert mixed
    assert straddle == (kw["slots"] > 64 and not kw.get("shared"))


# ---------------------------------------------------------------- at the limit
@pytest.mark.parametrize("fam", FAMILIES)
def test_edge_member_reaches_max_age_exactly(oracle_path, fam):
    r = ran(oracle_path, fam)
    max_age, _ = family_window(fam)
    print(fam, "tail", scenarios.WINDOW_FAMILIES[fam]["tail"], "N", r.e.N, "hops", r.hops, "oracle max age", r.max_age)
    assert r.max_age == max_age
    # every subscribed node receives every message
    want = ((r.e.subs[None, :] >> r.e.sched_top[:, None].astype(np.uint64)) & np.uint64(1)) != 0
    assert (r.hop[want] >= 0).all()
    # some hop has first deliveries of age maxAge and of age 1 together
    at_edge = set(r.hop[r.age == max_age].tolist())
    assert at_edge & set(r.hop[r.age == 1].tolist())
    # the readable messages (slots not used again) include one of age maxAge
    assert (r.age[r.e.snapshot_ids] == max_age).any()


@pytest.mark.parametrize("fam", FAMILIES)
def test_over_member_is_one_hop_past(oracle_path, fam):
    r = ran(oracle_path, fam, 1)
    max_age, _ = family_window(fam)
    assert r.max_age == max_age + 1
    first = first_over_hop(oracle_path, fam)
    print(fam, "first delivery of age", max_age + 1, "at hop", first)
    assert first == r.first_hop_of_age(max_age + 1) and first > max_age + 1


@pytest.mark.parametrize("fam", NEAR)
def test_one_inside_and_two_past(oracle_path, fam):
    max_age, _ = family_window(fam)
    assert ran(oracle_path, fam, -1).max_age == max_age - 1
    r = ran(oracle_path, fam, 2)
    assert r.max_age == max_age + 2
    # the first over-age delivery is one of age maxAge + 1, a hop before any of maxAge + 2
    assert first_over_hop(oracle_path, fam, 2) == r.first_hop_of_age(max_age + 1) < r.first_hop_of_age(max_age + 2)


@pytest.mark.parametrize("fam", [f for f in FAMILIES
                                 if scenarios.WINDOW_FAMILIES[f].get("router", "gossipsub") == "gossipsub"])
def test_gossip_is_live(oracle_path, fam):
    """The body's degree is above Dhi's reach of the mesh: IHAVE and IWANT
    run beside the eager push."""
    c = ran(oracle_path, fam).counters
    assert c["ihave_sent"] > 0 and c["iwant_served"] > 0


def test_the_long_window_is_what_the_option_alone_buys():
    """win_events is win_gossip's network and traffic with one scheduled
    event; win_adv the same with a validator."""
    honest = window()
    assert family_window("win_gossip") == honest
    assert family_window("win_events") == family_window("win_adv") == window(long=True) != honest
    assert family_window("win_gossip_h7")[1] < honest[1]


def test_edge_members_are_registered_with_goldens():
    golden = json.load(open(os.path.join(HERE, "golden", "scenarios.json")))
    for fam in FAMILIES:
        assert fam + "_edge" in scenarios.SCENARIOS and fam + "_edge" in golden
        assert fam + "_over" not in scenarios.SCENARIOS and fam + "_over" in scenarios.WINDOW_OVER
