"""What the P6 scenarios (scenarios.P6) are there for, pinned on the oracle: a
recount of the IP colocation factor moves the scores of the other peers on the
IP ("siblings", tests/p6_check.py) across the thresholds the engine's score
memos are kept against, at refresh hops and between them.  A change of seed
that empties one of these counts would leave tests/test_p6_gpu.py comparing
runs in which P6 never matters."""
import numpy as np
import pytest

import p6_check
import scenarios
from pubsub_amd import eth2_thresholds
from pubsub_amd.params import GossipSubParams
from score_check import oracle_scores, sample_edges

THR = eth2_thresholds()
CHURN = ["p6_churn_heavy", "p6_churn_light", "p6_churn_light_wl", "p6_churn_2t", "p6_expiry_flip", "p6_connect_flip",
         "p6_dhi", "ladder_p6_churn"]


def _changes(oracle_path, name):
    facts, snaps = p6_check.oracle_snaps(oracle_path, name)
    ch = p6_check.sibling_changes(facts, snaps)
    print(name, "sibling changes:", len(ch))
    return facts, snaps, ch


def test_every_scenario_is_registered():
    assert set(CHURN) | {"p6_static_dense", "p6_static_whitelist"} == set(scenarios.P6)
    assert all(scenarios.SCENARIOS[k] is v for k, v in scenarios.P6.items())


@pytest.mark.parametrize("name", CHURN)
def test_deliveries_survive_the_churn(oracle_path, name):
    """More than 95 % of (node, message) pairs are delivered (the ladder holds
    two isolated nodes of 160)."""
    facts, snaps = p6_check.oracle_snaps(oracle_path, name)
    got, want = p6_check.delivered(facts, snaps[-1]), facts["N"] * facts["n_published"]
    print(name, "deliveries", got, "of", want)
    assert got > 0.95 * want


@pytest.mark.parametrize("name", ["p6_churn_heavy", "p6_churn_2t"])
def test_heavy_falls_cross_every_threshold_between_refreshes(oracle_path, name):
    _, _, ch = _changes(oracle_path, name)
    for thr in (0.0, THR.GossipThreshold, THR.PublishThreshold, THR.GraylistThreshold):
        n = len(p6_check.crossings(ch, thr, refresh=False))
        print(name, "falls across", thr, "at non-refresh hops:", n)
        assert n >= 1
    falls = [c for c in ch if c[3] < c[2]]
    assert {c[0] % p6_check.REFRESH for c in falls} == set(range(p6_check.REFRESH))  # at every hop phase


@pytest.mark.parametrize("name", ["p6_churn_light", "p6_churn_light_wl", "p6_dhi", "ladder_p6_churn"])
def test_light_signs_flip_between_refreshes(oracle_path, name):
    _, _, ch = _changes(oracle_path, name)
    falls = len(p6_check.crossings(ch, 0.0, refresh=False))
    rises = len(p6_check.crossings(ch, 0.0, refresh=False, fall=False))
    print(name, ">= 0 -> < 0 at non-refresh hops:", falls, "; < 0 -> >= 0:", rises)
    assert falls >= 1 and rises >= 1


@pytest.mark.parametrize("name", ["p6_churn_heavy", "p6_churn_light", "p6_churn_2t"])
def test_expired_records_raise_siblings_at_refresh_hops(oracle_path, name):
    _, _, ch = _changes(oracle_path, name)
    rises = [c for c in ch if c[0] % p6_check.REFRESH == 0 and c[3] > c[2]]
    print(name, "rises at refresh hops:", len(rises))
    assert len(rises) >= 1


def test_expiry_flip_on_the_named_edges(oracle_path):
    """The siblings fall below 0 when Y connects (hop 33, no refresh, no
    heartbeat), are back at >= 0 after hop 40, whose refresh is the first past
    the retained record's expiry (disconnect at hop 25 + RetainScore 1 s) and
    whose heartbeat must not prune them, and stay in the mesh throughout."""
    facts, snaps = p6_check.oracle_snaps(oracle_path, "p6_expiry_flip")
    assert facts["flip_hop"] == 40 and facts["flip_hop"] % p6_check.REFRESH == 0
    assert [h for h, _, _ in facts["conn_events"]] == [25, 33]
    assert 30 * scenarios.HOP <= 25 * scenarios.HOP + scenarios.Second < 40 * scenarios.HOP
    hb = [h for h in range(1, len(snaps)) if snaps[h]["counters"]["heartbeats"] != snaps[h - 1]["counters"]["heartbeats"]]
    assert 40 in hb and not any(33 <= h < 40 for h in hb)
    for e in facts["flip_edges"]:
        s = [float(snap["scores"][e]) for snap in snaps]
        assert all(x > 0 for x in s[:33]) and all(x < 0 for x in s[33:40]) and all(x > 0 for x in s[40:50]), s[20:50]
        assert all(int(snap["mesh"][e]) & 1 for snap in snaps[:60])


def test_connect_flip_on_the_named_edges(oracle_path):
    """The mirror: the siblings fall below 0 at the hop of a fresh connect that
    is a heartbeat hop and no refresh hop, and that heartbeat prunes them."""
    facts, snaps = p6_check.oracle_snaps(oracle_path, "p6_connect_flip")
    h = facts["flip_hop"]
    assert h % p6_check.REFRESH != 0 and [x[0] for x in facts["conn_events"]] == [h]
    assert snaps[h]["counters"]["heartbeats"] == snaps[h - 1]["counters"]["heartbeats"] + 1
    for e in facts["flip_edges"]:
        assert snaps[h - 1]["scores"][e] > 0 > snaps[h]["scores"][e]
        assert int(snaps[h - 1]["mesh"][e]) & 1 and not int(snaps[h]["mesh"][e]) & 1


def test_static_dense_p6_on_most_observers(oracle_path, olib):
    """Recomputed without the IPs, the final scores of most observers' edges
    differ from the simulator's; with them they are the simulator's."""
    e, hops = scenarios.SCENARIOS["p6_static_dense"](oracle_path)
    e.step(hops)
    obs = np.arange(0, e.N, 8)
    edges = np.concatenate([np.arange(e.rowptr[u], e.rowptr[u + 1]) for u in obs])
    want = e.scores()[edges]
    with_ip, _ = oracle_scores(olib, e.score_params, e, edges, app=e.app_attr, ipv4=e.ipv4_attr)
    assert np.array_equal(with_ip.view(np.uint64), want.view(np.uint64))
    plain, _ = oracle_scores(olib, e.score_params, e, edges, app=e.app_attr)
    rows = np.searchsorted(e.rowptr, edges, side="right") - 1
    hit = np.unique(rows[plain != want])
    print("observers with a non-zero P6:", len(hit), "of", len(obs))
    assert len(hit) > len(obs) // 2


def test_static_whitelist_moves_only_the_whitelisted_ip(oracle_path, olib):
    a, hops = scenarios.SCENARIOS["p6_static_dense"](oracle_path)
    b, _ = scenarios.SCENARIOS["p6_static_whitelist"](oracle_path)
    assert np.array_equal(a.ipv4_attr, b.ipv4_attr)
    (net, mask), = scenarios._P6_WL
    listed = (b.ipv4_attr[b.col] & mask) == (net & mask)
    assert listed.any() and not listed.all()
    # after the first hop (Join only) the two runs differ by P6 alone
    a.step(1)
    b.step(1)
    diff = a.scores() != b.scores()
    assert diff.any() and not (diff & ~listed).any()
    # at the end the runs have gone apart; the whitelisted run's own state,
    # scored without the whitelist, differs from its scores only on listed edges
    b.step(hops - 1)
    edges = sample_edges(b.E, 300, 1, must=[0, b.E - 1])
    unlisted, _ = oracle_scores(olib, b.score_params, b, edges, app=b.app_attr, ipv4=b.ipv4_attr)
    diff = unlisted != b.scores()[edges]
    assert diff.any() and not (diff & ~listed[edges]).any()


def test_dhi_meshes_overflow_and_opportunistic_grafting_runs(oracle_path):
    """Some heartbeat after the first connection event (so with P6 moving)
    finds a mesh of more than Dhi peers and prunes it to D by the Dhi ranking,
    and going into some opportunistic-graft tick (every third heartbeat) a
    mesh's median score is below OpportunisticGraftThreshold."""
    facts, snaps = p6_check.oracle_snaps(oracle_path, "p6_dhi")
    hb = [h for h in range(1, len(snaps)) if snaps[h]["counters"]["heartbeats"] != snaps[h - 1]["counters"]["heartbeats"]]
    first_event = min(h for h, _, _ in facts["conn_events"])
    over = [h for h, _ in p6_check.overflow_prunes(facts, snaps, D=GossipSubParams().D) if h > first_event]
    og = [h for h in hb if snaps[h]["counters"]["heartbeats"] % 3 == 0]
    low = [h for h in og if min(p6_check.mesh_medians(facts, snaps[h - 1]).values()) < THR.OpportunisticGraftThreshold]
    print("heartbeats entered with a mesh over Dhi:", len(over), "; graft ticks with a low median:", len(low), "of", len(og))
    assert over and low
