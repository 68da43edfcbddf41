"""The two workloads of the per-topic message windows (include/gs_window.h),
shared by tests/test_topic_windows.py (their preconditions on the oracle) and
tests/test_topic_windows_gpu.py:

- tw_sparse(tail): a topic with few subscribers beside one everybody takes.
  window_engine's body of 24 nodes subscribes to topics 0 and 1, the tail of
  `tail` nodes hung on body node 0 to topic 1 only, so topic 0 is delivered
  within 2 hops and topic 1 walks the tail hop by hop (age tail + 2).
- tw_hot: one hot topic among 64 (1904 messages on topic 0 within 100 hops, at
  most 14 on any other), which no uniform layout within 16384 slots holds.
"""
import functools

import numpy as np

import latency_ref
import scenarios
from pubsub_amd import (NewGossipSub, Second, WithHop, WithMessageWindow, WithPeerScore, WithRecordDeliveries,
                        WithSeed, eth2_peer_score_params, eth2_thresholds, graphs)

SPARSE_START, SPARSE_COUNT, SPARSE_SEED = 25, 120, 101
# (tail: largest first-delivery age of topic 0, of topic 1), measured on the oracle
SPARSE_AGES = {28: (2, 30), 29: (2, 31), 45: (2, 47)}
HOT = dict(n=200, k=12, topics=64, seed=7, msgs=2400, hb=12, topic0_frac=0.8)
HOT_SLOTS = [2048] + [64] * 63
HOT_TOPIC0, HOT_OTHERS, HOT_MAX_AGE, HOT_DELIVERIES = 1904, 14, 4, 477600


def sparse_network(lib, tail, slots=128, extra=()):
    """tw_sparse's network, nothing published: Eth2 scoring with the mesh
    delivery penalties starting after the run (window_engine's p3_after)."""
    g = graphs.tailed(scenarios.WIN_BODY, 12, tail, SPARSE_SEED)
    n = scenarios.WIN_BODY + tail
    subs = np.full(n, 3, np.uint64)
    subs[scenarios.WIN_BODY:] = 2
    sp = eth2_peer_score_params(2)
    for tp in sp.Topics.values():
        tp.MeshMessageDeliveriesActivation = 60 * Second
    e = NewGossipSub(n, 2, g, subs, WithRecordDeliveries(), WithSeed(SPARSE_SEED), WithMessageWindow(slots),
                     WithPeerScore(sp, eth2_thresholds()), WithHop(scenarios.HOP), *extra, lib=lib)
    e.tip = n - 1
    return e


def tw_sparse(lib, tail, extra=(), slots=128):
    """(engine, hops): from hop 25, for 120 hops, one message per hop on topic
    0 by the body author and one on topic 1 by the body author and the tail's
    tip in turn; run until the last message has crossed the tail."""
    e = sparse_network(lib, tail, slots, extra)
    src, top, hops = [], [], []
    for i in range(SPARSE_COUNT):
        src += [scenarios.WIN_AUTHOR, e.tip if i % 2 else scenarios.WIN_AUTHOR]
        top += [0, 1]
        hops += [SPARSE_START + i] * 2
    src, top, hops = np.array(src, np.int32), np.array(top, np.int32), np.array(hops, np.int64)
    e.publish(src, top, hops)
    e.sched_src, e.sched_top, e.sched_hops = src, top, hops
    return e, int(hops[-1]) + tail + 12


def tw_hot(lib, extra=(), window=256):
    """(engine, hops); window: gs_config.slots_per_topic (64 x 256 is the
    largest uniform layout; the rings proper come through `extra`)."""
    return scenarios.gossipsub_scored(lib, window=window, extra=extra, **HOT)


class Ran:
    """An oracle run: hop[message, node] of every first delivery (-1: none; the
    author's own entry is its publish) and age = hop - publish hop."""

    def __init__(self, e, hops):
        e.step(hops)
        self.e, self.hops = e, hops
        self.top = e.sched_top
        self.hop = np.stack([e.deliveries(i)[0] for i in range(e.n_published)]).astype(np.int64)
        self.age = np.where(self.hop >= 0, self.hop - e.sched_hops[:, None], -1)
        self.counters = e.counters()
        self.hop.setflags(write=False)
        self.age.setflags(write=False)

    def max_age(self, t):
        return int(self.age[self.top == t].max())

    def first_hop_over(self, t, age):
        """The first hop with a first delivery of topic t older than `age`."""
        m = (self.age > age) & (self.top == t)[:, None]
        return int(self.hop[m].min())

    def all_delivered(self):
        want = ((self.e.subs[None, :] >> self.top[:, None].astype(np.uint64)) & np.uint64(1)) != 0
        return bool((self.hop[want] >= 0).all())


@functools.lru_cache(maxsize=None)
def sparse_ran(oracle, tail):
    return Ran(*tw_sparse(oracle, tail))


@functools.lru_cache(maxsize=None)
def hot_ran(oracle):
    return Ran(*tw_hot(oracle, window=2048))  # (the oracle has no window: any value)


@functools.lru_cache(maxsize=None)
def sparse_snap(oracle, tail):
    """The oracle's snapshot of tw_sparse(tail) (shared, read only)."""
    r = sparse_ran(oracle, tail)
    return scenarios.snapshot(r.e, range(r.e.n_published))


class SparseRef(latency_ref.Ref):
    """latency_ref.Ref of tw_sparse(tail) (not a registered scenario)."""

    def __init__(self, oracle, tail):  # pylint: disable=super-init-not-called
        r = sparse_ran(oracle, tail)
        e = r.e
        self.hops, self.N, self.T = r.hops, e.N, e.T
        self.msg_topic, self.msg_hop = e.msg_topic.copy(), e.msg_hop.copy()
        self.counters = r.counters
        ids = np.arange(e.n_published)
        self.hop = r.hop
        self.age = r.age.copy()
        self.age[ids, e.msg_src] = -1
        self.live_ids = list(ids)
        self.age.setflags(write=False)
