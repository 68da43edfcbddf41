"""Reference for the latency statistics (include/gs_latency.h): the same
scenario on the CPU oracle, whose per-message deliveries (every scenario sets
WithRecordDeliveries) are binned by age.  The oracle keeps a message's
deliveries after its slot is used again, so one reading at the end of the run
gives the whole-run reference, slot reuse included."""
import functools

import numpy as np

import scenarios

# scenario: (nodes, topics, first deliveries, largest age), measured on the
# oracle; tests/test_latency.py holds the oracle to them.  The window families
# (scenarios.WINDOW_FAMILIES, their _edge members) reach the last bin and use
# slots again exactly retireHops after their first use.
TABLE = {
    "gossipsub_dense": (20, 1, 1900, 2),
    "gossipsub_multitopic": (200, 3, 33108, 4),
    "floodsub_multitopic": (300, 3, 40915, 6),
    "randomsub_100": (200, 1, 11940, 4),
    "squatters": (50, 1, 49000, 2),
    "adversarial_mix": (400, 1, 106970, 62),
    "ladder_64t": (160, 64, 93101, 7),
    "win_flood": (69, 1, 9112, 48),
    "win_flood_3t": (68, 3, 23182, 48),
    "win_randomsub": (70, 1, 9246, 48),
    "win_gossip": (52, 1, 7548, 30),
    "win_gossip_4t": (51, 4, 29600, 30),
}
WINDOWS = [s for s in TABLE if s in scenarios.WINDOW_FAMILIES]


def builder(name):
    """(lib, extra) -> (engine, hops) of a TABLE scenario."""
    if name in scenarios.WINDOW_FAMILIES:
        return scenarios._win(name)
    return scenarios.SCENARIOS[name]


class Ref:
    """An oracle run: age[message, node] of every first delivery (delivery
    hop - publish hop), -1 for the author and for hosts never reached."""

    def __init__(self, oracle, name):
        e, hops = builder(name)(oracle)
        e.step(hops)
        self.hops, self.N, self.T = hops, e.N, e.T
        self.msg_topic, self.msg_hop = e.msg_topic.copy(), e.msg_hop.copy()
        self.counters = e.counters()
        ids = np.arange(e.n_published)
        self.hop = np.stack([e.deliveries(i)[0] for i in ids]).astype(np.int64)
        self.age = np.where(self.hop >= 0, self.hop - self.msg_hop[:, None], -1)
        self.age[ids, e.msg_src] = -1
        self.live_ids = list(getattr(e, "snapshot_ids", ids))
        e.close()
        self.age.setflags(write=False)
        self.hop.setflags(write=False)

    @property
    def max_age(self):
        return int(self.age.max())

    def _taken(self, nodes, from_hop):
        n0, n1 = nodes if nodes is not None else (0, self.N)
        m = self.age >= 0
        m[:, :n0] = False
        m[:, n1:] = False
        return m & (self.hop >= from_hop)

    def hist(self, bins, nodes=None, from_hop=0):
        """int64 [T, bins]: first deliveries by topic and age, of the hosts
        [nodes[0], nodes[1]) at hop from_hop or later."""
        m = self._taken(nodes, from_hop)
        key = (self.msg_topic[:, None].astype(np.int64) * bins + self.age)[m]
        return np.bincount(key, minlength=self.T * bins).reshape(self.T, bins).astype(np.int64)

    def message_rows(self, ids, bins, nodes=None):
        """uint32 [len(ids), bins]: first deliveries of each message by age."""
        m = self._taken(nodes, 0)
        return np.stack([np.bincount(self.age[i][m[i]], minlength=bins) for i in ids]).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def ref(oracle, name):
    """The oracle's run of a TABLE scenario (shared, read only)."""
    return Ref(oracle, name)
