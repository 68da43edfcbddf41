"""Reference for the bandwidth statistics (include/gs_bandwidth.h), oracle only:
the scenario on the CPU oracle, stepped `period` hops at a time.  After each
piece rpc_bytes() is read; its per-edge differences, reduced with np.bincount
over the row owner (egress) and over col (ingress), are the tick's `all` bytes
and RPC counts.  The class split comes from the oracle's trace with every node
traced and rpc=True: a SEND_RPC block of hop h belongs to tick h // period; its
MSG items are `eager` when the block has no CTL item and `pulled` when it has
one, field(msg_size[topic]) each; overhead is what is left.  (Control sizes
are not recomputed from the items: only the MSG items are needed.)  The rows
are binned with numpy exactly as the header defines them."""
import functools

import numpy as np

import inspect_ref
import scenarios
from pubsub_amd import WithEventTracer, WithRPCAccounting, _abi, default_bandwidth_bounds

_T = _abi.TRACE_TYPES.index
RECV, SEND, ITEM = _T("RECV_RPC"), _T("SEND_RPC"), _abi.GS_TRACE_RPC_ITEM
ALL, EAGER, PULLED, OVERHEAD = range(4)
EGRESS, INGRESS = 0, 1

# the scenarios compared tick for tick, classes included: period in hops
PERIOD = {
    "acct_ladder_multitopic": 7,
    "acct_multitopic": 10,
    "acct_churn": 10,
    "acct_adversarial": 10,
    "acct_floodsub": 10,
    "acct_randomsub": 10,
    "acct_mixed_px": 10,
    "acct_odd_203": 5,
    "acct_floodsub_1gib": 10,
}
CASES = ["acct_ladder_multitopic", "acct_multitopic", "acct_churn", "acct_adversarial", "acct_floodsub",
         "acct_randomsub", "acct_mixed_px"]
BIG, BIG_PERIOD = "acct_big_20011", 5
GIB_BOUNDS = [1, 1 << 32, 1 << 34, 1 << 36, 1 << 38, 1 << 39, 1 << 40, 1 << 41, 1 << 42, 1 << 44]
LOCAL = {
    # N = 203 fills no last pass of four nodes per workgroup (every acct scenario has N divisible by 4)
    "acct_odd_203": lambda lib, x=(): scenarios.gossipsub_scored(lib, n=203, k=8, topics=2, msgs=40,
                                                                 extra=(scenarios._acct(2),) + tuple(x)),
    # more nodes than one pass of k_bw_tick's capped grid covers (8 workgroups per CU x 4 nodes: 8192 on 256 CUs)
    BIG: lambda lib, x=(): scenarios.gossipsub_scored(lib, n=20011, k=6, topics=2, msgs=40,
                                                      extra=(scenarios._acct(2),) + tuple(x)),
    # per-node bytes per period far above 2^32
    "acct_floodsub_1gib": lambda lib, x=(): scenarios.floodsub_dense(
        lib, extra=(WithRPCAccounting(1 << 30, id_len=30),) + tuple(x)),
}


def builder(name):
    return LOCAL[name] if name in LOCAL else scenarios.SCENARIOS[name]


def msg_sizes(name, T):
    return [1 << 30] * T if name == "acct_floodsub_1gib" else [120 + 5 * t for t in range(T)]  # scenarios._acct


def pb_field(n):
    """gs_pb_field: a length-delimited field of n bytes with a one-byte tag."""
    v, k = n, 1
    while v >= 0x80:
        v >>= 7
        k += 1
    return 1 + k + n


def per_node(rowptr, col, edge_values):
    """int64 [2, N]: an int64 per-edge array summed over each node's out-edges
    (egress) and over the edges that point at it (ingress)."""
    n = len(rowptr) - 1
    src = np.repeat(np.arange(n), np.diff(rowptr))
    out = np.zeros((2, n), dtype=np.int64)
    np.add.at(out[EGRESS], src, edge_values)
    np.add.at(out[INGRESS], col, edge_values)
    return out


def message_bytes(ev, msgf, period, ticks, n):
    """int64 [ticks, 2 (eager, pulled), 2 (egress, ingress), N] from trace
    events: the MSG items of the SEND_RPC blocks, binned by the block's hop;
    and int64 [ticks], the SEND_RPC blocks per tick (every RPC but the hello
    packets, which are not traced)."""
    out = np.zeros((ticks, 2, 2, n), dtype=np.int64)
    typ = ev["type"]
    head = (typ == SEND) | (typ == RECV)
    hidx = np.flatnonzero(head)
    if not len(hidx):
        return out, np.zeros(ticks, dtype=np.int64)
    sent = ev["hop"][typ == SEND] // period
    sends = np.bincount(sent[sent < ticks], minlength=ticks).astype(np.int64)
    blk = np.cumsum(head) - 1
    item = typ == ITEM
    assert not item[:hidx[0]].any(), "an RPC item without its RPC event"
    has_ctl = np.zeros(len(hidx), dtype=bool)
    has_ctl[blk[item & (ev["reason"] == _abi.GS_RPC_ITEM_CTL)]] = True
    m = np.flatnonzero(item & (ev["reason"] == _abi.GS_RPC_ITEM_MSG))
    mb = blk[m]
    hd = ev[hidx[mb]]
    tick = hd["hop"] // period
    keep = (hd["type"] == SEND) & (tick < ticks)
    m, mb, hd, tick = m[keep], mb[keep], hd[keep], tick[keep]
    size = np.asarray(msgf, dtype=np.int64)[ev["topic"][m]]
    cls = has_ctl[mb].astype(np.int64)
    np.add.at(out, (tick, cls, EGRESS, hd["node"]), size)
    np.add.at(out, (tick, cls, INGRESS, hd["peer"]), size)
    return out, sends


def row_of(values, rpcs, bounds):
    """The row of a tick from values int64 [2, 4, N] and rpcs int64 [2, N]."""
    nb = len(bounds)
    hist = np.zeros((2, 4, nb + 1), dtype=np.int64)
    mx = np.zeros((2, 4), dtype=np.int64)
    arg = np.full((2, 4), -1, dtype=np.int64)
    for dr in range(2):
        for c in range(4):
            x = values[dr, c]
            hist[dr, c] = np.bincount(np.searchsorted(bounds, x, side="right"), minlength=nb + 1)
            mx[dr, c] = x.max()
            if mx[dr, c] > 0:
                arg[dr, c] = int(np.argmax(x))  # the first (lowest index) of the largest
    return dict(total=values[EGRESS].sum(axis=1), total_rpcs=int(rpcs[EGRESS].sum()), hist=hist, max=mx, argmax=arg)


def with_classes(all_bytes, split):
    """int64 [2, 4, N] from all int64 [2, N] and split int64 [2 (eager, pulled), 2, N]."""
    v = np.zeros((2, 4, all_bytes.shape[1]), dtype=np.int64)
    v[:, ALL] = all_bytes
    v[:, EAGER] = split[0]
    v[:, PULLED] = split[1]
    v[:, OVERHEAD] = all_bytes - split[0] - split[1]
    return v


class Ref:
    """An oracle run read every `period` hops: values[k] int64 [2, 4, N] and
    rpcs[k] int64 [2, N] of tick k; cum_bytes / cum_rpcs the cumulative per-edge
    readback at the last tick."""

    def __init__(self, oracle, name, classes=True, period=None):
        probe, _ = builder(name)(oracle)
        n = probe.N
        probe.close()
        extra = (WithEventTracer(np.ones(n, dtype=bool), rpc=True),) if classes else ()
        e, hops = builder(name)(oracle, extra)
        self.name, self.hops, self.period = name, hops, PERIOD[name] if period is None else period
        self.N, self.T, self.E = e.N, e.T, e.E
        self.rowptr, self.col = e.rowptr.copy(), e.col.copy()
        self.ticks = hops // self.period
        self.observers = inspect_ref.observers_of(self.rowptr)
        msgf = [pb_field(s) for s in msg_sizes(name, e.T)]
        pb, pn = np.zeros(e.E, dtype=np.int64), np.zeros(e.E, dtype=np.int64)
        all_bytes, self.rpcs = [], []
        split = np.zeros((self.ticks, 2, 2, n), dtype=np.int64)
        self.sends = np.zeros(self.ticks, dtype=np.int64)  # the traced RPCs per tick
        for _ in range(self.ticks):
            e.step(self.period)
            b, c = e.rpc_bytes()
            all_bytes.append(per_node(self.rowptr, self.col, b - pb))
            self.rpcs.append(per_node(self.rowptr, self.col, c - pn))
            pb, pn = b, c
            if classes:  # read until it is empty; binned by the events' hop, not by the read
                got = message_bytes(e.trace_events(), msgf, self.period, self.ticks, n)
                split += got[0]
                self.sends += got[1]
        self.cum_bytes, self.cum_rpcs = pb, pn
        e.close()
        self.classes = classes
        self.values = [with_classes(all_bytes[k], split[k]) for k in range(self.ticks)]
        self.bounds = self._bounds()
        for a in self.values + self.rpcs + [self.cum_bytes, self.cum_rpcs, self.bounds]:
            a.setflags(write=False)

    def _bounds(self):
        """The default bounds (for the 1 GiB messages: bounds above 2^32) and
        three bounds that equal per-node values that occur, the quartiles of the
        non-zero egress `all` values of the middle tick: the upper-bin rule, and
        more than two populated bins where every host sends about the same
        (floodsub, randomsub)."""
        base = GIB_BOUNDS if self.name == "acct_floodsub_1gib" else default_bandwidth_bounds()
        x = np.sort(self.values[self.ticks // 2][EGRESS, ALL])
        x = x[x > 0]
        self.exact_bounds = sorted({int(x[len(x) * q // 4]) for q in (1, 2, 3)})
        return np.array(sorted(set(base) | set(self.exact_bounds)), dtype=np.int64)

    def hop(self, k):
        return (k + 1) * self.period

    def row(self, k):
        return row_of(self.values[k], self.rpcs[k], self.bounds)

    def sampled(self, k):
        """(bytes [nS, 2, 4], rpcs [nS, 2]) of the observers."""
        obs = np.array(self.observers)
        return (np.ascontiguousarray(self.values[k][:, :, obs].transpose(2, 0, 1)),
                np.ascontiguousarray(self.rpcs[k][:, obs].T))


@functools.lru_cache(maxsize=None)
def ref(oracle, name, classes=True, period=None):
    """The oracle's run of a scenario (shared, read only)."""
    return Ref(oracle, name, classes, period)


ROW = ("total", "total_rpcs", "hist", "max", "argmax")


def differences(got, want, k, fields=ROW):
    return [f"tick {k}: {f} {np.asarray(got[f]).tolist()} != {np.asarray(want[f]).tolist()}" for f in fields
            if not np.array_equal(got[f], want[f])]
