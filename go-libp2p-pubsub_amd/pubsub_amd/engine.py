"""Host-side mirror of the reference's router selection over the C-ABI.

The reference builds one PubSub per host with NewFloodSub / NewRandomSub /
NewGossipSub plus Options (pubsub.go:221, floodsub.go:25, randomsub.go:21,
gossipsub.go:198-391).  This engine is one batched instance for N simulated
hosts; the constructors below take the same parameter structs and options:

    eng = NewGossipSub(n, topics, graph, WithGossipSubParams(p),
                       WithPeerScore(score_params, thresholds), WithFloodPublish(True))

The product path loads ONLY the HIP library (libgossip_engine.so, built for
gfx950) and raises if it is missing: there is no CPU fallback.  Tests pass an
explicit `lib=` to drive the CPU oracle through the identical ABI.
"""
import ctypes as C
import os
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np

from . import _abi
from .params import GossipSubParams, Millisecond

_HERE = os.path.dirname(os.path.abspath(__file__))
PRODUCT_LIB = os.path.join(os.path.dirname(_HERE), "build", "libgossip_engine.so")

_lib_cache = {}


def load(path=None):
    """Bind the ABI on `path` (default: the HIP product library)."""
    path = os.path.abspath(path or PRODUCT_LIB)
    if path not in _lib_cache:
        _lib_cache[path] = _abi.bind(path)
    return _lib_cache[path]


class GossipEngineError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"gossip engine error {code}: {msg}")
        self.code = code


def _check(lib, rc):
    if rc != _abi.GS_OK:
        raise GossipEngineError(rc, lib.gs_last_error().decode(errors="replace"))
    return rc


def _ptr(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype)) if a is not None else None


# ---------------------------------------------------------------- options
def WithGossipSubParams(cfg):
    return ("gossipsub_params", cfg)


def WithPeerScore(params, thresholds):
    return ("peer_score", (params, thresholds))


def WithFloodPublish(flood):
    return ("flood_publish", bool(flood))


def WithPeerExchange(do_px=True):
    """WithPeerExchange (gossipsub.go:320): PRUNEs carry peer suggestions and a
    pruned host dials them (needs connection slots: WithDormant)."""
    return ("px", bool(do_px))


def WithDormant(pairs):
    """Connections (a, b) of the graph that start down (gs_set_dormant): slots
    a peer-exchange dial or a GS_EV_CONNECT event can bring up."""
    return ("dormant", [(int(a), int(b)) for a, b in pairs])


def WithDirectPeers(direct_edges):
    """direct_edges: uint8[E] flags in CSR order (WithDirectPeers, gossipsub.go:338)."""
    return ("direct", direct_edges)


def WithSeed(seed):
    return ("seed", int(seed))


def WithHop(hop_ns):
    return ("hop_ns", int(hop_ns))


def WithMessageWindow(slots_per_topic):
    return ("slots_per_topic", int(slots_per_topic))


def WithTopicWindows(slots=None, max_age_hops=None):
    """The message window per topic (include/gs_window.h): slots[t] is topic t's
    ring (a positive multiple of 64, default WithMessageWindow's value for every
    topic; at most 16384 in total) and max_age_hops[t] > 0 the age in hops up to
    which a first delivery of a message of topic t is accepted (0 or None: the
    engine's policy, 3 heartbeats for honest runs).  A hot topic among many
    takes a large ring and the others small ones; a sparsely subscribed topic
    takes a long age.  The CPU oracle has no window: there the option is
    accepted and does nothing.  Read with Engine.topic_windows()."""
    conv = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
    return ("topic_windows", (conv(slots), conv(max_age_hops)))


def WithRecordDeliveries(on=True):
    return ("record", bool(on))


def WithDevice(dev):
    return ("device", int(dev))


def WithRPCAccounting(msg_size, id_len=40, topic_len=None, peer_id_len=38, record_len=0):
    """Per-edge RPC byte accounting (gs_set_rpc_accounting, SURVEY.md §8(f)
    rank 3): every RPC a host sends is measured as RPC.Size() (gossipsub.go:
    1121-1137) with messages of topic t msg_size[t] bytes (a scalar: all
    topics), ids id_len bytes, topic names topic_len[t] bytes (default: the
    decimal index's length, as the trace encoder names topics), PX entries of
    a PRUNE PeerInfo{peer id of peer_id_len bytes, signed record of record_len
    bytes or none} (makePrune, gossipsub.go:1811-1836; gs_set_rpc_px_sizes).
    Read with Engine.rpc_bytes()."""
    return ("rpc_acct", (msg_size, int(id_len), topic_len, int(peer_id_len), int(record_len)))


def WithEventTracer(nodes, capacity=1 << 22, rpc=False):
    """EventTracer (pubsub.go:418, trace.go) for the hosts in `nodes` (indices
    or a bool mask): their PublishMessage / DeliverMessage / DuplicateMessage /
    AddPeer / Join / Graft / Prune events, and with rpc=True every RPC they
    send or receive (SendRPC / RecvRPC with the RPCMeta items), read with
    Engine.trace_events()."""
    return ("trace", (nodes, int(capacity), bool(rpc)))


def WithPeerGater(params):
    """WithPeerGater (peer_gater.go:164-191): random early drop of payload from
    peers with poor goodput while the validation queue is throttling."""
    return ("gater", params)


def WithValidation(topic_validators, queue_per_hop=0):
    """RegisterTopicValidator for the topics with topic_validators[t] true (the
    verdict is each message's `kind`, see Engine.publish), and the validation
    queue: at most queue_per_hop received messages enter validation per node
    per hop (0 = unlimited; WithValidateQueueSize, validation.go:236-241)."""
    return ("validation", (topic_validators, int(queue_per_hop)))


def WithBehaviour(bits):
    """Per-node attacker behaviours (uint8[N] of GS_BEHAVE_* bits)."""
    return ("behaviour", bits)


def WithRouters(routers):
    """The router each host runs (gs_set_routers): GS_ROUTER_FLOODSUB /
    RANDOMSUB / GOSSIPSUB / GOSSIPSUB_V10 per node -- a mixed network
    (TestMixedGossipsub, gossipsub_test.go:810-851)."""
    return ("routers", np.ascontiguousarray(routers, dtype=np.uint8))


def WithProtocols(proto):
    """The protocol.ID of every connection (GS_PROTO_* per CSR edge, the
    `proto` of PubSubRouter.AddPeer, pubsub.go:165); default: negotiated from
    the hosts' routers."""
    return ("protocols", np.ascontiguousarray(proto, dtype=np.uint8))


def WithIPWhitelist(nets):
    """PeerScoreParams.IPColocationFactorWhitelist (score_params.go:75, score.go:
    344-361) as (net, mask) pairs of uint32 (gs_set_ip_whitelist): a peer whose
    IPv4 address lies in one of the subnets takes no P6 penalty."""
    return ("ip_whitelist", [(int(n) & 0xFFFFFFFF, int(m) & 0xFFFFFFFF) for n, m in nets])


def WithPeertxCapacity(home_bits, overflow_bits):
    """mcache.peertx capacity (gs_set_peertx_capacity): 2^home_bits slots per
    node, and a per-rank overflow table of 2^overflow_bits entries for nodes
    whose own table is full.  A row must fit the device's LDS per workgroup
    (4 << home_bits bytes: 15 at most on an MI355X), else the first step fails
    with GS_ECAPACITY."""
    return ("peertx", (int(home_bits), int(overflow_bits)))


def WithFrontierLists():
    """Phase A reads the senders' per-copy frontier lists even where the engine
    would OR their frontier bitmaps (gs_set_frontier_mode GS_FRONTIER_LISTS):
    same results, the other kernel path (A/B runs and parity tests)."""
    return ("frontier_mode", 1)


def WithFrontierBitmaps():
    """Phase A ORs the senders' frontier bitmaps wherever the engine supports
    them (GS_FRONTIER_BITMAPS), also where the lists measured faster."""
    return ("frontier_mode", 2)


def WithLatencyStats():
    """Propagation-latency histograms counted on the device (include/
    gs_latency.h, product library only): first deliveries by age in hops, per
    topic and per message.  Read with Engine.latency_hist() and
    Engine.message_latency(); see latency_quantiles()."""
    return ("latency_stats", True)


def latency_quantiles(hist, qs):
    """Per row of `hist` (counts by age, [..., bins]) and per q in `qs`, the
    smallest age whose cumulative count reaches q x the row's total; -1 for an
    empty row.  q is taken as the decimal it is written as (0.95 = 95/100) and
    q x total is computed exactly, so a cumulative count equal to it counts as
    reached.  Returns int64 [..., len(qs)]."""
    hist = np.asarray(hist)
    cum = np.cumsum(hist.astype(np.int64), axis=-1)
    total = cum[..., -1]
    fr = [Fraction(str(q)) for q in qs]
    out = np.full(hist.shape[:-1] + (len(qs),), -1, dtype=np.int64)
    for idx in np.ndindex(total.shape):
        n = int(total[idx])
        if n == 0:
            continue
        for k, q in enumerate(fr):
            need = max(1, -((-q.numerator * n) // q.denominator))  # ceil(q n); q = 0: the first delivery
            out[idx + (k,)] = int(np.searchsorted(cum[idx], need, side="left"))
    return out


@dataclass
class TopicScoreSnapshot:
    """score.go:137-142."""
    TimeInMesh: int = 0
    FirstMessageDeliveries: float = 0.0
    MeshMessageDeliveries: float = 0.0
    InvalidMessageDeliveries: float = 0.0


@dataclass
class PeerScoreSnapshot:
    """score.go:128-135; Topics is keyed by topic index."""
    Score: float = 0.0
    Topics: dict = field(default_factory=dict)
    AppSpecificScore: float = 0.0
    IPColocationFactor: float = 0.0
    BehaviourPenalty: float = 0.0


def default_inspect_bounds(thresholds):
    """WithPeerScoreInspect's default bin bounds: the sorted distinct values of
    the Graylist-, Publish-, Gossip- and OpportunisticGraftThreshold, 0 and the
    smallest positive subnormal (so that "exactly 0" has a bin of its own)."""
    return sorted({float(thresholds.GraylistThreshold), float(thresholds.PublishThreshold),
                   float(thresholds.GossipThreshold), 0.0, 5e-324,
                   float(thresholds.OpportunisticGraftThreshold)})


def _checked_bounds(bounds):
    b = np.ascontiguousarray(bounds, dtype=np.float64).reshape(-1)
    if len(b) > _abi.GS_INSPECT_MAX_BOUNDS:
        raise ValueError(f"WithPeerScoreInspect: at most {_abi.GS_INSPECT_MAX_BOUNDS} bounds, got {len(b)}")
    if not np.isfinite(b).all() or not (np.diff(b) > 0).all():
        raise ValueError("WithPeerScoreInspect: bounds must be finite and strictly ascending")
    return b


def WithPeerScoreInspect(inspect, period, *, bounds=None, nodes=None, ticks=64, extended=False):
    """WithPeerScoreInspect / WithPeerScoreInspectExtended (score.go:120-175,
    438-491), taken on the device (include/gs_inspect.h, product library
    only).  Every `period` (ns, a positive multiple of the hop) the engine
    keeps, inside step() and without a synchronise, a histogram of all scores
    over `bounds` (default: default_inspect_bounds of the thresholds), the
    mesh-degree distribution per topic, and the scores of the peers of the
    observers in `nodes` (indices or a bool mask) -- with extended=True their
    PeerScoreSnapshot fields too -- in a ring of `ticks` ticks.  `inspect` is
    None or a callable: step() then runs in chunks of at most ticks x period
    and calls inspect(hop, scores) once per tick, in order, with scores =
    {observer: {peer: score}} (PeerScoreInspectFn) or, extended,
    {observer: {peer: PeerScoreSnapshot}}.  Read with Engine.inspect_row(),
    inspect_scores(), inspect_snapshot()."""
    if inspect is not None and not callable(inspect):
        raise ValueError("WithPeerScoreInspect: inspect must be None or a callable")
    if int(ticks) < 1:
        raise ValueError("WithPeerScoreInspect: ticks must be at least 1")
    if bounds is not None:
        bounds = _checked_bounds(bounds)
    return ("score_inspect", dict(inspect=inspect, period=int(period), bounds=bounds, nodes=nodes, ticks=int(ticks),
                                  extended=bool(extended)))


def _inspect_period_hops(period, hop_ns, what="WithPeerScoreInspect"):
    if period <= 0 or period % hop_ns:
        raise ValueError(f"{what}: period {period} ns must be a positive multiple of the hop ({hop_ns} ns)")
    return period // hop_ns


def WithMeshHealth(period, *, nodes=None, ticks=64, labels=False):
    """Mesh health (include/gs_mesh_health.h, product library only): every
    `period` (ns, a positive multiple of the hop) the engine counts, inside
    step(), each topic's mesh components over the mutual mesh edges of the
    hosts in `nodes` (a bool or byte mask over the hosts; None: all), and the
    one-sided, outside and eclipsed mesh entries, into a ring of `ticks` ticks;
    labels=True keeps the newest tick's component labels readable.  Read with
    Engine.mesh_health_row(), mesh_labels().  Not on a partitioned engine."""
    if int(ticks) < 1:
        raise ValueError("WithMeshHealth: ticks must be at least 1")
    return ("mesh_health", dict(period=int(period), nodes=nodes, ticks=int(ticks), labels=bool(labels)))


def WithMeshReach(period, sources, *, nodes=None, ticks=64, depths=False):
    """Mesh reach (include/gs_mesh_reach.h, product library only): every
    `period` (ns, a positive multiple of the hop) the engine searches, inside
    step(), breadth first from each host of `sources` (distinct host ids, at
    most 256) over every topic's eager-push edges (mesh | fanout) through the
    member hosts of `nodes` (a bool or byte mask over the hosts; None: all), and
    counts the targets reached, not reached, the largest depth and the targets
    per depth into a ring of `ticks` ticks; depths=True keeps the newest tick's
    depth per (source, host, topic) readable.  Read with Engine.mesh_reach_row(),
    mesh_reach_depths().  Not on a partitioned engine."""
    if int(ticks) < 1:
        raise ValueError("WithMeshReach: ticks must be at least 1")
    src = np.asarray(sources)
    if src.ndim != 1 or not 1 <= len(src) <= _abi.GS_REACH_MAX_SOURCES:
        raise ValueError(f"WithMeshReach: sources must be 1 .. {_abi.GS_REACH_MAX_SOURCES} host ids")
    if src.dtype.kind not in "iu":
        raise ValueError("WithMeshReach: sources must be host ids (integers)")
    if len(np.unique(src)) != len(src):
        raise ValueError("WithMeshReach: a source is given twice")
    return ("mesh_reach", dict(period=int(period), sources=src.astype(np.int64), nodes=nodes, ticks=int(ticks),
                               depths=bool(depths)))


def default_bandwidth_bounds():
    """WithBandwidthStats' default bin bounds in bytes: 1 (bin 0 holds the
    silent nodes), then the powers of 4 from 1 KiB to 16 GiB."""
    return [1] + [1 << s for s in range(10, 35, 2)]


def _checked_bandwidth_bounds(bounds):
    b = np.asarray(bounds)
    if b.ndim != 1 or (len(b) and b.dtype.kind not in "iu"):
        raise ValueError("WithBandwidthStats: bounds must be a list of byte counts (integers)")
    if len(b) > _abi.GS_BW_MAX_BOUNDS:
        raise ValueError(f"WithBandwidthStats: at most {_abi.GS_BW_MAX_BOUNDS} bounds, got {len(b)}")
    if len(b) and int(b.max()) >= 1 << 63:
        raise ValueError("WithBandwidthStats: bounds must fit 63 bits")
    b = np.ascontiguousarray(b, dtype=np.int64)
    if not (b > 0).all() or not (np.diff(b) > 0).all():
        raise ValueError("WithBandwidthStats: bounds must be positive and strictly ascending")
    return b


def WithBandwidthStats(period, *, bounds=None, nodes=None, ticks=64):
    """Bandwidth statistics (include/gs_bandwidth.h, product library only; needs
    WithRPCAccounting, in any order): every `period` (ns, a positive multiple
    of the hop) the engine reduces, inside step() and without a synchronise,
    the bytes every host sent (egress) and was sent (ingress) in the period,
    split into eager push, payload pulled through IWANT and overhead: their
    totals, histograms over `bounds` (byte counts; default:
    default_bandwidth_bounds()), the maxima and the hosts that attain them, and
    the exact values of the hosts in `nodes` (indices or a bool mask), into a
    ring of `ticks` ticks.  Read with Engine.bandwidth_row(),
    bandwidth_sampled(); see bandwidth_quantiles().  Not on a partitioned
    engine."""
    if int(ticks) < 1:
        raise ValueError("WithBandwidthStats: ticks must be at least 1")
    bounds = _checked_bandwidth_bounds(default_bandwidth_bounds() if bounds is None else bounds)
    return ("bandwidth", dict(period=int(period), bounds=bounds, nodes=nodes, ticks=int(ticks)))


def bandwidth_quantiles(hist_row, bounds, qs):
    """Per row of `hist_row` (hosts by their bytes over `bounds`, [..., len(bounds)
    + 1]) and per q in `qs`, the upper edge of the first bin whose cumulative
    count reaches q x the row's total: the smallest bound that the quantile lies
    below (bounds[0] = 1: a silent host).  -1 for an empty row, and when the
    quantile lies in the last, open bin.  q is taken as the decimal it is
    written as, as latency_quantiles does.  Returns int64 [..., len(qs)]."""
    b = np.asarray(bounds, dtype=np.int64)
    hist_row = np.asarray(hist_row)
    if hist_row.shape[-1] != len(b) + 1:
        raise ValueError(f"bandwidth_quantiles: a row needs len(bounds) + 1 = {len(b) + 1} bins")
    edge = np.concatenate([b, [-1]]).astype(np.int64)
    bins = latency_quantiles(hist_row, qs)
    return np.where(bins < 0, -1, edge[np.maximum(bins, 0)])


def WithPartition(rank, world, transport):
    """Simulate only this rank's node range; exchange RPCs with the other
    ranks through `transport` (a pubsub_amd.transport.TorchTransport) once per
    hop.  Every rank makes the same calls (graph, subscriptions, publishes)."""
    return ("partition", (int(rank), int(world), transport))


# The headers only the product library exports (include/gs_window.h, gs_latency.h,
# gs_inspect.h, gs_mesh_health.h, gs_mesh_reach.h, gs_bandwidth.h): their
# functions and how Engine._product names them when the library lacks them.
_PRODUCT_ONLY = {
    "windows": (_abi.WINDOW_FUNCTIONS, "topic windows (WithTopicWindows)"),
    "latency": (_abi.LATENCY_FUNCTIONS, "latency statistics (WithLatencyStats)"),
    "inspect": (_abi.INSPECT_FUNCTIONS, "score inspection (WithPeerScoreInspect)"),
    "mesh_health": (_abi.MESH_HEALTH_FUNCTIONS, "mesh health (WithMeshHealth)"),
    "mesh_reach": (_abi.MESH_REACH_FUNCTIONS, "mesh reach (WithMeshReach)"),
    "bandwidth": (_abi.BANDWIDTH_FUNCTIONS, "bandwidth statistics (WithBandwidthStats)"),
}


def _node_mask(nodes, num_nodes):
    """uint8 [num_nodes]: 1 at the hosts of `nodes` (indices or a bool mask); None for None."""
    if nodes is None:
        return None
    mask = np.zeros(num_nodes, dtype=np.uint8)
    nodes = np.asarray(nodes)
    mask[np.nonzero(nodes)[0] if nodes.dtype == bool else nodes.astype(np.int64)] = 1
    return mask


class Engine:
    """One batched simulation of N routers (see module docstring)."""

    def __init__(self, router, num_nodes, num_topics, graph, subscriptions, *options,
                 randomsub_size=0, app_score=None, ipv4=None, lib=None):
        self.lib = load(lib)
        opts = dict(options)
        gsp = opts.get("gossipsub_params") or GossipSubParams()
        score = opts.get("peer_score")
        cfg = _abi.ConfigC()
        cfg.router = router
        cfg.randomsub_size = randomsub_size
        cfg.num_nodes = num_nodes
        cfg.num_topics = num_topics
        cfg.slots_per_topic = opts.get("slots_per_topic", 1024)
        cfg.seed = opts.get("seed", 1)
        cfg.hop_ns = opts.get("hop_ns", 100 * Millisecond)
        insp = opts.get("score_inspect")
        if insp is not None:  # refused before anything is created
            insp = dict(insp, period_hops=_inspect_period_hops(insp["period"], cfg.hop_ns))
        mh = opts.get("mesh_health")
        if mh is not None:
            mh = dict(mh, period_hops=_inspect_period_hops(mh["period"], cfg.hop_ns, "WithMeshHealth"))
            if mh["nodes"] is not None and len(mh["nodes"]) != num_nodes:
                raise ValueError(f"WithMeshHealth: nodes needs one entry per host ({num_nodes}), got {len(mh['nodes'])}")
        mr = opts.get("mesh_reach")
        if mr is not None:
            mr = dict(mr, period_hops=_inspect_period_hops(mr["period"], cfg.hop_ns, "WithMeshReach"))
            if mr["nodes"] is not None and len(mr["nodes"]) != num_nodes:
                raise ValueError(f"WithMeshReach: nodes needs one entry per host ({num_nodes}), got {len(mr['nodes'])}")
            if mr["sources"].min() < 0 or mr["sources"].max() >= num_nodes:
                raise ValueError(f"WithMeshReach: a source is outside 0 .. {num_nodes - 1}")
        bw = opts.get("bandwidth")
        if bw is not None:
            bw = dict(bw, period_hops=_inspect_period_hops(bw["period"], cfg.hop_ns, "WithBandwidthStats"))
            if bw["nodes"] is not None:
                nodes = np.asarray(bw["nodes"])
                if nodes.dtype == bool and len(nodes) != num_nodes:
                    raise ValueError(f"WithBandwidthStats: a node mask needs one entry per host ({num_nodes}), "
                                     f"got {len(nodes)}")
                if nodes.dtype != bool and len(nodes) and (nodes.min() < 0 or nodes.max() >= num_nodes):
                    raise ValueError(f"WithBandwidthStats: a node is outside 0 .. {num_nodes - 1}")
        flags = 0
        if score is not None:
            flags |= _abi.GS_FLAG_SCORING
        if opts.get("flood_publish"):
            flags |= _abi.GS_FLAG_FLOOD_PUBLISH
        if opts.get("px"):
            flags |= _abi.GS_FLAG_PEER_EXCHANGE
        if opts.get("record"):
            flags |= _abi.GS_FLAG_RECORD_DELIVERIES
        cfg.flags = flags
        cfg.device = opts.get("device", 0)
        self.N, self.T = num_nodes, num_topics
        self.score_params = score[0] if score is not None else None
        gsp_c = gsp.to_c()
        psp_c = topics_c = scored_c = thr_c = None
        if score is not None:
            params, thresholds = score
            psp_c = params.to_c()
            topics_c, scored_c = params.topics_c(num_topics)
            thr_c = thresholds.to_c()
        h = C.c_void_p()
        _check(self.lib, self.lib.gs_engine_create(
            C.byref(cfg), C.byref(gsp_c),
            C.byref(psp_c) if psp_c is not None else None,
            topics_c, scored_c,
            C.byref(thr_c) if thr_c is not None else None,
            C.byref(opts["gater"].to_c()) if opts.get("gater") is not None else None, C.byref(h)))
        self.h = h
        self._has = {feature: self._bind(functions) for feature, (functions, _) in _PRODUCT_ONLY.items()}
        tw = opts.get("topic_windows")
        if tw is not None and self._has["windows"]:  # (the oracle has no window)
            for a, what in zip(tw, ("slots", "max_age_hops")):
                if a is not None and len(a) != num_topics:
                    self.close()
                    raise ValueError(f"WithTopicWindows: {what} needs one entry per topic ({num_topics}), got {len(a)}")
            _check(self.lib, self.lib.gs_set_topic_windows(h, _ptr(tw[0], C.c_int32), _ptr(tw[1], C.c_int32)))
        rowptr, col, outbound = graph
        self.rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
        self.col = np.ascontiguousarray(col, dtype=np.int32)
        self.E = int(self.rowptr[-1])
        ob = np.ascontiguousarray(outbound, dtype=np.uint8) if outbound is not None else None
        direct = opts.get("direct")
        direct = np.ascontiguousarray(direct, dtype=np.uint8) if direct is not None else None
        proto = opts.get("protocols")
        if proto is None:
            _check(self.lib, self.lib.gs_set_graph(h, _ptr(self.rowptr, C.c_int64), _ptr(self.col, C.c_int32),
                                                   _ptr(ob, C.c_uint8), _ptr(direct, C.c_uint8)))
        else:
            _check(self.lib, self.lib.gs_set_graph_ex(h, _ptr(self.rowptr, C.c_int64), _ptr(self.col, C.c_int32),
                                                      _ptr(ob, C.c_uint8), _ptr(direct, C.c_uint8),
                                                      _ptr(proto, C.c_uint8)))
        routers = opts.get("routers")
        if routers is not None:
            _check(self.lib, self.lib.gs_set_routers(h, _ptr(routers, C.c_uint8)))
        self.routers = routers
        dormant = opts.get("dormant")
        if dormant:
            da = np.array([a for a, _ in dormant], dtype=np.int32)
            db = np.array([b for _, b in dormant], dtype=np.int32)
            _check(self.lib, self.lib.gs_set_dormant(h, len(da), _ptr(da, C.c_int32), _ptr(db, C.c_int32)))
        tr = opts.get("trace")
        if tr is not None:
            nodes, cap, rpc = tr
            mask = np.zeros(num_nodes, dtype=np.uint8)
            nodes = np.asarray(nodes)
            mask[np.nonzero(nodes)[0] if nodes.dtype == bool else nodes] = 1
            _check(self.lib, self.lib.gs_set_trace(h, _ptr(mask, C.c_uint8), cap))
            if rpc:
                _check(self.lib, self.lib.gs_set_trace_rpc(h, 1))
        ptx = opts.get("peertx")
        if ptx is not None:
            _check(self.lib, self.lib.gs_set_peertx_capacity(h, *ptx))
        if opts.get("frontier_mode"):
            _check(self.lib, self.lib.gs_set_frontier_mode(h, opts["frontier_mode"]))
        # the product-only options: a library without one's exports closes the engine and raises
        if opts.get("latency_stats"):
            _check(self.lib, self._product("latency", closing=True).gs_set_latency_stats(h, 1))
        self._inspect = None
        if insp is not None:
            lib = self._product("inspect", closing=True)
            bounds = insp["bounds"]
            if bounds is None:
                bounds = _checked_bounds(default_inspect_bounds(score[1])) if score is not None else np.zeros(0)
            mask = _node_mask(insp["nodes"], num_nodes)
            ic = _abi.InspectConfigC(insp["period_hops"], insp["ticks"], len(bounds), _ptr(bounds, C.c_double),
                                     _ptr(mask, C.c_uint8), 1 if insp["extended"] else 0)
            _check(lib, lib.gs_set_score_inspect(h, C.byref(ic)))
            self._inspect = dict(insp, bounds=bounds, mask=mask, delivered=0)
        if mh is not None:
            lib = self._product("mesh_health", closing=True)
            mask = np.ascontiguousarray(np.asarray(mh["nodes"]) != 0, dtype=np.uint8) if mh["nodes"] is not None else None
            mc = _abi.MeshHealthConfigC(mh["period_hops"], mh["ticks"], _ptr(mask, C.c_uint8), 1 if mh["labels"] else 0)
            _check(lib, lib.gs_set_mesh_health(h, C.byref(mc)))
        self._reach_sources = 0
        if mr is not None:
            lib = self._product("mesh_reach", closing=True)
            mask = np.ascontiguousarray(np.asarray(mr["nodes"]) != 0, dtype=np.uint8) if mr["nodes"] is not None else None
            src = np.ascontiguousarray(mr["sources"], dtype=np.int32)
            rc = _abi.MeshReachConfigC(mr["period_hops"], mr["ticks"], len(src), _ptr(src, C.c_int32),
                                       _ptr(mask, C.c_uint8), 1 if mr["depths"] else 0)
            _check(lib, lib.gs_set_mesh_reach(h, C.byref(rc)))
            self._reach_sources = len(src)
        acct = opts.get("rpc_acct")
        if acct is not None:
            ms, idl, tl, pid, rec = acct
            ms = np.ascontiguousarray(np.broadcast_to(np.asarray(ms, dtype=np.int32), (num_topics,)))
            tl = (np.array([len(str(t)) for t in range(num_topics)], dtype=np.int32) if tl is None
                  else np.ascontiguousarray(np.broadcast_to(np.asarray(tl, dtype=np.int32), (num_topics,))))
            _check(self.lib, self.lib.gs_set_rpc_accounting(h, _ptr(ms, C.c_int32), idl, _ptr(tl, C.c_int32)))
            _check(self.lib, self.lib.gs_set_rpc_px_sizes(h, pid, rec))
        self.rpc_acct = acct is not None
        self._bw_bounds = None
        if bw is not None:  # after the accounting it needs
            lib = self._product("bandwidth", closing=True)
            mask = _node_mask(bw["nodes"], num_nodes)
            bc = _abi.BandwidthConfigC(bw["period_hops"], bw["ticks"], len(bw["bounds"]), _ptr(bw["bounds"], C.c_int64),
                                       _ptr(mask, C.c_uint8))
            _check(lib, lib.gs_set_bandwidth_stats(h, C.byref(bc)))
            self._bw_bounds = bw["bounds"]
        self.router = router
        self.hop_ns = cfg.hop_ns
        self.rank, self.world, self.transport = opts.get("partition", (0, 1, None))
        if self.world > 1:
            _check(self.lib, self.lib.gs_set_partition(h, self.rank, self.world, C.byref(self.transport.c)))
        b, e = C.c_int32(), C.c_int32()
        _check(self.lib, self.lib.gs_partition_range(h, C.byref(b), C.byref(e)))
        self.node_range = (b.value, e.value)
        self.n_published = 0  # messages scheduled by publish() (all ranks)
        # the schedule by message id (publish() appends): author, topic, hop
        self.msg_src, self.msg_topic = np.empty(0, np.int32), np.empty(0, np.int32)
        self.msg_hop = np.empty(0, np.int64)
        self.events = []  # the events scheduled by schedule_events(): (hop, kind, a, b)
        self.edge_range = (int(self.rowptr[b.value]), int(self.rowptr[e.value]))
        subs = np.ascontiguousarray(subscriptions, dtype=np.uint64)
        _check(self.lib, self.lib.gs_set_subscriptions(h, _ptr(subs, C.c_uint64)))
        self.subs = subs  # the initial subscriptions (topic bit masks per node)
        val = opts.get("validation")
        if val is not None:
            tv = np.zeros(num_topics, dtype=np.uint8)
            tv[:] = np.asarray(val[0], dtype=bool)[:num_topics] if np.ndim(val[0]) else bool(val[0])
            _check(self.lib, self.lib.gs_set_validation(h, _ptr(tv, C.c_uint8), val[1]))
        beh = opts.get("behaviour")
        if beh is not None:
            beh = np.ascontiguousarray(beh, dtype=np.uint8)
            _check(self.lib, self.lib.gs_set_behaviour(h, _ptr(beh, C.c_uint8)))
        app = np.ascontiguousarray(app_score, dtype=np.float64) if app_score is not None else None
        ips = np.ascontiguousarray(ipv4, dtype=np.uint32) if ipv4 is not None else None
        self.app_attr, self.ipv4_attr = app, ips  # gs_set_peer_attrs inputs (None: zeros)
        if app is not None or ips is not None:
            _check(self.lib, self.lib.gs_set_peer_attrs(h, _ptr(app, C.c_double), _ptr(ips, C.c_uint32)))
        wl = opts.get("ip_whitelist")
        if wl is not None:
            net = np.array([n for n, _ in wl], dtype=np.uint32)
            mask = np.array([m for _, m in wl], dtype=np.uint32)
            _check(self.lib, self.lib.gs_set_ip_whitelist(h, len(wl), _ptr(net, C.c_uint32), _ptr(mask, C.c_uint32)))

    def close(self):
        if getattr(self, "h", None):
            self.lib.gs_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------------------------------------------------------- the product-only headers
    def _bind(self, functions):
        """Binds restype / argtypes of a header's `functions` if the library
        exports them all; whether it does."""
        if not all(hasattr(self.lib, name) for name, _, _ in functions):
            return False
        for name, res, args in functions:
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = res, args
        return True

    def _product(self, feature, closing=False):
        """The library, if it exports the header of `feature` (_PRODUCT_ONLY);
        else ValueError, from __init__ (`closing`) after closing the engine."""
        if not self._has[feature]:
            if closing:
                self.close()
            raise ValueError(f"{_PRODUCT_ONLY[feature][1]}: product library only")
        return self.lib

    def _ticks(self, fn):
        """Ticks taken so far; a negative result is the call's GS_* code."""
        n = fn(self.h)
        if n < 0:
            _check(self.lib, int(n))
        return int(n)

    def _kernel_stats(self, fn, names, n, counters=()):
        """{name: (total_ms, launches)} of the call's first len(names) of n
        entries, and {counter: launches[]} of the `counters` that follow them."""
        ms = np.zeros(n, dtype=np.float64)
        cnt = np.zeros(n, dtype=np.int64)
        _check(self.lib, fn(self.h, _ptr(ms, C.c_double), _ptr(cnt, C.c_int64)))
        out = {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(names)}
        out.update((k, int(cnt[len(names) + j])) for j, k in enumerate(counters))
        return out

    # ---------------------------------------------------------------- driving
    def publish(self, src, topic, hop, kind=None):
        """Topic.Publish at node src[i] at hop hop[i]; kind[i] (GS_MSG_*) is the
        verdict of the receivers' topic validator, or PHANTOM (advertised only)."""
        src = np.ascontiguousarray(src, dtype=np.int32)
        topic = np.ascontiguousarray(topic, dtype=np.int32)
        hop = np.ascontiguousarray(hop, dtype=np.int64)
        ids = np.empty(len(src), dtype=np.int64)
        kd = np.ascontiguousarray(kind, dtype=np.uint8) if kind is not None else None
        _check(self.lib, self.lib.gs_publish_ex(self.h, len(src), _ptr(src, C.c_int32), _ptr(topic, C.c_int32),
                                                _ptr(hop, C.c_int64), _ptr(kd, C.c_uint8), _ptr(ids, C.c_int64)))
        self.n_published += len(src)
        self.msg_src = np.concatenate([self.msg_src, src])
        self.msg_topic = np.concatenate([self.msg_topic, topic])
        self.msg_hop = np.concatenate([self.msg_hop, hop])
        return ids

    def schedule_events(self, kind, a, b, hop):
        """Connection churn and subscription changes at the start of hop[i]
        (gs_schedule_events): GS_EV_DISCONNECT / GS_EV_CONNECT of the connection
        a[i] - b[i], GS_EV_LEAVE / GS_EV_JOIN of topic b[i] by node a[i]."""
        kind = np.ascontiguousarray(kind, dtype=np.int32)
        a = np.ascontiguousarray(a, dtype=np.int32)
        b = np.ascontiguousarray(b, dtype=np.int32)
        hop = np.ascontiguousarray(hop, dtype=np.int64)
        _check(self.lib, self.lib.gs_schedule_events(self.h, len(kind), _ptr(kind, C.c_int32), _ptr(a, C.c_int32),
                                                     _ptr(b, C.c_int32), _ptr(hop, C.c_int64)))
        self.events += list(zip(hop.tolist(), kind.tolist(), a.tolist(), b.tolist()))

    def exchange_stats(self):
        """(host ms spent in the transport, bytes received from other ranks)."""
        ms, nb = C.c_double(), C.c_int64()
        _check(self.lib, self.lib.gs_read_exchange_stats(self.h, C.byref(ms), C.byref(nb)))
        return ms.value, nb.value

    @property
    def frontier_dense(self):
        """True once started if phase A ORs frontier bitmaps (gs_frontier_dense)."""
        return bool(self.lib.gs_frontier_dense(self.h))

    def step(self, hops=1):
        hops = int(hops)
        if self._inspect is None or self._inspect["inspect"] is None:
            _check(self.lib, self.lib.gs_step(self.h, hops))
            return
        # a callback: chunks no longer than the ring, so that no tick is overwritten unread
        chunk = self._inspect["ticks"] * self._inspect["period_hops"]
        while hops > 0:
            n = min(hops, chunk)
            _check(self.lib, self.lib.gs_step(self.h, n))
            hops -= n
            self._deliver_ticks()

    def sync(self):
        _check(self.lib, self.lib.gs_sync(self.h))

    def set_topic_score_params(self, topic, p):
        c = p.to_c()
        _check(self.lib, self.lib.gs_set_topic_score_params(self.h, topic, C.byref(c)))

    @property
    def hop(self):
        return int(self.lib.gs_current_hop(self.h))

    # ---------------------------------------------------------------- readbacks
    def counters(self):
        c = _abi.CountersC()
        _check(self.lib, self.lib.gs_read_counters(self.h, C.byref(c)))
        return c.as_dict()

    def scores(self):
        a = np.empty(self.E, dtype=np.float64)
        _check(self.lib, self.lib.gs_read_scores(self.h, _ptr(a, C.c_double)))
        return a

    def mesh(self):
        a = np.empty(self.E, dtype=np.uint64)
        _check(self.lib, self.lib.gs_read_mesh(self.h, _ptr(a, C.c_uint64)))
        return a

    def fanout(self):
        a = np.empty(self.E, dtype=np.uint64)
        _check(self.lib, self.lib.gs_read_fanout(self.h, _ptr(a, C.c_uint64)))
        return a

    def backoff(self):
        a = np.empty(self.E * self.T, dtype=np.int64)
        _check(self.lib, self.lib.gs_read_backoff(self.h, _ptr(a, C.c_int64)))
        return a.reshape(self.T, self.E)

    def topic_stats(self):
        n = self.E * self.T
        fmd, mmd, mfp, imd = (np.empty(n, dtype=np.float64) for _ in range(4))
        mt, gt = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
        fl = np.empty(n, dtype=np.uint8)
        _check(self.lib, self.lib.gs_read_topic_stats(
            self.h, _ptr(fmd, C.c_double), _ptr(mmd, C.c_double), _ptr(mfp, C.c_double),
            _ptr(imd, C.c_double), _ptr(mt, C.c_int64), _ptr(gt, C.c_int64), _ptr(fl, C.c_uint8)))
        sh = (self.T, self.E)
        return dict(fmd=fmd.reshape(sh), mmd=mmd.reshape(sh), mfp=mfp.reshape(sh), imd=imd.reshape(sh),
                    mesh_time=mt.reshape(sh), graft_time=gt.reshape(sh), flags=fl.reshape(sh))

    def topic_stats_at(self, edges):
        """topic_stats() of the given edges only, shape (len(edges), T) per field
        (gs_read_topic_stats_edges): spot checks at full size."""
        edges = np.ascontiguousarray(edges, dtype=np.int64)
        n = len(edges) * self.T
        fmd, mmd, mfp, imd = (np.empty(n, dtype=np.float64) for _ in range(4))
        mt, gt = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
        fl = np.empty(n, dtype=np.uint8)
        _check(self.lib, self.lib.gs_read_topic_stats_edges(
            self.h, len(edges), _ptr(edges, C.c_int64), _ptr(fmd, C.c_double), _ptr(mmd, C.c_double),
            _ptr(mfp, C.c_double), _ptr(imd, C.c_double), _ptr(mt, C.c_int64), _ptr(gt, C.c_int64),
            _ptr(fl, C.c_uint8)))
        sh = (len(edges), self.T)
        return dict(fmd=fmd.reshape(sh), mmd=mmd.reshape(sh), mfp=mfp.reshape(sh), imd=imd.reshape(sh),
                    mesh_time=mt.reshape(sh), graft_time=gt.reshape(sh), flags=fl.reshape(sh))

    def backoff_at(self, edges):
        """backoff() of the given edges only, shape (len(edges), T) (gs_read_backoff_edges)."""
        edges = np.ascontiguousarray(edges, dtype=np.int64)
        out = np.empty(len(edges) * self.T, dtype=np.int64)
        _check(self.lib, self.lib.gs_read_backoff_edges(self.h, len(edges), _ptr(edges, C.c_int64),
                                                        _ptr(out, C.c_int64)))
        return out.reshape(len(edges), self.T)

    def enough_peers(self, topic, suggested=0):
        """PubSubRouter.EnoughPeers(topic, suggested) of every host (bool [N])."""
        out = np.zeros(self.N, dtype=np.uint8)
        _check(self.lib, self.lib.gs_enough_peers(self.h, int(topic), int(suggested), _ptr(out, C.c_uint8)))
        return out.astype(bool)

    def behaviour_penalty(self):
        a = np.empty(self.E, dtype=np.float64)
        _check(self.lib, self.lib.gs_read_behaviour_penalty(self.h, _ptr(a, C.c_double)))
        return a

    def set_profiling(self, on=True):
        _check(self.lib, self.lib.gs_set_profiling(self.h, 1 if on else 0))

    def kernel_stats(self):
        """{kernel: (total_ms, launches)} accumulated since set_profiling(True)."""
        n = len(_abi.KERNEL_NAMES)
        ms = np.zeros(n, dtype=np.float64)
        cnt = np.zeros(n, dtype=np.int64)
        _check(self.lib, self.lib.gs_read_kernel_stats(self.h, _ptr(ms, C.c_double), _ptr(cnt, C.c_int64)))
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(_abi.KERNEL_NAMES)}

    def rpc_bytes(self):
        """(bytes[E], rpcs[E]) sent over every directed edge since the start."""
        b = np.empty(self.E, dtype=np.int64)
        n = np.empty(self.E, dtype=np.int64)
        _check(self.lib, self.lib.gs_read_rpc_bytes(self.h, _ptr(b, C.c_int64), _ptr(n, C.c_int64)))
        return b, n

    def trace_events(self, chunk=1 << 16):
        """Every recorded event since the last call, in canonical order
        (include/gs_trace.h), as a structured array (_abi.TRACE_EVENT_DTYPE)."""
        parts = []
        n = C.c_int64()
        while True:
            buf = np.empty(chunk, dtype=_abi.TRACE_EVENT_DTYPE)
            _check(self.lib, self.lib.gs_trace_read(self.h, buf.ctypes.data, chunk, C.byref(n)))
            parts.append(buf[:n.value])
            if n.value < chunk:
                return np.concatenate(parts)

    # ---------------------------------------------------------------- latency statistics
    def topic_windows(self):
        """(slots, max_age_hops, retire_hops), int32 [T] each: the message window
        in force per topic (gs_read_topic_windows): its ring, the age up to which
        a first delivery is accepted, and the hops after which its slots are
        taken again.  Product library only."""
        lib = self._product("windows")
        out = [np.zeros(self.T, dtype=np.int32) for _ in range(3)]
        _check(lib, lib.gs_read_topic_windows(self.h, *[_ptr(a, C.c_int32) for a in out]))
        return tuple(out)

    def latency_bins(self):
        """maxAge + 1 (gs_latency_bins), once the engine has started."""
        lib = self._product("latency")
        bins = lib.gs_latency_bins(self.h)
        if bins < 0:
            _check(lib, bins)
        return bins

    def latency_hist(self):
        """First deliveries by topic and age in hops, int64 [T, bins], since the
        start or the last reset_latency_stats(); a partitioned rank's own nodes."""
        bins = self.latency_bins()
        a = np.zeros((self.T, bins), dtype=np.int64)
        _check(self.lib, self.lib.gs_read_latency_hist(self.h, _ptr(a, C.c_int64), bins))
        return a

    def message_latency(self, ids):
        """First deliveries by age of the messages `ids`, uint32 [n, bins]
        (gs_read_message_latency: a recycled slot is refused, a message not
        yet published reads zeros)."""
        bins = self.latency_bins()
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        a = np.zeros((len(ids), bins), dtype=np.uint32)
        _check(self.lib, self.lib.gs_read_message_latency(self.h, len(ids), _ptr(ids, C.c_int64),
                                                          _ptr(a, C.c_uint32), bins))
        return a

    def reset_latency_stats(self):
        """Zeroes the per-topic table (message_latency is unaffected)."""
        _check(self.lib, self._product("latency").gs_reset_latency_stats(self.h))

    def latency_kernel_stats(self):
        """{"lat_count" | "lat_fold": (total_ms, launches)} since set_profiling(True)."""
        return self._kernel_stats(self._product("latency").gs_read_latency_kernel_stats, ("lat_count", "lat_fold"), 2)

    # ---------------------------------------------------------------- score inspection
    def inspect_ticks(self):
        """Ticks taken so far (gs_inspect_ticks)."""
        return self._ticks(self._product("inspect").gs_inspect_ticks)

    def inspect_row(self, k):
        """Tick k: dict(hop, score_hist int64 [len(bounds) + 1], mesh_deg int64
        [T, 65]) of this rank's owned edges and nodes (gs_read_inspect_row)."""
        lib = self._product("inspect")
        nb = len(self._inspect["bounds"]) if self._inspect else 0
        hop = C.c_int64()
        hist = np.zeros(nb + 1, dtype=np.int64)
        deg = np.zeros((self.T, _abi.GS_INSPECT_DEG_BINS), dtype=np.int64)
        _check(lib, lib.gs_read_inspect_row(self.h, int(k), C.byref(hop), _ptr(hist, C.c_int64),
                                            _ptr(deg, C.c_int64)))
        return dict(hop=hop.value, score_hist=hist, mesh_deg=deg)

    def inspect_edges(self):
        """The sampled edges of this rank (the out-edges of its observers), ascending."""
        lib = self._product("inspect")
        n = C.c_int64()
        _check(lib, lib.gs_inspect_num_edges(self.h, C.byref(n)))
        edges = np.zeros(n.value, dtype=np.int64)
        _check(lib, lib.gs_inspect_edges(self.h, _ptr(edges, C.c_int64), n.value))
        return edges

    def inspect_scores(self, k):
        """The sampled edges' scores at tick k, float64 [len(inspect_edges())]."""
        lib = self._product("inspect")
        n = C.c_int64()
        _check(lib, lib.gs_inspect_num_edges(self.h, C.byref(n)))
        a = np.zeros(n.value, dtype=np.float64)
        _check(lib, lib.gs_read_inspect_scores(self.h, int(k), _ptr(a, C.c_double)))
        return a

    def inspect_snapshot(self, k):
        """The sampled edges' PeerScoreSnapshot fields at tick k (extended=True):
        dict(app, ip_colocation, behaviour_penalty [nS]; time_in_mesh int64, fmd,
        mmd, imd [nS, T])."""
        lib = self._product("inspect")
        n = C.c_int64()
        _check(lib, lib.gs_inspect_num_edges(self.h, C.byref(n)))
        nS, sh = n.value, (n.value, self.T)
        app, ipc, bp = (np.zeros(nS, dtype=np.float64) for _ in range(3))
        tim = np.zeros(sh, dtype=np.int64)
        fmd, mmd, imd = (np.zeros(sh, dtype=np.float64) for _ in range(3))
        _check(lib, lib.gs_read_inspect_snapshot(self.h, int(k), _ptr(app, C.c_double), _ptr(ipc, C.c_double),
                                                 _ptr(bp, C.c_double), _ptr(tim, C.c_int64), _ptr(fmd, C.c_double),
                                                 _ptr(mmd, C.c_double), _ptr(imd, C.c_double)))
        return dict(app=app, ip_colocation=ipc, behaviour_penalty=bp, time_in_mesh=tim, fmd=fmd, mmd=mmd, imd=imd)

    def inspect_kernel_stats(self):
        """{"insp_score" | "insp_reduce" | "insp_gather": (total_ms, launches)} since set_profiling(True)."""
        return self._kernel_stats(self._product("inspect").gs_read_inspect_kernel_stats, _abi.INSPECT_KERNEL_NAMES, 3)

    def _inspect_maps(self, k, edges):
        """Tick k as the reference's inspect functions get it: {observer: {peer:
        score}}, or {observer: {peer: PeerScoreSnapshot}} when extended."""
        obs = np.searchsorted(self.rowptr, edges, side="right") - 1
        score = self.inspect_scores(k)
        snap = self.inspect_snapshot(k) if self._inspect["extended"] else None
        mask, (n0, n1) = self._inspect["mask"], self.node_range
        out = {int(u): {} for u in (np.flatnonzero(mask[n0:n1]) + n0 if mask is not None else ())}
        for i, (u, e) in enumerate(zip(obs.tolist(), edges.tolist())):
            if snap is None:
                val = float(score[i])
            else:
                topics = {t: TopicScoreSnapshot(int(snap["time_in_mesh"][i, t]), float(snap["fmd"][i, t]),
                                                float(snap["mmd"][i, t]), float(snap["imd"][i, t]))
                          for t in range(self.T)}
                val = PeerScoreSnapshot(float(score[i]), topics, float(snap["app"][i]),
                                        float(snap["ip_colocation"][i]), float(snap["behaviour_penalty"][i]))
            out.setdefault(u, {})[int(self.col[e])] = val
        return out

    def _deliver_ticks(self):
        st = self._inspect
        taken = self.inspect_ticks()
        edges = self.inspect_edges() if taken > st["delivered"] else None
        while st["delivered"] < taken:
            k = st["delivered"]
            st["delivered"] += 1
            st["inspect"]((k + 1) * st["period_hops"], self._inspect_maps(k, edges))

    # ---------------------------------------------------------------- mesh health
    def mesh_health_ticks(self):
        """Ticks taken so far (gs_mesh_health_ticks)."""
        return self._ticks(self._product("mesh_health").gs_mesh_health_ticks)

    def mesh_health_row(self, k):
        """Tick k: dict(hop; members, components, largest, isolated, one_sided,
        outside, eclipsed int64 [T]; comp_hist int64 [T, 32]) (gs_read_mesh_health_row)."""
        lib = self._product("mesh_health")
        hop = C.c_int64()
        row = np.zeros((self.T, len(_abi.MESH_ROW_FIELDS)), dtype=np.int64)
        hist = np.zeros((self.T, _abi.GS_MESH_SIZE_BINS), dtype=np.int64)
        _check(lib, lib.gs_read_mesh_health_row(self.h, int(k), C.byref(hop), _ptr(row, C.c_int64),
                                                _ptr(hist, C.c_int64)))
        out = {name: np.ascontiguousarray(row[:, i]) for i, name in enumerate(_abi.MESH_ROW_FIELDS)}
        return dict(out, hop=hop.value, comp_hist=hist)

    def mesh_labels(self):
        """(tick, int32 [N, T]): the newest tick and every host's component label
        per topic, the smallest host id of its component, -1 for a non-member
        (WithMeshHealth(labels=True))."""
        lib = self._product("mesh_health")
        tick = C.c_int64()
        lab = np.zeros((self.N, self.T), dtype=np.int32)
        _check(lib, lib.gs_read_mesh_labels(self.h, C.byref(tick), _ptr(lab, C.c_int32)))
        return tick.value, lab

    def mesh_health_kernel_stats(self):
        """{"mesh_init" | "mesh_label" | "mesh_sizes" | "mesh_row": (total_ms,
        launches)} since set_profiling(True), and "iterations" / "bytes": the
        label iterations run and the bytes moved since then (or the start)."""
        return self._kernel_stats(self._product("mesh_health").gs_read_mesh_health_kernel_stats,
                                  _abi.MESH_KERNEL_NAMES, len(_abi.MESH_STAT_NAMES), ("iterations", "bytes"))

    # ---------------------------------------------------------------- bandwidth statistics
    def bandwidth_ticks(self):
        """Ticks taken so far (gs_bandwidth_ticks)."""
        return self._ticks(self._product("bandwidth").gs_bandwidth_ticks)

    def bandwidth_nodes(self):
        """The sampled nodes, ascending (gs_bandwidth_nodes), int32 [nS]."""
        lib = self._product("bandwidth")
        n = C.c_int64()
        _check(lib, lib.gs_bandwidth_num_nodes(self.h, C.byref(n)))
        nodes = np.zeros(n.value, dtype=np.int32)
        _check(lib, lib.gs_bandwidth_nodes(self.h, _ptr(nodes, C.c_int32), n.value))
        return nodes

    def bandwidth_row(self, k):
        """Tick k: dict(hop; total int64 [4] bytes per class (all, eager, pulled,
        overhead); total_rpcs; hist int64 [2, 4, len(bounds) + 1] hosts by their
        bytes (egress / ingress, class); max and argmax int64 [2, 4], argmax -1
        where max is 0) (gs_read_bandwidth_row)."""
        lib = self._product("bandwidth")
        nb = len(self._bw_bounds) if self._bw_bounds is not None else 0
        hop, rpcs = C.c_int64(), C.c_int64()
        total = np.zeros(4, dtype=np.int64)
        hist = np.zeros((2, 4, nb + 1), dtype=np.int64)
        mx, arg = np.zeros((2, 4), dtype=np.int64), np.zeros((2, 4), dtype=np.int64)
        _check(lib, lib.gs_read_bandwidth_row(self.h, int(k), C.byref(hop), _ptr(total, C.c_int64), C.byref(rpcs),
                                              _ptr(hist, C.c_int64), _ptr(mx, C.c_int64), _ptr(arg, C.c_int64)))
        return dict(hop=hop.value, total=total, total_rpcs=rpcs.value, hist=hist, max=mx, argmax=arg)

    def bandwidth_sampled(self, k):
        """Tick k: (bytes int64 [nS, 2, 4], rpcs int64 [nS, 2]) of the sampled
        nodes, in bandwidth_nodes() order (gs_read_bandwidth_nodes)."""
        lib = self._product("bandwidth")
        n = C.c_int64()
        _check(lib, lib.gs_bandwidth_num_nodes(self.h, C.byref(n)))
        b = np.zeros((n.value, 2, 4), dtype=np.int64)
        r = np.zeros((n.value, 2), dtype=np.int64)
        _check(lib, lib.gs_read_bandwidth_nodes(self.h, int(k), _ptr(b, C.c_int64), _ptr(r, C.c_int64)))
        return b, r

    def bandwidth_kernel_stats(self):
        """{"bw_tick" | "bw_argmax" | "bw_gather": (total_ms, launches)} since
        set_profiling(True)."""
        return self._kernel_stats(self._product("bandwidth").gs_read_bandwidth_kernel_stats,
                                  _abi.BANDWIDTH_KERNEL_NAMES, len(_abi.BANDWIDTH_KERNEL_NAMES))

    # ---------------------------------------------------------------- mesh reach
    def mesh_reach_ticks(self):
        """Ticks taken so far (gs_mesh_reach_ticks)."""
        return self._ticks(self._product("mesh_reach").gs_mesh_reach_ticks)

    def mesh_reach_row(self, k):
        """Tick k: dict(hop; reached, unreached, ecc int64 [K, T]; depth_hist
        int64 [K, T, 64]) over the K sources (gs_read_mesh_reach_row)."""
        lib = self._product("mesh_reach")
        K = max(self._reach_sources, 1)
        hop = C.c_int64()
        row = np.zeros((K, self.T, len(_abi.REACH_ROW_FIELDS)), dtype=np.int64)
        hist = np.zeros((K, self.T, _abi.GS_REACH_DEPTH_BINS), dtype=np.int64)
        _check(lib, lib.gs_read_mesh_reach_row(self.h, int(k), C.byref(hop), _ptr(row, C.c_int64),
                                               _ptr(hist, C.c_int64)))
        out = {name: np.ascontiguousarray(row[:, :, i]) for i, name in enumerate(_abi.REACH_ROW_FIELDS)}
        return dict(out, hop=hop.value, depth_hist=hist)

    def mesh_reach_depths(self):
        """(tick, uint8 [K, N, T]): the newest tick and every host's eager-push
        depth from every source per topic: 0 in the source's own row, 255 where
        it is not reached, depths past 254 read 254 (WithMeshReach(depths=True))."""
        lib = self._product("mesh_reach")
        tick = C.c_int64()
        dep = np.zeros((max(self._reach_sources, 1), self.N, self.T), dtype=np.uint8)
        _check(lib, lib.gs_read_mesh_reach_depths(self.h, C.byref(tick), _ptr(dep, C.c_uint8)))
        return tick.value, dep

    def mesh_reach_kernel_stats(self):
        """{"reach_members" | "reach_init" | "reach_level" | "reach_finish":
        (total_ms, launches)} since set_profiling(True), and "passes" / "levels"
        / "bytes": the passes and levels run and the bytes moved since then (or
        the start)."""
        return self._kernel_stats(self._product("mesh_reach").gs_read_mesh_reach_kernel_stats,
                                  _abi.REACH_KERNEL_NAMES, len(_abi.REACH_STAT_NAMES), ("passes", "levels", "bytes"))

    def deliveries(self, msg_id):
        hop = np.empty(self.N, dtype=np.int32)
        frm = np.empty(self.N, dtype=np.int32)
        _check(self.lib, self.lib.gs_read_deliveries(self.h, int(msg_id), _ptr(hop, C.c_int32),
                                                     _ptr(frm, C.c_int32)))
        return hop, frm


PROTOCOLS = {_abi.GS_ROUTER_FLOODSUB: "/floodsub/1.0.0", _abi.GS_ROUTER_RANDOMSUB: "/randomsub/1.0.0",
             _abi.GS_ROUTER_GOSSIPSUB: "/meshsub/1.1.0"}  # floodsub.go:15, randomsub.go:16, gossipsub.go:25


def encode_trace(events, fmt=_abi.GS_TRACE_FORMAT_PB, hop_ns=100 * Millisecond, topic_names=None,
                 proto="/meshsub/1.1.0", lib=None):
    """The reference tracers' output for `events` (Engine.trace_events()):
    uvarint-delimited pb.TraceEvent (PBTracer) or JSON lines (JSONTracer)."""
    lib = load(lib)
    ev = np.ascontiguousarray(events, dtype=_abi.TRACE_EVENT_DTYPE)
    names = None
    if topic_names is not None:
        names = (C.c_char_p * len(topic_names))(*[t if isinstance(t, bytes) else t.encode() for t in topic_names])
    need = C.c_int64()
    rc = lib.gs_trace_encode(ev.ctypes.data, len(ev), fmt, hop_ns, names, proto.encode(), None, 0, C.byref(need))
    if rc not in (_abi.GS_OK, _abi.GS_ECAPACITY):
        _check(lib, rc)
    buf = (C.c_uint8 * max(1, need.value))()
    _check(lib, lib.gs_trace_encode(ev.ctypes.data, len(ev), fmt, hop_ns, names, proto.encode(),
                                    C.cast(buf, C.c_void_p), need.value, C.byref(need)))
    return bytes(buf[:need.value])


def NewFloodSub(num_nodes, num_topics, graph, subscriptions, *options, **kw):
    """floodsub.go:25-27 (batched)."""
    return Engine(_abi.GS_ROUTER_FLOODSUB, num_nodes, num_topics, graph, subscriptions, *options, **kw)


def NewRandomSub(num_nodes, num_topics, graph, subscriptions, size, *options, **kw):
    """randomsub.go:21-27 (batched)."""
    return Engine(_abi.GS_ROUTER_RANDOMSUB, num_nodes, num_topics, graph, subscriptions, *options,
                  randomsub_size=size, **kw)


def NewGossipSub(num_nodes, num_topics, graph, subscriptions, *options, **kw):
    """gossipsub.go:198-222 (batched)."""
    return Engine(_abi.GS_ROUTER_GOSSIPSUB, num_nodes, num_topics, graph, subscriptions, *options, **kw)
