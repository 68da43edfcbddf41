// gs_engine.hip — product C-ABI (include/gossip_engine.h) over HIP kernels
// for gfx950.  Host side: validation, graph preprocessing (reverse edges,
// P6 colocation factors), message-slot assignment, device allocation and the
// per-hop launch schedule (DESIGN.md §4 "Canonical round").  Every kernel runs
// on one HIP stream per engine; gs_step enqueues many hops and synchronises
// once at the end to check the device error word.
#include "gs_engine.h"

static thread_local std::string g_err;
void gs_set_error(const std::string& msg) { g_err = msg; }

// Contiguous node ranges balanced by edges: rank r owns the nodes whose CSR
// rows start in [E*r/world, E*(r+1)/world).  Identical on every rank.
static std::vector<int32_t> partition_bounds(const std::vector<int64_t>& rowptr, int N, int world) {
  const int64_t E = rowptr[N];
  std::vector<int32_t> part(world + 1, N);
  part[0] = 0;
  for (int r = 1; r < world; ++r)
    part[r] = (int32_t)(std::lower_bound(rowptr.begin(), rowptr.begin() + N, (E * r) / world) - rowptr.begin());
  for (int r = 1; r <= world; ++r) part[r] = std::max(part[r], part[r - 1]);
  return part;
}

static TopicP to_dev(const gs_topic_score_params& p, bool scored) {
  TopicP t{};
  t.TopicWeight = p.TopicWeight;
  t.TimeInMeshWeight = p.TimeInMeshWeight;
  t.TimeInMeshQuantum = p.TimeInMeshQuantum ? p.TimeInMeshQuantum : 1;
  t.TimeInMeshCap = p.TimeInMeshCap;
  t.FmdWeight = p.FirstMessageDeliveriesWeight;
  t.FmdDecay = p.FirstMessageDeliveriesDecay;
  t.FmdCap = p.FirstMessageDeliveriesCap;
  t.MmdWeight = p.MeshMessageDeliveriesWeight;
  t.MmdDecay = p.MeshMessageDeliveriesDecay;
  t.MmdCap = p.MeshMessageDeliveriesCap;
  t.MmdThreshold = p.MeshMessageDeliveriesThreshold;
  t.MmdWindow = p.MeshMessageDeliveriesWindow;
  t.MmdActivation = p.MeshMessageDeliveriesActivation;
  t.MfpWeight = p.MeshFailurePenaltyWeight;
  t.MfpDecay = p.MeshFailurePenaltyDecay;
  t.ImdWeight = p.InvalidMessageDeliveriesWeight;
  t.ImdDecay = p.InvalidMessageDeliveriesDecay;
  t.scored = scored ? 1 : 0;
  // reciprocal of the quantum for quantum_div: floor(2^64 / q), q >= 2
  t.qMagic = gs_quantum_magic(t.TimeInMeshQuantum);
  return t;
}

static inline unsigned nblk(int64_t n, int b) { return (unsigned)((n + b - 1) / b); }

// Runtime values as compile-time constants, for choosing a kernel variant:
// with_consts(f, a, b...) calls f(A, B...), where a Flag{b} arrives as
// std::bool_constant<b> and a Pick<N>{v} as std::integral_constant<int, v>
// (v at most N - 1).  f is instantiated for every combination, so the
// arguments must span exactly the variants that exist.
struct Flag { bool v; };
template <int N>
struct Pick { int v; };
#define CV(c) (decltype(c)::value)
template <class G>
static void pick_const(Flag p, G&& g) {
  if (p.v) g(std::true_type{});
  else g(std::false_type{});
}
template <class G, int... I>
static void pick_seq(int v, G&& g, std::integer_sequence<int, I...>) {
  // tried from N - 1 down: clang then instantiates g, and places the kernels
  // it names in the code object, in ascending order
  constexpr int N = (int)sizeof...(I);
  (void)(((v >= N - 1 - I || I == N - 1) && (g(std::integral_constant<int, N - 1 - I>{}), true)) || ...);
}
template <int N, class G>
static void pick_const(Pick<N> p, G&& g) { pick_seq(p.v, g, std::make_integer_sequence<int, N>{}); }
template <class F>
static void with_consts(F&& f) { f(); }
template <class F, class P, class... Rest>
static void with_consts(F&& f, P p, Rest... rest) {
  pick_const(p, [&](auto c) { with_consts([&](auto... cs) { f(c, cs...); }, rest...); });
}
static Pick<GS_MAX_WPL> wpl_of(int W) { return {(W + 63) / 64 - 1}; }  // words per lane - 1

// k_score_rows over nEdges edges from d.e0 (lanes hold whole topic rows when
// T divides 64)
template <int MODE>
static void score_rows(const Dev& d, int64_t nEdges, int T, double* out, hipStream_t s) {
  const unsigned g = nblk(nEdges, GS_SCW);
  if (g == 0) return;
  with_consts([&](auto laneT) { k_score_rows<MODE, CV(laneT)><<<g, 64, 0, s>>>(d, out); }, Flag{64 % T == 0});
}

// Launch `stmt` on g's stream; with profiling on, bracket it with HIP events
// recorded on that same stream (so the measured interval is the kernel's).
#define TIMED(g, kid, stmt)                                   \
  do {                                                        \
    if ((g)->profiling) {                                     \
      hipEvent_t _a = (g)->nextEvent(), _b = (g)->nextEvent(); \
      (void)hipEventRecord(_a, (g)->stream);                  \
      stmt;                                                   \
      (void)hipEventRecord(_b, (g)->stream);                  \
      (g)->pendKid.push_back(kid);                            \
    } else {                                                  \
      stmt;                                                   \
    }                                                         \
  } while (0)

// The rules of gs_set_routers / gs_set_graph_ex (gossip_engine.h): protocols
// both hosts speak, equal on both directions; the negotiated one by default.
int gs_engine::validateMixed() {
  auto rt = [&](int u) { return routerH.empty() ? cfg.router : (int)routerH[u]; };
  mixed = !routerH.empty() || protoGiven;
  const bool given = protoGiven;  // (a start() tried again finds protoH filled in by the first)
  if (!given) protoH.assign((size_t)E, 0);
  auto edgeOf = [&](int a, int b) -> int64_t {
    return (int64_t)(std::lower_bound(col.begin() + rowptr[a], col.begin() + rowptr[a + 1], b) - col.begin());
  };
  for (int u = 0; u < N; ++u) {
    const int ru = rt(u);
    const bool gsHost = ru == GS_ROUTER_GOSSIPSUB || ru == GS_ROUTER_GOSSIPSUB_V10;
    if (gsHost && cfg.router != GS_ROUTER_GOSSIPSUB) {
      gs_set_error("gossipsub hosts need cfg.router == GS_ROUTER_GOSSIPSUB (their params come from the engine)");
      return GS_EINVAL;
    }
    if (!behaveH.empty() && behaveH[u] && !gsHost) { gs_set_error("attacker behaviours need gossipsub hosts"); return GS_EINVAL; }
    for (int64_t e = rowptr[u]; e < rowptr[u + 1]; ++e) {
      const int v = col[e], rv = rt(v);
      if (!gsHost && !direct.empty() && direct[e]) { gs_set_error("direct peers need a gossipsub host"); return GS_EINVAL; }
      if (!given) {
        protoH[e] = (uint8_t)gs_negotiate(ru, rv);
        continue;
      }
      const int64_t r = edgeOf(v, u);
      const int pr = protoH[e] == GS_PROTO_DEFAULT ? gs_negotiate(ru, rv) : protoH[e];
      const int pb = protoH[r] == GS_PROTO_DEFAULT ? gs_negotiate(rv, ru) : protoH[r];
      if (pr != pb || !gs_router_speaks(ru, pr) || !gs_router_speaks(rv, pr)) {
        gs_set_error("proto[e] must be a protocol both hosts speak, equal on both directions of the connection");
        return GS_EINVAL;
      }
    }
  }
  if (given)
    for (int u = 0; u < N; ++u)
      for (int64_t e = rowptr[u]; e < rowptr[u + 1]; ++e)
        if (protoH[e] == GS_PROTO_DEFAULT) protoH[e] = (uint8_t)gs_negotiate(rt(u), rt(col[e]));
  return GS_OK;
}

// The first step: everything the host can work out and refuse first, then
// the device state.  A device-side failure gives everything back, so start()
// can be tried again.
int gs_engine::start() {
  Plan pl;
  GS_TRY(validateMixed());
  GS_TRY(chooseModes(pl));
  GS_TRY(hostGraph(pl));
  GS_TRY(planCapacities(pl));
  const int rc = buildDevice(pl);
  if (rc) release();
  return rc;
}

int gs_engine::buildDevice(const Plan& pl) {
  HIPCHECK(hipSetDevice(cfg.device));
  HIPCHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  int n = 0;
  HIPCHECK(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, cfg.device));
  cus = (unsigned)std::max(n, 1);
  dDev = dalloc<Dev>(1);
  GS_TRY(allocFail("Dev record"));
  setDevScalars(pl);
  GS_TRY(allocGraph(pl));
  GS_TRY(allocNodeState());
  GS_TRY(allocFrontiers());
  GS_TRY(allocNodeTables(pl));
  GS_TRY(allocEdgeState());
  GS_TRY(allocIwantPool());
  GS_TRY(allocAdversary(pl));
  GS_TRY(allocGater(pl));
  GS_TRY(allocReadback());
  GS_TRY(allocTrace());
  GS_TRY(allocPartition());
  GS_TRY(allocLatency());
  GS_TRY(allocInspect());
  GS_TRY(allocMeshHealth());
  GS_TRY(allocMeshReach());
  GS_TRY(allocFail("state", "; reduce num_nodes or slots_per_topic"));
  GS_TRY(initConnections(pl));
  GS_TRY(allocAcct(pl));
  GS_TRY(allocBandwidth());
  started = true;
  return uploadMessages();
}

int gs_engine::chooseModes(Plan& pl) {
  pl.anyRandom = cfg.router == GS_ROUTER_RANDOMSUB;
  pushOn = T >= 4;
  denseFlood = cfg.router == GS_ROUTER_FLOODSUB && !mixed && routerH.empty() && world == 1 && traceMask.empty() &&
               !acctOn && events.empty() && dormant.empty() && topicVal == 0 && behaveAll == 0 &&
               frontierMode != GS_FRONTIER_LISTS;
  // (no P3 window shorter than a message's lifetime: the dense pass counts
  // duplicates per sender, not per copy's age; one rank: the senders' rows)
  denseGossip = cfg.router == GS_ROUTER_GOSSIPSUB && T == 1 && !mixed && routerH.empty() && world == 1 &&
                events.empty() && dormant.empty() && !doPX && topicVal == 0 && behaveAll == 0 && !gaterOn &&
                !(scoring && ageWindowNeeded()) && frontierMode == GS_FRONTIER_BITMAPS;
  if (!routerH.empty()) {
    pl.anyRandom = false;
    for (uint8_t r : routerH) pl.anyRandom = pl.anyRandom || r == GS_ROUTER_RANDOMSUB;
  }
  if (doPX && N >= (1 << 26)) {  // a PX arena entry is topic << 26 | peer (gs_kernels_ctl.h px_append)
    gs_set_error("peer exchange supports fewer than 2^26 peers in this build");
    return GS_EUNSUPPORTED;
  }
  return GS_OK;
}

// Reverse edges, edge sources, this rank's range, the connections down at the
// start, P6, the direct pairs.
int gs_engine::hostGraph(Plan& pl) {
  rev.assign(E, -1);
  esrc.assign(E, 0);
  for (int u = 0; u < N; ++u) {
    pl.maxdeg = std::max<int>(pl.maxdeg, (int)(rowptr[u + 1] - rowptr[u]));
    for (int64_t e = rowptr[u]; e < rowptr[u + 1]; ++e) {
      esrc[e] = u;
      const int v = col[e];
      auto b = col.begin() + rowptr[v], en = col.begin() + rowptr[v + 1];
      auto it = std::lower_bound(b, en, u);
      if (it == en || *it != u) {
        gs_set_error("graph must be symmetric");
        return GS_EINVAL;
      }
      rev[e] = (int32_t)(it - col.begin());
    }
  }
  if (pl.maxdeg > 64) {
    gs_set_error("this build supports node degree <= 64 (one wave per node)");
    return GS_EUNSUPPORTED;
  }
  if (E > INT32_MAX) {
    gs_set_error("this build supports < 2^31 edges per engine");
    return GS_EUNSUPPORTED;
  }
  part = partition_bounds(rowptr, N, world);
  n0 = part[rank];
  n1 = part[rank + 1];
  e0 = rowptr[n0];
  e1 = rowptr[n1];
  eOwn = e1 - e0;
  // connections down at the start (gs_set_dormant): no score record, no IP
  if (!dormant.empty()) {
    pl.downH.assign((size_t)E, 0);
    for (int u = 0; u < N; ++u)
      for (int64_t e = rowptr[u]; e < rowptr[u + 1]; ++e)
        pl.downH[e] = dormant.count({std::min(u, col[e]), std::max(u, col[e])}) ? 1 : 0;
  }
  pl.p6.assign((size_t)E, 0.0);
  if (p6Live()) {
    // ipColocationFactor (score.go:335-379): peers per IP among the observer's peers
    std::unordered_map<uint32_t, int> cnt;
    for (int u = 0; u < N; ++u) {
      cnt.clear();
      for (int64_t e = rowptr[u]; e < rowptr[u + 1]; ++e)
        if (ipv4[col[e]] != 0 && !pl.isDown(e)) cnt[ipv4[col[e]]]++;
      for (int64_t e = rowptr[u]; e < rowptr[u + 1]; ++e) {
        const uint32_t ip = ipv4[col[e]];
        if (ip == 0 || pl.isDown(e)) continue;
        bool wl = false;
        for (auto& nm : whitelist)
          if ((ip & nm.second) == (nm.first & nm.second)) { wl = true; break; }
        if (wl) continue;
        const int c = cnt[ip];
        if (c > sp.IPColocationFactorThreshold) {
          const double s = (double)(c - sp.IPColocationFactorThreshold);
          pl.p6[e] = s * s;
        }
      }
    }
  }
  if (app.empty()) app.assign(N, 0.0);
  if (sub.empty()) sub.assign(N, 0);
  if (outbound.empty()) outbound.assign(E, 0);
  if (direct.empty()) direct.assign(E, 0);
  directPairs.clear();
  if (cfg.router == GS_ROUTER_GOSSIPSUB)
    for (int u = 0; u < N; ++u)
      for (int64_t e = rowptr[u]; e < rowptr[u + 1]; ++e)
        if (direct[e]) directPairs.push_back({u, col[e]});
  directInitHop = gp.DirectConnectInitialDelay <= 0 ? 0 : (gp.DirectConnectInitialDelay + cfg.hop_ns - 1) / cfg.hop_ns;
  return GS_OK;
}

// The table capacities that depend on the input, each with its limit.
int gs_engine::planCapacities(Plan& pl) {
  // frontier lists: per node FC entries of 4 bytes (a node's first deliveries
  // of one hop plus its own publishes), at most 8 GiB per parity
  const int64_t budget = 8ll << 30;
  const int64_t fc = std::min<int64_t>(S + 64, budget / (4 * (int64_t)N));
  d.FC = (int32_t)std::max<int64_t>(64, fc & ~3ll);
  // the budget gives N * FC <= 2^31 entries, the bound phase A's 32-bit list
  // offsets (sAddr, in entries) rely on; only the 64-entry floor can break
  // it (N > 2^25)
  if ((int64_t)N * d.FC > (1ll << 31)) {
    gs_set_error("too many peers for the frontier lists (N * list capacity must stay <= 2^31)");
    return GS_EUNSUPPORTED;
  }
  // gossipTracer promises (gossip_tracer.go:48-77): at most one per IWANT,
  // i.e. per peer per heartbeat (the IHAVE rides the heartbeat RPC); a
  // promise lives until its message arrives or the first heartbeat after its
  // expiry (applyIwantPenalties), so a node holds at most
  // degree x (ceil(IWantFollowupTime / HeartbeatInterval) + 2) of them.  The
  // table is sized to that bound in banks of 64 (E_PROMISES only guards it).
  int64_t live = 1;
  if (cfg.router == GS_ROUTER_GOSSIPSUB && gp.HeartbeatInterval > 0)
    live = (gp.IWantFollowupTime + gp.HeartbeatInterval - 1) / gp.HeartbeatInterval + 2;
  const int64_t bound = std::max<int64_t>(1, (int64_t)pl.maxdeg * live);
  if (bound > (int64_t)1 << 24) {
    gs_set_error("promise table bound too large (degree x (IWantFollowupTime / HeartbeatInterval + 2) > 2^24)");
    return GS_EUNSUPPORTED;
  }
  d.promCap = (int32_t)(64 * ((bound + 63) / 64));
  if (gp.GossipRetransmission > 253) {  // a peertx count byte peaks at GossipRetransmission + 2
    gs_set_error("GossipRetransmission > 253 is not supported");
    return GS_EUNSUPPORTED;
  }
  if (behaveAll & GS_BEHAVE_IWANT_SPAM) {
    pl.pmaskRowH.assign((size_t)N, -1);
    for (int v = n0; v < n1; ++v)  // drec.peers rows of the owned spammers
      if (behaveH[v] & GS_BEHAVE_IWANT_SPAM) pl.pmaskRowH[v] = pl.nSpam++;
    // peertx counts of the owned edges whose peer is an IWANT spammer
    spamRowH.assign((size_t)E, -1);
    for (int64_t ee = e0; ee < e1; ++ee)
      if (behaveH[col[ee]] & GS_BEHAVE_IWANT_SPAM) spamRowH[ee] = (int32_t)pl.nSpamEdges++;
    if (pl.nSpamEdges > INT32_MAX) { gs_set_error("too many IWANT-spammer edges"); return GS_ECAPACITY; }
    if (gp.GossipRetransmission >= 14) {  // spam_incr's nibble peaks at GossipRetransmission + 2
      gs_set_error("IWANT spammers need GossipRetransmission < 14 in this build");
      return GS_EUNSUPPORTED;
    }
  }
  return GS_OK;
}

void gs_engine::setDevScalars(const Plan& pl) {
  Dev& x = d;
  x.N = N; x.T = T; x.Wt = Wt; x.W = W; x.St = St; x.S = S; x.R = R;
  x.HL = gp.HistoryLength; x.HG = gp.HistoryGossip; x.E = E;
  x.router = cfg.router; x.scoring = scoring; x.floodPublish = floodPublish;
  x.rsTarget = 6;
  if (pl.anyRandom) {
    const int sq = (int)std::ceil(std::sqrt((double)cfg.randomsub_size));
    x.rsTarget = std::max(6, sq);
  }
  x.maxAge = ageMax; x.seed = cfg.seed; x.hop_ns = cfg.hop_ns;
  x.n0 = n0; x.n1 = n1; x.e0 = e0; x.e1 = e1; x.eOwn = eOwn; x.rank = rank; x.world = world;
  x.nOwnH = nOwn();
  x.TopicScoreCap = sp.TopicScoreCap; x.AppW = sp.AppSpecificWeight; x.IPW = sp.IPColocationFactorWeight;
  x.BPW = sp.BehaviourPenaltyWeight; x.BPThr = sp.BehaviourPenaltyThreshold; x.BPDecay = sp.BehaviourPenaltyDecay;
  x.DecayToZero = sp.DecayToZero;
  x.RetainScore = sp.RetainScore; x.IPThr = sp.IPColocationFactorThreshold;
  x.gossipThr = thr.GossipThreshold; x.publishThr = thr.PublishThreshold; x.graylistThr = thr.GraylistThreshold;
  x.oppThr = thr.OpportunisticGraftThreshold;
  x.D = gp.D; x.Dlo = gp.Dlo; x.Dhi = gp.Dhi; x.Dscore = gp.Dscore; x.Dout = gp.Dout; x.Dlazy = gp.Dlazy;
  x.GR = gp.GossipRetransmission; x.OGP = gp.OpportunisticGraftPeers; x.MaxIHaveLength = gp.MaxIHaveLength;
  x.MaxIHaveMessages = gp.MaxIHaveMessages; x.GossipFactor = gp.GossipFactor;
  x.PruneBackoff = gp.PruneBackoff; x.GraftFloodThreshold = gp.GraftFloodThreshold;
  x.IWantFollowupTime = gp.IWantFollowupTime; x.FanoutTTL = gp.FanoutTTL;
  // the PRUNE we receive carries the sender's PruneBackoff in whole seconds
  // (makePrune gossipsub.go:1809, handlePrune :819-825)
  x.PruneRecv = (gp.PruneBackoff / kSec) > 0 ? (gp.PruneBackoff / kSec) * kSec : gp.PruneBackoff;
  x.OGT = gp.OpportunisticGraftTicks ? gp.OpportunisticGraftTicks : 1;
  x.record = record ? 1 : 0;
  // per-slot first-delivery hops only when read back or when the P3 window
  // check can fail: a duplicate always arrives less than retireHops after the
  // message's first delivery, so a MeshMessageDeliveriesWindow of at least
  // that long always credits it (score.go:955)
  x.needAge = (x.record || (scoring && ageWindowNeeded())) ? 1 : 0;
  x.maxDeg = std::max(1, pl.maxdeg);
  x.stMagic = lay.uniform ? (uint32_t)(((1ull << 32) + (uint64_t)St - 1) / (uint64_t)St) : 0u;  // 0: the tables
  x.tDivM = T == 1 ? 0 : ~0ull / (uint64_t)T + 1;  // ceil(2^64 / T)
  foldEvery = std::max<int64_t>(1, 65535 / (2 * (int64_t)St));  // a hop adds at most 2*St per (edge, topic): the largest topic's
  x.doPX = doPX ? 1 : 0;
  x.PrunePeers = gp.PrunePeers;
  x.acceptPX = thr.AcceptPXThreshold;
  x.topicVal = topicVal;
  std::fill(std::begin(x.valW), std::end(x.valW), 0ull);
  for (int w = 0; w < W; ++w)
    if ((topicVal >> lay.wTopic[(size_t)w]) & 1) x.valW[w >> 6] |= 1ull << (w & 63);
  x.valQueue = valQueue;
  x.anyImd = topicVal != 0 ? 1 : 0;  // P4 can only come from a validator's rejection
  x.anyBehave = behaveAll != 0;
  x.gater = gaterOn ? 1 : 0;
  x.gRetain = gaterP.RetainStats;
  x.lastRefresh = INT64_MIN;
  x.traceRpc = traceRpc && !traceMask.empty();
}

int gs_engine::allocGraph(const Plan& pl) {
  Dev& x = d;
  int64_t* dRowptr = dalloc<int64_t>(N + 1);
  int32_t* dCol = dalloc<int32_t>(E);
  int32_t* dEsrc = dalloc<int32_t>(E);
  int32_t* dRev = dalloc<int32_t>(E);
  uint8_t* dOut = ealloc<uint8_t>();
  uint8_t* dDir = ealloc<uint8_t>();
  uint8_t* dJrIn = ealloc<uint8_t>();
  dSubOwn = dalloc<uint64_t>(N);
  dSubA = dalloc<uint64_t>(N);
  double* dApp = dalloc<double>(N);
  dP6w = ealloc<double>();
  dTp = dalloc<TopicP>(T);
  GS_TRY(allocFail("graph"));
  std::vector<uint8_t> jr(E);
  for (int64_t e = 0; e < E; ++e) jr[e] = (uint8_t)(rev[e] - rowptr[col[e]]);
  std::vector<TopicP> htp(T);
  for (int t = 0; t < T; ++t) htp[t] = to_dev(tps[t], scoring && tscored[t]);
  GS_TRY(put(dRowptr, rowptr.data(), (size_t)N + 1));
  GS_TRY(put(dCol, col.data(), (size_t)E));
  GS_TRY(put(dEsrc, esrc.data(), (size_t)E));
  GS_TRY(put(dRev, rev.data(), (size_t)E));
  GS_TRY(put(dSubOwn, sub.data(), (size_t)N));
  GS_TRY(put(dSubA, sub.data(), (size_t)N));
  subA = sub;
  GS_TRY(put(dApp, app.data(), (size_t)N));
  GS_TRY(put(dTp, htp.data(), (size_t)T));
  GS_TRY(putEdges(dJrIn, jr));
  GS_TRY(putEdges(dOut, outbound));
  GS_TRY(putEdges(dDir, direct));
  GS_TRY(putEdges(dP6w, pl.p6));  // (each waits for the stream: the locals above may go)
  x.rowptr = dRowptr; x.col = dCol; x.esrc = dEsrc; x.rev = dRev; x.outbound = dOut; x.direct = dDir; x.jrIn = dJrIn;
  x.sub = dSubOwn; x.subA = dSubA; x.app = dApp; x.p6 = dP6w; x.tp = dTp;
  return GS_OK;
}

// Per-node state only the node's own wave touches (seen, the mcache ring,
// first-delivery ages / senders, promises, peertx, drec.peers) is allocated
// for the owned nodes [n0, n1) only: seen / age / ffrom / promises / peertx
// through nalloc's shifted base, the mcache ring [R][nOwn][W] indexed by
// v - n0 (hist_row).  A partitioned rank holds 1/world of it.
int gs_engine::allocNodeState() {
  Dev& x = d;
  x.seen = nalloc<uint64_t>(W);
  x.hist = dalloc<uint64_t>((size_t)R * nOwn() * W);
  if (cfg.router == GS_ROUTER_GOSSIPSUB) x.gw = dalloc<uint64_t>((size_t)N * W);
  if (x.needAge) x.age = nalloc<int16_t>(S);
  if (x.record) x.ffrom = nalloc<uint8_t>(S);
  return allocFail("per-node state");
}

int gs_engine::allocFrontiers() {
  Dev& x = d;
  const size_t NW = (size_t)N * W;
  const bool denseAny = denseFlood || denseGossip;
  for (int k = 0; k < 2; ++k) {
    x.fl[k] = dalloc<uint32_t>((size_t)N * x.FC);
    x.fln[k] = dalloc<int32_t>(N);
    if (!denseAny) continue;
    x.fb[k] = dalloc<uint64_t>(NW);
    x.fex[k] = dalloc<int32_t>(E);
    x.fbN[k] = dalloc<int32_t>(N);
  }
  if (denseAny) x.own = dalloc<uint64_t>(NW);
  GS_TRY(allocFail("frontiers"));
  // push arena: a region of GS_PUSHR slots (4 KiB) per owned sender and parity
  for (int k = 0; k < 2 && pushOn; ++k) {
    ibxOwnSlots = (int64_t)std::max<int64_t>(nOwn(), 1) * GS_PUSHR;
    if (ibx[k].reserve((size_t)ibxOwnSlots * 2) != GS_OK) {
      allocFailed = true;
      continue;
    }
    HIPCHECK(hipMemsetAsync(ibx[k].p, 0, (size_t)ibxOwnSlots * 2, stream));
    x.ibx[k] = reinterpret_cast<uint16_t*>(ibx[k].p);
    x.ibxRec[k] = ralloc<int64_t>(0xFF);
  }
  if (pushOn && world > 1) x.pushOvf = dalloc<int32_t>(1);
  return GS_OK;
}

// The small per-node tables, the routers of a mixed network, the promises
// and mcache.peertx.
int gs_engine::allocNodeTables(const Plan& pl) {
  Dev& x = d;
  x.oldm = dalloc<uint64_t>(W);
  x.yTab = dalloc<uint64_t>(2 * (size_t)W);
  x.nAuth = dalloc<int32_t>(N);
  // topic windows (gs_window.h): the lookup tables only where the rings differ
  // in size, the ages only where a topic has its own
  if (!lay.uniform) {
    uint8_t* wt = dalloc<uint8_t>(gsw::kMaxWords);
    uint16_t* w0 = dalloc<uint16_t>((size_t)T + 1);
    GS_TRY(allocFail("topic window tables"));
    GS_TRY(putNow(wt, lay.wTopic.data(), (size_t)gsw::kMaxWords));
    GS_TRY(putNow(w0, lay.w0.data(), (size_t)T + 1));
    x.wTopic = wt;
    x.tW0 = w0;
  }
  if (agesSet()) {
    int32_t* ta = dalloc<int32_t>(T);
    GS_TRY(allocFail("topic age limits"));
    std::vector<int32_t> ah((size_t)T);
    for (int t = 0; t < T; ++t) ah[(size_t)t] = ageOf(t);
    GS_TRY(putNow(ta, ah.data(), (size_t)T));
    x.tAge = ta;
  }
  if (pl.anyRandom) x.sel = dalloc<uint64_t>((size_t)N * S);
  if (mixed) {
    // the hosts' routers (v1.0 folded into gossipsub) and the connections' protocols
    uint8_t* nr = dalloc<uint8_t>(N);
    uint8_t* pr = dalloc<uint8_t>(E);
    std::vector<uint8_t> rh((size_t)N);
    for (int u = 0; u < N; ++u) rh[u] = (uint8_t)routerOf(u);
    GS_TRY(putNow(nr, rh.data(), (size_t)N));
    GS_TRY(putNow(pr, protoH.data(), (size_t)E));
    x.nrouter = nr;
    x.proto = pr;
  }
  x.lastpub = dalloc<int64_t>((size_t)N * T);
  x.fanoutPresent = dalloc<uint64_t>(N);
  x.promMid = nalloc<int64_t>(x.promCap); x.promExp = nalloc<int64_t>(x.promCap);
  x.promSlot = nalloc<int32_t>(x.promCap); x.promEdge = nalloc<uint8_t>(x.promCap);
  x.promN = nalloc<int32_t>(1);
  // mcache.peertx: a hash of 1024 slots per node in HBM.  With IWANT spammers
  // present the honest requests grow too (messages dropped by validation
  // queues come back through gossip; config5 at 1M peers: 43 live entries per
  // node on average, 881 at most), so those runs get 4096; the spammers' own
  // requests, one per (message, spammer), are counted in spamCnt
  // A node whose table fills takes further keys in the rank's overflow table.
  const bool spamRun = (behaveAll & GS_BEHAVE_IWANT_SPAM) != 0;
  x.ptxBits = ptxHomeBits >= 0 ? ptxHomeBits : (spamRun ? 12 : GS_PTX_BITS);
  x.ptxOBits = ptxOvfBits >= 0 ? ptxOvfBits : (spamRun ? 20 : 16);
  {
    // the heartbeat's rebuild stages a node's whole table in LDS: refuse here
    // what the device cannot hold instead of failing that launch
    int lim = 0;
    hipFuncAttributes fa{};
    HIPCHECK(hipDeviceGetAttribute(&lim, hipDeviceAttributeMaxSharedMemoryPerBlock, cfg.device));
    HIPCHECK(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&k_ptx_rebuild)));
    const size_t need = ptx_rebuild_lds(x.ptxBits) + fa.sharedSizeBytes;
    if (need > (size_t)lim) {
      gs_set_error("gs_set_peertx_capacity: home_bits " + std::to_string(x.ptxBits) + " needs " + std::to_string(need) +
                   " bytes of LDS per workgroup for the heartbeat's peertx rebuild, the device has " +
                   std::to_string(lim) + ": lower home_bits");
      return GS_ECAPACITY;
    }
  }
  x.ptxT = nalloc<uint32_t>((size_t)1 << x.ptxBits);
  x.ptxN = nalloc<int32_t>(1);
  x.ptxO = dalloc<unsigned long long>((size_t)1 << x.ptxOBits);
  x.ptxOStage = dalloc<unsigned long long>((size_t)1 << x.ptxOBits);
  x.ptxOCnt = dalloc<unsigned int>(4);
  GS_TRY(allocFail("promises / peertx"));
  std::vector<int64_t> lp((size_t)N * T, INT64_MIN);
  return putNow(x.lastpub, lp.data(), lp.size());
}

// Per-edge and per-(edge, topic) state of the owned edges.
int gs_engine::allocEdgeState() {
  Dev& x = d;
  x.mesh = ealloc<uint64_t>(); x.fanout = ealloc<uint64_t>();
  for (int k = 0; k < 2; ++k) {
    x.fwdRelay[k] = ealloc<uint64_t>(); x.fwdPub[k] = ealloc<uint64_t>();
    x.fwdIn[k] = ralloc<ulonglong2>();
    x.cPre[k] = ralloc<uint8_t>(); x.cHb[k] = ralloc<uint8_t>();
    x.cGraftJoin[k] = ralloc<uint64_t>(); x.cGraftHb[k] = ralloc<uint64_t>();
    x.cPruneReply[k] = ralloc<uint64_t>(); x.cPruneHb[k] = ralloc<uint64_t>();
    x.cIhave[k] = ralloc<uint64_t>();
    x.cIwant[k] = ralloc<int64_t>(0xFF); x.cIresp[k] = ralloc<int64_t>(0xFF);
    x.pubmask[k] = dalloc<uint64_t>(W);
  }
  x.score0 = ealloc<double>(); x.score1 = ealloc<double>();
  x.sdirty = ealloc<uint8_t>(1);
  x.backoff = palloc<int64_t>();
  x.boMask = ealloc<uint64_t>();
  x.fmd = palloc<double>(); x.mmd = palloc<double>(); x.mfp = palloc<double>(); x.imd = palloc<double>();
  // 16-bit pending counts when a topic's slots (at most St + 1 messages live at
  // one hop) fit a byte and the pairs of an edge pack into whole words
  narrowDlt = St <= 254 && (T % 2) == 0;  // (St: the largest topic's)
  if (narrowDlt) x.dltN = palloc<uint16_t>();
  else x.dlt = palloc<uint32_t>();
  x.graftTime = palloc<int64_t>(); x.meshTime = palloc<int64_t>(); x.flags = palloc<uint8_t>();
  GS_TRY(allocFail("per-(edge, topic) state"));
  x.bp = ealloc<double>(); x.peerhave = ealloc<int32_t>(); x.iasked = ealloc<int32_t>();
  return GS_OK;
}

// IWANT payload arena (slot ids): 4 ids per owned edge per hop, >= 16M in
// total; rank r allocates from its own segment [r*seg, (r+1)*seg).  Then the
// MaxIHaveLength cut spill, the PX queue and the per-slot message records.
int gs_engine::allocIwantPool() {
  Dev& x = d;
  poolSeg = cfg.router == GS_ROUTER_GOSSIPSUB ? std::max<int64_t>((1 << 24) / world, 4 * eOwn) : 16;
  poolSeg = (poolSeg + 63) & ~63ll;
  x.poolCap = (int64_t)(rank + 1) * poolSeg;
  // sub-arenas of at least 2^20 ids (one counter each) on an unpartitioned
  // engine; a partitioned one keeps one counter so its used ids stay one
  // prefix of its segment (the exchange ships that prefix)
  int sub = 1;
  while (world == 1 && sub < 256 && (poolSeg / (2 * sub)) >= (1 << 20)) sub *= 2;
  x.poolSub = sub;
  x.poolSubCap = poolSeg / sub;
  x.poolBase0 = (int64_t)rank * poolSeg;
  x.poolS0Mask = -1;
  // tests only: small sub-arenas, every node trying sub-arena 0 first, so
  // allocations fill it and spill into the next ones (tests/test_parity_gpu.py)
  if (const char* dbg = std::getenv("GS_DEBUG_POOL_SUB_CAP"))
    if (world == 1) {
      x.poolSubCap = std::min<int64_t>(x.poolSubCap, std::max<long long>(1, std::atoll(dbg)));
      x.poolS0Mask = 0;
      // never silent: it changes the arena's capacity and allocation order
      std::fprintf(stderr, "gossip engine: GS_DEBUG_POOL_SUB_CAP=%s active (IWANT sub-arenas of %lld ids, "
                   "sub-arena 0 first; a test-only setting)\n", dbg, (long long)x.poolSubCap);
    }
  for (int k = 0; k < 2; ++k) x.pool[k] = dalloc<int32_t>((size_t)poolSeg * world);
  x.poolCnt = dalloc<unsigned long long>((size_t)2 * x.poolSub * 16);
  x.cutSpK = dalloc<unsigned long long>(GS_CUTSPILL); x.cutSpM = dalloc<int64_t>(GS_CUTSPILL);
  x.cutSpN = dalloc<unsigned long long>(1);
  if (doPX) {
    for (int k = 0; k < 2; ++k) x.cPx[k] = ralloc<int64_t>(0xFF);
    x.pxqCap = std::max<int64_t>(1 << 16, 4 * (int64_t)N);
    x.pxq = dalloc<unsigned long long>((size_t)x.pxqCap); x.pxqN = dalloc<unsigned long long>(1);
  }
  x.slotSrc = dalloc<int32_t>(S, 0xFF); x.slotPubHop = dalloc<int64_t>(S); x.slotMid = dalloc<int64_t>(S, 0xFF);
  x.slotKind = dalloc<uint8_t>(S);
  return GS_OK;
}

// Adversarial model: the nodes' behaviour bits and the IWANT spammers' tables.
int gs_engine::allocAdversary(const Plan& pl) {
  Dev& x = d;
  if (!behaveAll) return GS_OK;
  uint8_t* b = dalloc<uint8_t>(N);
  GS_TRY(putNow(b, behaveH.data(), (size_t)N));
  x.behave = b;
  if (!(behaveAll & GS_BEHAVE_IWANT_SPAM)) return GS_OK;
  for (int k = 0; k < 2; ++k) {
    x.cSpam[k] = ralloc<int64_t>(0xFF);
    x.cNSrv[k] = ralloc<uint8_t>();
  }
  x.pmaskRow = dalloc<int32_t>(N);
  x.pmask = dalloc<uint64_t>((size_t)pl.nSpam * S);
  x.spamRow = ealloc<int32_t>();
  for (int k = 0; k < 2; ++k) x.pflag[k] = dalloc<uint8_t>((size_t)poolSeg * world);
  x.spamCnt = dalloc<uint32_t>((size_t)std::max<int64_t>(pl.nSpamEdges, 1) * (S / 8));
  GS_TRY(putNow(x.pmaskRow, pl.pmaskRowH.data(), (size_t)N));
  return putEdges(x.spamRow, spamRowH);
}

int gs_engine::allocGater(const Plan& pl) {
  Dev& x = d;
  if (!gaterOn) return GS_OK;
  x.gThreshold = gaterP.Threshold; x.gGlobalDecay = gaterP.GlobalDecay; x.gSourceDecay = gaterP.SourceDecay;
  x.gDecayToZero = gaterP.DecayToZero; x.gDupW = gaterP.DuplicateWeight; x.gIgnW = gaterP.IgnoreWeight;
  x.gRejW = gaterP.RejectWeight; x.gQuiet = gaterP.Quiet;
  x.gValidate = dalloc<double>(N); x.gThrottle = dalloc<double>(N); x.gLast = dalloc<int64_t>(N);
  // gSt: [4][eOwn] through the e0-shifted base, stat k of edge e at k * eOwn + e
  x.gSt = ealloc<double>(0, 4);
  x.gGrp = ealloc<uint8_t>();
  x.gConn = ealloc<int32_t>(); x.gExp = ealloc<int64_t>();
  // peers of one IP share a stats object (peer_gater.go:262-280); getIP = ipv4, 0 = "<unknown>"
  std::vector<uint8_t> grp(E);
  for (int u = 0; u < N; ++u)
    for (int64_t e = rowptr[u]; e < rowptr[u + 1]; ++e) {
      const uint32_t ip = ipv4.empty() ? 0u : ipv4[col[e]];
      int64_t f = rowptr[u];
      while ((ipv4.empty() ? 0u : ipv4[col[f]]) != ip) ++f;
      grp[e] = (uint8_t)(f - rowptr[u]);
    }
  std::vector<int64_t> never(N, INT64_MIN);
  // connected peers per stats object (AddPeer of every connection up at the start)
  std::vector<int32_t> conn((size_t)E, 0);
  for (int u = 0; u < N; ++u)
    for (int64_t e = rowptr[u]; e < rowptr[u + 1]; ++e)
      if (!pl.isDown(e)) conn[rowptr[u] + grp[e]]++;
  GS_TRY(putEdges(x.gConn, conn));
  GS_TRY(putEdges(x.gGrp, grp));
  return putNow(x.gLast, never.data(), (size_t)N);
}

// Scratch, counters, the error word and the readback buffers.
int gs_engine::allocReadback() {
  Dev& x = d;
#ifdef GS_STAMPS
  x.stamps = dalloc<unsigned long long>((size_t)(N / 1024 + 1) * 24);  // phase A | phase B | heartbeat
#endif
  x.pad = dalloc<double>(256 * 64 * 2);
  x.ctr = dalloc<unsigned long long>((size_t)C_NCOUNTERS * GS_CTR_SPREAD); x.err = dalloc<int32_t>(1);
  dScoreTmp = ealloc<double>();
  dHopOut = dalloc<int32_t>(N); dFromOut = dalloc<int32_t>(N);
  return GS_OK;
}

// Latency statistics (gs_latency.h), at their exact sizes: S + S * bins
// uint32 and T * bins uint64.
int gs_engine::allocLatency() {
  if (!lat.on) return GS_OK;
  const size_t bins = (size_t)latBins();
  d.latCnt = dalloc<uint32_t>((size_t)S);
  lat.dev.perMsg = dalloc<uint32_t>((size_t)S * bins);
  lat.dev.hist = dalloc<unsigned long long>((size_t)T * bins);
  // k_lat_count's grid: as many workgroups per CU as its LDS holds of their 4 S byte tables,
  // GS_LAT_WGS_PER_CU at the most (a workgroup that is not resident only runs as a tail)
  const unsigned fit = (unsigned)(GS_LAT_CU_LDS / std::max<size_t>((size_t)S * 4, 1));
  lat.dev.grid = std::min<unsigned>(std::max(fit, 1u), GS_LAT_WGS_PER_CU) * cus;
  return GS_OK;
}

// WithPeerScoreInspect (gs_inspect.h): the sampled edges (the out-edges of the
// owned observers, ascending), the ring at its exact size and
// k_inspect_reduce's grid.
int gs_engine::allocInspect() {
  if (!insp.tk.on) return GS_OK;
  auto& v = insp.dev;
  v.edges.clear();
  if (!insp.mask.empty())
    for (int u = n0; u < n1; ++u)
      if (insp.mask[u])
        for (int64_t e = rowptr[u]; e < rowptr[u + 1]; ++e) v.edges.push_back(e);
  const size_t nS = v.edges.size(), cap = (size_t)insp.tk.cap, nb = insp.bounds.size();
  GS_TRY(allocGroup("score inspection ring", "; reduce ticks or the sampled nodes", [&] {
    v.rows = dalloc<unsigned long long>(cap * (size_t)inspRowLen());
    v.bounds = dalloc<double>(std::max<size_t>(nb, 1));
    if (nS) {
      v.edgeList = dalloc<int64_t>(nS);
      v.score = dalloc<double>(cap * nS);
      if (insp.ext) v.ext = dalloc<double>(cap * inspExtLen());
    }
  }));
  GS_TRY(put(v.bounds, insp.bounds.data(), nb));
  GS_TRY(putNow(v.edgeList, v.edges.data(), nS));
  // k_inspect_reduce's grid: as many workgroups per CU as its LDS holds of their tables,
  // GS_INSP_WGS_PER_CU at the most (a workgroup that is not resident only runs as a tail)
  const unsigned fit = (unsigned)(GS_INSP_CU_LDS / insp_lds_bytes((int)nb, T));
  v.grid = std::min<unsigned>(std::max(fit, 1u), GS_INSP_WGS_PER_CU) * cus;
  return GS_OK;
}

// A tick at the end of a hop (`hop` already counts it): the exact scores as
// gs_read_scores computes them, then the row and the sampled edges into the
// tick's ring slot.  Nothing is read back: the host knows a tick's hop.
int gs_engine::inspectTick() {
  const auto& v = insp.dev;
  const size_t slot = insp.tk.slot();
  const int nb = (int)insp.bounds.size();
  const int64_t nS = (int64_t)v.edges.size();
  unsigned long long* row = v.rows + slot * inspRowLen();
  HIPCHECK(hipMemsetAsync(row, 0, (size_t)inspRowLen() * 8, stream));
  TIMED(this, kInspScore, (score_rows<0>(d, eOwn, T, dScoreTmp, stream)));
  if (nOwn()) {
    const unsigned grid = std::min(v.grid, nblk(nOwn(), GS_INSP_BLOCK / 64));
    TIMED(this, kInspReduce, (k_inspect_reduce<<<grid, GS_INSP_BLOCK, insp_row_lds(nb, T), stream>>>(
                                 d, dScoreTmp, v.bounds, nb, row)));
  }
  if (nS) {
    double* ext = insp.ext ? v.ext + slot * inspExtLen() : nullptr;
    TIMED(this, kInspGather, (k_inspect_gather<<<nblk(nS * T, 256), 256, 0, stream>>>(
                                 d, v.edgeList, nS, dScoreTmp, v.score + slot * nS, ext)));
  }
  HIPCHECK(hipGetLastError());
  return GS_OK;
}

// Mesh health (gs_mesh_health.h) at its exact sizes: the two [N][T] tables, the
// ring of rows, the include mask, a batch's flags and the word counter; the
// grid of the three node passes.
int gs_engine::allocMeshHealth() {
  if (!mesh.tk.on) return GS_OK;
  auto& v = mesh.dev;
  const size_t nt = (size_t)N * (size_t)T;
  GS_TRY(allocGroup("mesh health tables", "; reduce ticks or num_nodes", [&] {
    v.L = dalloc<uint32_t>(nt);
    v.Z = dalloc<uint32_t>(nt);
    v.rows = dalloc<unsigned long long>((size_t)mesh.tk.cap * (size_t)mesh_row_len(T));
    v.flag = dalloc<uint32_t>(GS_MESH_BATCH + 1);
    v.words = dalloc<unsigned long long>(1);
    if (!mesh.mask.empty()) v.mask = dalloc<uint8_t>((size_t)N);
  }));
  GS_TRY(putNow(v.mask, mesh.mask.data(), mesh.mask.size()));
  v.grid = std::min<unsigned>(GS_MESH_WGS_PER_CU * cus, std::max(nblk(mesh_groups(N, T), GS_MESH_BLOCK / 64), 1u));
  return GS_OK;
}

// A tick at the end of a hop (`hop` already counts it): labels to their fixed
// point in batches of GS_MESH_BATCH iterations (runBatched: an iteration that
// had work ran; the labels have settled when one lowers nothing), at most N
// iterations in all; then the sizes and the row.  The byte count: what every
// pass streams, from the shapes, plus the label words the kernels counted.
int gs_engine::meshTick() {
  const auto& v = mesh.dev;
  unsigned long long* row = v.rows + mesh.tk.slot() * (size_t)mesh_row_len(T);
  const int64_t nt = (int64_t)N * T;
  const bool wide = mesh_tp(T) == 64;
  HIPCHECK(hipMemsetAsync(row, 0, (size_t)mesh_row_len(T) * 8, stream));
  HIPCHECK(hipMemsetAsync(v.words, 0, 8, stream));
  TIMED(this, kMeshInit + GS_MESH_K_INIT, (k_mesh_init<<<nblk(nt, 256), 256, 0, stream>>>(d, v.mask, v.L, v.Z)));
  int64_t iters = 0;
  GS_TRY(runBatched(GS_MESH_BATCH, v.flag, N, "mesh health: labels did not converge after ", " iterations",
                    [&](int i, int64_t) {
                      with_consts([&](auto w) {
                        TIMED(this, kMeshInit + GS_MESH_K_LABEL,
                              (k_mesh_label<CV(w)><<<v.grid, GS_MESH_BLOCK, 0, stream>>>(d, v.L, v.flag + i, v.words)));
                      }, Flag{wide});
                    }, &iters));
  TIMED(this, kMeshInit + GS_MESH_K_SIZES, (k_mesh_sizes<<<v.grid, GS_MESH_BLOCK, 0, stream>>>(d, v.L, v.Z, v.words)));
  with_consts([&](auto w) {
    TIMED(this, kMeshInit + GS_MESH_K_ROW,
          (k_mesh_row<CV(w)><<<v.grid, GS_MESH_BLOCK, 0, stream>>>(d, v.mask, v.L, v.Z, row)));
  }, Flag{wide});
  HIPCHECK(hipGetLastError());
  unsigned long long words = 0;
  HIPCHECK(hipMemcpyAsync(&words, v.words, 8, hipMemcpyDeviceToHost, stream));
  HIPCHECK(hipStreamSynchronize(stream));
  // per edge: mesh word, reverse edge, peer, the reverse edge's mesh word (the
  // row pass: the peer's include byte too); per node: its CSR row bounds
  const int64_t edgeWalk = E * (8 + 4 + 4 + 8) + (int64_t)N * 8;
  mesh.iters += iters;
  mesh.bytes += nt * 8 + (int64_t)N * 10          // init: two stores; the subscription word, router and include bytes
                + iters * (edgeWalk + nt * 4)     // an iteration: the edges and the nodes' own labels
                + nt * 4                          // sizes: every label
                + nt * 4 + edgeWalk + E           // row: every label, the edges
                + (int64_t)words * 4;             // what the label and size passes counted besides
  return GS_OK;
}

// Bandwidth statistics (gs_bandwidth.h) at their exact sizes: the split
// counters of every edge, the two per-node tables, the ring of rows and of the
// sampled nodes' values; k_bw_tick's grid.  After allocAcct: the counters
// start at zero, as the hello packets are overhead.
int gs_engine::allocBandwidth() {
  if (!bw.tk.on) return GS_OK;
  auto& v = bw.dev;
  const size_t nS = bw.nodes.size(), cap = (size_t)bw.tk.cap, nb = bw.bounds.size();
  GS_TRY(allocGroup("bandwidth statistics", "; reduce ticks or the sampled nodes", [&] {
    d.bwX = ealloc<unsigned long long>(0, 2);
    v.prev = dalloc<unsigned long long>((size_t)N * GS_BW_NODE_WORDS);
    v.delta = dalloc<unsigned long long>((size_t)N * GS_BW_NODE_WORDS);
    v.rows = dalloc<unsigned long long>(cap * (size_t)bwRowLen());
    v.bounds = dalloc<long long>(std::max<size_t>(nb, 1));
    if (nS) {
      v.nodes = dalloc<int32_t>(nS);
      v.bytes = dalloc<unsigned long long>(cap * nS * GS_BW_NODE_WORDS);
      v.rpcs = dalloc<unsigned long long>(cap * nS * GS_BW_DIRS);
    }
  }));
  GS_TRY(put(v.bounds, reinterpret_cast<const long long*>(bw.bounds.data()), nb));
  GS_TRY(putNow(v.nodes, bw.nodes.data(), nS));
  v.grid = GS_BW_WGS_PER_CU * cus;
  return GS_OK;
}

// A tick at the end of a hop (`hop` already counts it): the row and the
// sampled nodes into the tick's ring slot.  Nothing is read back: the host
// knows a tick's hop.
int gs_engine::bandwidthTick() {
  const auto& v = bw.dev;
  const size_t slot = bw.tk.slot();
  const int64_t nS = (int64_t)bw.nodes.size();
  unsigned long long* row = v.rows + slot * bwRowLen();
  HIPCHECK(hipMemsetAsync(row, 0, (size_t)bwRowLen() * 8, stream));
  HIPCHECK(hipMemsetAsync(row + GS_BW_ROW_ARG, 0xFF, (size_t)GS_BW_DIRS * GS_BW_CLASSES * 8, stream));  // -1: no node
  if (nOwn()) {
    const unsigned grid = std::min(v.grid, nblk(nOwn(), GS_BW_BLOCK / 64));
    TIMED(this, kBwTick + GS_BW_K_TICK, (k_bw_tick<<<grid, GS_BW_BLOCK, 0, stream>>>(
                                            d, v.bounds, (int)bw.bounds.size(), v.prev, v.delta, row)));
    TIMED(this, kBwTick + GS_BW_K_ARGMAX,
          (k_bw_argmax<<<nblk((int64_t)nOwn() * GS_BW_NODE_WORDS, 256), 256, 0, stream>>>(d, v.delta, row)));
  }
  if (nS)
    TIMED(this, kBwTick + GS_BW_K_GATHER,
          (k_bw_gather<<<nblk(nS * GS_BW_NODE_WORDS, 256), 256, 0, stream>>>(
              v.nodes, nS, v.delta, v.bytes + slot * nS * GS_BW_NODE_WORDS, v.rpcs + slot * nS * GS_BW_DIRS)));
  HIPCHECK(hipGetLastError());
  return GS_OK;
}

// Mesh reach (gs_mesh_reach.h) at its exact sizes: the two bit tables, the ring
// of rows, the sources, the include mask, the members per topic, a batch's
// flags, the byte counters and, when asked for, the depth table; the grid of
// the node passes (mesh health's).
int gs_engine::allocMeshReach() {
  if (!reach.tk.on) return GS_OK;
  auto& v = reach.dev;
  const size_t nt = (size_t)N * (size_t)T, K = reach.src.size();
  GS_TRY(allocGroup("mesh reach tables", "; reduce ticks, num_sources or num_nodes, or drop depths", [&] {
    v.R[0] = dalloc<uint64_t>(nt);
    v.R[1] = dalloc<uint64_t>(nt);
    v.rows = dalloc<unsigned long long>((size_t)reach.tk.cap * (size_t)reach_row_len((int)K, T));
    v.src = dalloc<int32_t>(K);
    v.members = dalloc<uint32_t>((size_t)T);
    v.flag = dalloc<uint32_t>(GS_REACH_BATCH + 1);
    v.words = dalloc<unsigned long long>(GS_REACH_W_NUM);
    if (!reach.mask.empty()) v.mask = dalloc<uint8_t>((size_t)N);
    if (reach.depths) v.depths = dalloc<uint8_t>(K * nt, 0xFF);
  }));
  GS_TRY(put(v.src, reach.src.data(), K));
  GS_TRY(putNow(v.mask, reach.mask.data(), reach.mask.size()));
  v.grid = std::min<unsigned>(GS_MESH_WGS_PER_CU * cus, std::max(nblk(mesh_groups(N, T), GS_MESH_BLOCK / 64), 1u));
  return GS_OK;
}

// A tick at the end of a hop (`hop` already counts it), after the other
// inspectors': the members once, then a pass per 64 sources.  A pass clears R0,
// sets its sources' bits and runs the levels in batches of GS_REACH_BATCH
// (runBatched: the search has ended when a level sets nothing), level L reading
// R[(L - 1) & 1] and writing R[L & 1], at most N levels per pass.  The byte
// count: what every kernel streams, from the shapes, plus what the level
// kernel counted.
int gs_engine::reachTick() {
  const auto& v = reach.dev;
  const int K = (int)reach.src.size();
  const int64_t nt = (int64_t)N * T;
  unsigned long long* row = v.rows + reach.tk.slot() * (size_t)reach_row_len(K, T);
  unsigned long long* hist = row + (size_t)K * T * GS_REACH_ROW_FIELDS;
  const bool wide = mesh_tp(T) == 64;
  HIPCHECK(hipMemsetAsync(row, 0, (size_t)reach_row_len(K, T) * 8, stream));
  HIPCHECK(hipMemsetAsync(v.words, 0, GS_REACH_W_NUM * 8, stream));
  HIPCHECK(hipMemsetAsync(v.members, 0, (size_t)T * 4, stream));
  if (reach.depths) HIPCHECK(hipMemsetAsync(v.depths, 0xFF, (size_t)K * (size_t)nt, stream));
  TIMED(this, kReachMembers + GS_REACH_K_MEMBERS,
        (k_reach_members<<<v.grid, GS_MESH_BLOCK, 0, stream>>>(d, v.mask, v.members)));
  int64_t levels = 0;
  int passes = 0;
  for (int k0 = 0; k0 < K; k0 += 64, ++passes) {
    const int ns = std::min(64, K - k0);
    const uint64_t full = ns == 64 ? ~0ull : (1ull << ns) - 1ull;
    unsigned long long* prow = row + (size_t)k0 * T * GS_REACH_ROW_FIELDS;
    unsigned long long* phist = hist + (size_t)k0 * T * GS_REACH_DEPTH_BINS;
    uint8_t* pdepths = reach.depths ? v.depths + (size_t)k0 * (size_t)nt : nullptr;
    HIPCHECK(hipMemsetAsync(v.R[0], 0, (size_t)nt * 8, stream));
    TIMED(this, kReachMembers + GS_REACH_K_INIT,
          (k_reach_init<<<nblk((int64_t)ns * T, 256), 256, 0, stream>>>(d, v.src + k0, ns, v.R[0], pdepths)));
    int64_t ran = 0;
    GS_TRY(runBatched(GS_REACH_BATCH, v.flag, N, "mesh reach: levels did not end after ", "",
                      [&](int i, int64_t before) {
                        // (a launch past the search's end returns at once: its level is not used)
                        const int level = (int)before + i + 1;
                        with_consts([&](auto w) {
                          TIMED(this, kReachMembers + GS_REACH_K_LEVEL,
                                (k_reach_level<CV(w)><<<v.grid, GS_MESH_BLOCK, 0, stream>>>(
                                    d, v.mask, v.R[(level - 1) & 1], v.R[level & 1], full, level, v.flag + i, prow,
                                    phist, pdepths, v.words)));
                        }, Flag{wide});
                      }, &ran));
    TIMED(this, kReachMembers + GS_REACH_K_FINISH,
          (k_reach_finish<<<nblk((int64_t)ns * T, 256), 256, 0, stream>>>(d, v.mask, v.src + k0, ns, v.members, prow)));
    levels += ran;
  }
  HIPCHECK(hipGetLastError());
  unsigned long long words[GS_REACH_W_NUM];
  HIPCHECK(hipMemcpyAsync(words, v.words, sizeof words, hipMemcpyDeviceToHost, stream));
  HIPCHECK(hipStreamSynchronize(stream));
  reach.passes += passes;
  reach.levels += levels;
  reach.bytes += (int64_t)N * 10                                   // members: the subscription word, router and include bytes
                 + (reach.depths ? (int64_t)K * nt : 0)            // the depth table's fill
                 + passes * nt * 8 + (int64_t)K * T * (4 + 8)      // a pass's cleared table, its sources' words
                 + levels * (nt * 16 + (int64_t)N * (10 + 8))      // a level: both tables, the member test, the CSR row bounds
                 + (int64_t)words[GS_REACH_W_GATHER] * 8           // the neighbours' words gathered
                 + (int64_t)words[GS_REACH_W_EDGES] * (8 + 8 + 4 + 4)  // per edge walked: mesh and fanout of the reverse edge, it, the peer
                 + (int64_t)words[GS_REACH_W_DEPTHS]               // depth bytes stored
                 + (int64_t)K * T * (GS_REACH_ROW_T + 1) * 8;      // the row: cleared, UNREACHED
  return GS_OK;
}

int gs_engine::allocTrace() {
  Dev& x = d;
  if (traceMask.empty()) return GS_OK;
  uint8_t* tm = dalloc<uint8_t>(N);
  x.trace = dalloc<gs_trace_event>((size_t)traceCap);
  x.traceN = dalloc<unsigned long long>(1);
  x.traceCap = traceCap;
  GS_TRY(putNow(tm, traceMask.data(), (size_t)N));
  x.traced = tm;
  // AddPeer (gossipsub.go:507, floodsub.go:45) and Join (gossipsub.go:1018,
  // floodsub.go:103) of the traced hosts at time 0, recorded on the host
  for (int u = n0; u < n1; ++u) {
    if (!traceMask[u]) continue;
    auto up = [&](int64_t e) { return !dormant.count({std::min(u, col[e]), std::max(u, col[e])}); };
    for (int64_t e = rowptr[u]; e < rowptr[u + 1]; ++e)
      if (up(e))  // the connection's protocol in `reason` on a mixed network
        tracePending.push_back(gs_trace_event{0, -1, GS_TRACE_ADD_PEER, u, col[e], -1, 0, mixed ? protoH[e] : (uint8_t)0});
    for (int t = 0; t < T; ++t)
      if ((sub[u] >> t) & 1) tracePending.push_back(gs_trace_event{0, -1, GS_TRACE_JOIN, u, -1, (int16_t)t, 0, 0});
    // the hello packet of every peer (pubsub.go:495; its RecvRPC at time 0)
    for (int64_t e = rowptr[u]; e < rowptr[u + 1]; ++e)
      if (up(e)) hostRpc(GS_TRACE_RECV_RPC, u, col[e], 0, GS_RPC_ORD(0, GS_RPC_O_HELLO), -1, sub[col[e]], 1);
  }
  return GS_OK;
}

int gs_engine::allocPartition() {
  Dev& x = d;
  if (world == 1) return GS_OK;
  x.xmark = ealloc<uint8_t>();
  uint8_t* nr = dalloc<uint8_t>(N);
  xCnt = dalloc<unsigned long long>(gsx::XCnt::words(world));
  xOff = dalloc<int64_t>(world);
  xpCnt = dalloc<unsigned long long>(gsx::XpCnt::words(world));
  xpOff = dalloc<int64_t>(gsx::XpOff::words(world));
  std::vector<uint8_t> h(N);
  for (int r = 0; r < world; ++r)
    for (int v = part[r]; v < part[r + 1]; ++v) h[v] = (uint8_t)r;
  GS_TRY(putNow(nr, h.data(), (size_t)N));
  x.nodeRank = nr;
  HIPCHECK(hipHostMalloc((void**)&xHost, gsx::Readback::words(world) * 8, hipHostMallocDefault));
  return GS_OK;
}

// Churn state where the run needs it, and the connections that start down.
int gs_engine::initConnections(const Plan& pl) {
  if (!events.empty() || doPX || !dormant.empty()) GS_TRY(enableChurn());
  if (dormant.empty()) return GS_OK;
  // gs_set_dormant: these connections start down, without a score record
  std::vector<uint8_t> al((size_t)E, 1);
  for (int64_t e = 0; e < E; ++e)
    if (pl.downH[e]) al[e] = aliveH[e] = 0;
  GS_TRY(putNow(d.alive, al.data(), (size_t)E));
  if (d.rstate) GS_TRY(putNow(d.rstate, al.data(), (size_t)E));
  return GS_OK;
}

int gs_engine::allocAcct(const Plan& pl) {
  Dev& x = d;
  if (!acctOn) return GS_OK;
  // partitioned: every RPC is counted by its sender's rank, on the sender's
  // (owned) edge; gs_read_rpc_bytes returns the owned edges
  x.rpcB = ealloc<unsigned long long>(); x.rpcN = ealloc<unsigned long long>();
  AcctT* ac = dalloc<AcctT>(T);
  GS_TRY(allocFail("RPC accounting"));
  const uint64_t bo = (uint64_t)(gp.PruneBackoff / kSec);
  std::vector<AcctT> ah(T);
  for (int t = 0; t < T; ++t) {
    ah[t].msgF = (int32_t)gs_pb_field(acctMsg[t]);
    ah[t].graftEnt = (int32_t)gs_pb_field(gs_pb_graft(acctTl[t]));
    ah[t].pruneBody = (int32_t)gs_pb_prune(acctTl[t], bo);
    ah[t].pruneEnt10 = (int32_t)gs_pb_field(gs_pb_prune_v10(acctTl[t]));
    ah[t].ihaveHead = (int32_t)gs_pb_field(acctTl[t]);
  }
  x.acctIdF = (int32_t)gs_pb_field(acctIdLen);
  x.acctPiF = (int32_t)gs_pb_field(gs_pb_peerinfo(acctPidLen, acctRecLen));
  // the hello packet of every connection present at the start (pubsub.go:495)
  std::vector<unsigned long long> hb((size_t)E), hn((size_t)E, 1ull);
  for (int u = 0; u < N; ++u)
    for (int64_t e = rowptr[u]; e < rowptr[u + 1]; ++e) {
      hb[e] = pl.isDown(e) ? 0ull : (unsigned long long)helloBytes(sub[u]);
      hn[e] = pl.isDown(e) ? 0ull : 1ull;
    }
  GS_TRY(putNow(ac, ah.data(), (size_t)T));
  GS_TRY(putEdges(x.rpcB, hb));
  GS_TRY(putEdges(x.rpcN, hn));
  x.acc = ac;
  return GS_OK;
}

// host-side RPCs of this hop (hello packets, subscription announcements): one
// (edge, bytes) pair each, added on the device
int gs_engine::flushAcct() {
  if (world > 1) {  // a partitioned rank counts what its own nodes send
    size_t k = 0;
    for (size_t i = 0; i + 1 < acctPend.size(); i += 2)
      if (acctPend[i] >= e0 && acctPend[i] < e1) {
        acctPend[k++] = acctPend[i];
        acctPend[k++] = acctPend[i + 1];
      }
    acctPend.resize(k);
  }
  if (acctPend.empty()) return GS_OK;
  GS_TRY(acctBuf.reserve(acctPend.size()));
  GS_TRY(putNow(acctBuf.p, acctPend.data(), acctPend.size()));
  const int n = (int)(acctPend.size() / 2);
  k_acct_add<<<nblk(n, 256), 256, 0, stream>>>(d, acctBuf.p, n);
  acctPend.clear();
  return GS_OK;
}

// The messages published since the last call go to the device; when the five
// arrays had to grow, the kernels get the new addresses and every message is
// uploaded again.
int gs_engine::uploadMessages() {
  if (!started) return GS_OK;
  const size_t n = mSrc.size();
  if (n == uploaded) return GS_OK;
  if (n > msgSrc.cap) {
    GS_TRY(msgKind.reserve(n));
    GS_TRY(msgSrc.reserve(n));
    GS_TRY(msgTopic.reserve(n));
    GS_TRY(msgSlot.reserve(n));
    GS_TRY(msgId.reserve(n));
    d.mKind = msgKind.p; d.mSrc = msgSrc.p; d.mTopic = msgTopic.p; d.mSlot = msgSlot.p; d.mId = msgId.p;
    uploaded = 0;
  }
  const size_t k = n - uploaded;
  GS_TRY(put(d.mSrc + uploaded, mSrc.data() + uploaded, k));
  GS_TRY(put(d.mTopic + uploaded, mTopic.data() + uploaded, k));
  GS_TRY(put(d.mSlot + uploaded, mSlot.data() + uploaded, k));
  GS_TRY(put(d.mId + uploaded, mId.data() + uploaded, k));
  GS_TRY(putNow(d.mKind + uploaded, mKind.data() + uploaded, k));
  uploaded = n;
  return GS_OK;
}

// Connection churn state (gs_schedule_events): connection flags, score-record
// states and the P6 inputs, allocated on the first scheduled event.
int gs_engine::enableChurn() {
  if (churnOn) return GS_OK;
  if (denseFlood) {  // (its frontiers carry no per-copy lists to replay a lost connection from)
    gs_set_error("floodsub connection churn must be scheduled before the first step");
    return GS_EUNSUPPORTED;
  }
  auto* al = dalloc<uint8_t>(E, 1);
  auto* rs = scoring ? dalloc<uint8_t>(E, 1) : nullptr;
  auto* rx = scoring ? dalloc<int64_t>(E) : nullptr;
  auto* ip = dalloc<uint32_t>(N);
  auto* wl = dalloc<uint8_t>(N);
  GS_TRY(allocFail("churn state"));
  std::vector<uint32_t> iph(N, 0);
  std::vector<uint8_t> wlh(N, 0);
  for (int v = 0; v < N; ++v) {
    iph[v] = ipv4.empty() ? 0u : ipv4[v];
    for (auto& nm : whitelist)
      if ((iph[v] & nm.second) == (nm.first & nm.second)) { wlh[v] = 1; break; }
  }
  GS_TRY(put(ip, iph.data(), (size_t)N));
  GS_TRY(putNow(wl, wlh.data(), (size_t)N));
  d.alive = al; d.rstate = rs; d.rexpire = rx; d.ipv4 = ip; d.ipWL = wl;
  aliveH.assign((size_t)E, 1);
  churnOn = true;
  return GS_OK;
}

// The peer-exchange dial requests of this hop (v << 32 | peer), for the next
// hop's applyEvents.
int gs_engine::readPx() {
  unsigned long long n = 0;
  HIPCHECK(hipMemcpyAsync(&n, d.pxqN, 8, hipMemcpyDeviceToHost, stream));
  HIPCHECK(hipStreamSynchronize(stream));
  n = std::min<unsigned long long>(n, (unsigned long long)d.pxqCap);
  if (n) {
    pxqH.resize(n);
    HIPCHECK(hipMemcpyAsync(pxqH.data(), d.pxq, n * 8, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipMemsetAsync(d.pxqN, 0, 8, stream));
    HIPCHECK(hipStreamSynchronize(stream));
    for (unsigned long long x : pxqH) {
      const int a = (int)(x >> 32), b = (int)(x & 0xFFFFFFFFu);
      pxPend.push_back({std::min(a, b), std::max(a, b)});
    }
  }
  return GS_OK;
}

int gs_engine::uploadList(const std::vector<int32_t>& v) {
  GS_TRY(evBuf.reserve(v.size()));
  return upload(evBuf.p, v.data(), v.size() * 4);
}

// The events of hop h, at its start (the oracle's Sim::applyEvents): the
// announcements of hop h - 1 reach the peers, then every disconnect, connect,
// leave and join of hop h in that order.
int gs_engine::applyEvents(int64_t h) {
  const int64_t now = h * cfg.hop_ns;
  const int cur = (int)(h & 1), prv = cur ^ 1;
  bool subAChanged = false, subChanged = false;
  for (const Ann& an : pendAnn) {
    if (traceRpc)  // RecvRPC of the announcement at every still-connected peer
      for (int64_t e = rowptr[an.node]; e < rowptr[an.node + 1]; ++e)
        if (aliveH[e])
          hostRpc(GS_TRACE_RECV_RPC, col[e], an.node, h, GS_RPC_ORD(0, GS_RPC_O_ANNOUNCE + an.topic), an.topic, 0,
                  an.sub ? 1 : 0);
    const uint64_t bit = 1ull << an.topic;
    subA[an.node] = an.sub ? (subA[an.node] | bit) : (subA[an.node] & ~bit);
    subAChanged = true;
  }
  pendAnn.clear();
  size_t end = nextEv;
  while (end < events.size() && events[end].hop == h) end++;
  std::vector<int32_t> down, up, leave, join;
  std::map<int, uint64_t> leaveM, joinM;
  auto edgeOf = [&](int a, int b) -> int64_t {
    auto bgn = col.begin() + rowptr[a], fin = col.begin() + rowptr[a + 1];
    auto it = std::lower_bound(bgn, fin, b);
    return (int64_t)(it - col.begin());
  };
  for (int pass = GS_EV_DISCONNECT; pass <= GS_EV_JOIN; ++pass) {
    if (pass == GS_EV_LEAVE && (doPX || !directPairs.empty())) {
      // the connector's dials of the previous hop (peer exchange, direct
      // peers) complete after this hop's scheduled disconnects and connects:
      // each pair once, ascending
      std::sort(pxPend.begin(), pxPend.end());
      pxPend.erase(std::unique(pxPend.begin(), pxPend.end()), pxPend.end());
      for (auto& pr : pxPend) {
        const int64_t ab = edgeOf(pr.first, pr.second), ba = edgeOf(pr.second, pr.first);
        if (aliveH[ab]) continue;
        aliveH[ab] = aliveH[ba] = 1;
        if (world == 1 || (ab >= e0 && ab < e1) || (ba >= e0 && ba < e1)) {
          up.push_back((int32_t)ab);
          up.push_back((int32_t)ba);
        }
        if (acctOn)  // hello packets both ways (pubsub.go:534)
          acctPend.insert(acctPend.end(), {ab, helloBytes(sub[pr.first]), ba, helloBytes(sub[pr.second])});
        if (traceRpc) {
          hostRpc(GS_TRACE_RECV_RPC, pr.first, pr.second, h, GS_RPC_ORD(0, GS_RPC_O_HELLO), -1, sub[pr.second], 1);
          hostRpc(GS_TRACE_RECV_RPC, pr.second, pr.first, h, GS_RPC_ORD(0, GS_RPC_O_HELLO), -1, sub[pr.first], 1);
        }
      }
      pxPend.clear();
    }
    for (size_t k = nextEv; k < end; ++k) {
      const Event& ev = events[k];
      if (ev.kind != pass) continue;
      if (pass <= GS_EV_CONNECT) {
        const int64_t ab = edgeOf(ev.a, ev.b), ba = edgeOf(ev.b, ev.a);
        const uint8_t want = pass == GS_EV_CONNECT ? 1 : 0;
        if (aliveH[ab] == want) continue;
        aliveH[ab] = aliveH[ba] = want;
        auto& lst = pass == GS_EV_CONNECT ? up : down;
        // a partitioned rank launches the pairs with a side it owns (the
        // kernels do only that side)
        if (world == 1 || (ab >= e0 && ab < e1) || (ba >= e0 && ba < e1)) {
          lst.push_back((int32_t)ab);
          lst.push_back((int32_t)ba);
        }
        if (acctOn && want) {  // hello packets both ways (pubsub.go:534)
          acctPend.insert(acctPend.end(), {ab, helloBytes(sub[ev.a]), ba, helloBytes(sub[ev.b])});
        }
        if (traceRpc && want) {  // the hellos' RecvRPC
          hostRpc(GS_TRACE_RECV_RPC, ev.a, ev.b, h, GS_RPC_ORD(0, GS_RPC_O_HELLO), -1, sub[ev.b], 1);
          hostRpc(GS_TRACE_RECV_RPC, ev.b, ev.a, h, GS_RPC_ORD(0, GS_RPC_O_HELLO), -1, sub[ev.a], 1);
        }
        if (traceRpc && !want) {  // RPCs in flight on the connection are lost
          rpcDowns.push_back({h, ev.a, ev.b});
          rpcDowns.push_back({h, ev.b, ev.a});
        }
      } else {
        const uint64_t bit = 1ull << ev.b;
        const bool joinEv = pass == GS_EV_JOIN;
        if (((sub[ev.a] & bit) != 0) == joinEv) continue;
        if (acctOn)  // announce (pubsub.go:775-792) to every connected peer
          for (int64_t e = rowptr[ev.a]; e < rowptr[ev.a + 1]; ++e)
            if (aliveH[e]) acctPend.insert(acctPend.end(), {e, gs_pb_field(gs_pb_subopts(acctTl[ev.b]))});
        if (traceRpc)
          for (int64_t e = rowptr[ev.a]; e < rowptr[ev.a + 1]; ++e)
            if (aliveH[e])
              hostRpc(GS_TRACE_SEND_RPC, ev.a, col[e], h, GS_RPC_ORD(0, GS_RPC_O_ANNOUNCE + ev.b), ev.b, 0,
                      joinEv ? 1 : 0);
        sub[ev.a] = joinEv ? (sub[ev.a] | bit) : (sub[ev.a] & ~bit);
        subChanged = true;
        pendAnn.push_back({ev.a, ev.b, joinEv});
        (joinEv ? joinM : leaveM)[ev.a] |= bit;
      }
    }
  }
  nextEv = end;
  // one item per node: node, topic mask (lo, hi) — its topics run in one wave
  // (a partitioned rank: its own nodes)
  for (auto* pr : {&leaveM, &joinM}) {
    auto& lst = pr == &leaveM ? leave : join;
    for (auto& kv : *pr) {
      if (kv.first < n0 || kv.first >= n1) continue;
      lst.push_back(kv.first);
      lst.push_back((int32_t)(uint32_t)kv.second);
      lst.push_back((int32_t)(uint32_t)(kv.second >> 32));
    }
  }
  if (acctOn) GS_TRY(flushAcct());
  if (subAChanged) GS_TRY(upload(dSubA, subA.data(), (size_t)N * 8));
  if (subChanged) GS_TRY(upload(dSubOwn, sub.data(), (size_t)N * 8));
  if (!down.empty()) {
    GS_TRY(uploadList(down));
    k_edge_down<<<(unsigned)down.size(), 64, 0, stream>>>(d, evBuf.p, h, now, prv);
  }
  if (!up.empty()) {
    GS_TRY(uploadList(up));
    k_edge_up<<<nblk((int64_t)up.size(), 256), 256, 0, stream>>>(d, evBuf.p, (int)up.size(), h);
  }
  const bool recChanged = !down.empty() || !up.empty();
  if (recChanged && p6Live() && n1 > n0) k_p6<<<n1 - n0, 64, 0, stream>>>(d, dP6w);
  if (!leave.empty()) {
    GS_TRY(uploadList(leave));
    k_leave<<<(unsigned)(leave.size() / 3), 64, 0, stream>>>(d, evBuf.p, h, cur);
  }
  if (!join.empty()) {
    GS_TRY(uploadList(join));
    k_join_pairs<<<(unsigned)(join.size() / 3), 64, 0, stream>>>(d, evBuf.p, h, now, cur);
  }
  HIPCHECK(hipGetLastError());
  return GS_OK;
}

// One hop (DESIGN.md §4 "Canonical round"): the stages below in launch order.
int gs_engine::stepOne() {
  Hop hp{hop, hop * cfg.hop_ns, (int)(hop & 1)};
  if (churnOn) {
    GS_TRY(applyEvents(hp.h));
    if (hp.h == directInitHop) directConnect();  // after DirectConnectInitialDelay (gossipsub.go:492-502)
  }
  const bool gossip = cfg.router == GS_ROUTER_GOSSIPSUB;
  GS_TRY(hopWindow(hp));
  if (scoring && narrowDlt && narrowFoldDue(hp.h)) {
    // this hop's counts could take a 16-bit pending word past 255 per field:
    // fold what has accumulated since foldStart first
    if (eOwn) k_fold_all<<<nblk(eOwn * T, 256), 256, 0, stream>>>(d);
    foldStart = hp.h;
  }
  if (scoring) TIMED(this, GS_K_SCORE, (score_rows<1>(d, eOwn, T, nullptr, stream)));
  if (hp.h == 0 && gossip && nOwn()) TIMED(this, GS_K_JOIN, (k_join<<<nOwn(), 64, 0, stream>>>(d, hp.h, hp.now, hp.cur)));
  if (gossip && !floodPublish && hp.n > 0) GS_TRY(fanoutPublish(hp));
  GS_TRY(phaseA(hp));
  if (lat.on) GS_TRY(latencyStats(hp));
  GS_TRY(retireAndPublish(hp));
  // the copies the owned senders send next hop, per edge (phase A reads them)
  if (d.pushOvf) HIPCHECK(hipMemsetAsync(d.pushOvf, 0, 4, stream));
  if (nOwn() && pushOn) TIMED(this, GS_K_PUSH, (k_push<<<nOwn(), 64, 0, stream>>>(d, hp.cur)));
  if (gossip) GS_TRY(phaseB(hp));
  refreshOrFold(hp);
  if (gaterDecayDue(hp.now)) {  // peerGater.background ticker (peer_gater.go:204-217)
    const int64_t nth = std::max<int64_t>(nOwn(), eOwn);
    if (nth) k_gater_decay<<<nblk(nth, 256), 256, 0, stream>>>(d, hp.now);
  }
  if (heartbeatDue(hp.now)) heartbeat(hp);
  // RPC accounting: this hop's forwarded and published messages, one RPC each
  if (acctOn && nOwn()) k_acct_payload<<<nOwn(), 64, 0, stream>>>(d, hp.cur);
  if (traceRpc && nOwn()) k_trace_payload<<<nOwn(), 64, 0, stream>>>(d, hp.cur, hp.h);
  if (doPX) GS_TRY(readPx());
  HIPCHECK(hipGetLastError());
  if (world > 1) GS_TRY(exchange(hp.cur, heartbeatDue(hp.now)));
  hop++;
  for (const Tick& t : tickers)
    if (t.tk->due(hop)) {
      GS_TRY((this->*t.take)());
      t.tk->taken++;
    }
  return GS_OK;
}

// This hop's publishes, the active word windows and phase A's young-slot
// table: per amR word (by rank) the slot mask, then the number of young slots
// in the words before it.  A message is young, and its word active, while
// hop - publish hop <= its topic's age limit: the scan starts at the largest.
int gs_engine::hopWindow(Hop& hp) {
  const int64_t h = hp.h;
  hp.b = hp.e = nextMsg;
  while (hp.e < mHop.size() && mHop[hp.e] == h) hp.e++;
  nextMsg = hp.e;
  hp.n = (int)(hp.e - hp.b);
  yWord.assign((size_t)W, 0);
  yTabH.assign(2 * (size_t)W, 0);
  auto build = [&](int64_t lo, int64_t hi, WMask& m, bool young) {
    auto it = std::lower_bound(mHop.begin(), mHop.end(), lo);
    for (size_t k = (size_t)(it - mHop.begin()); k < mHop.size() && mHop[k] <= hi; ++k) {
      if (hi - mHop[k] > ageOf(mTopic[k])) continue;  // past its topic's own age limit
      const int w = mSlot[k] >> 6;
      m.m[w >> 6] |= 1ull << (w & 63);
      if (young) yWord[w] |= 1ull << (mSlot[k] & 63);
    }
  };
  build(h - 1 - ageMax, h - 1, hp.amR, true);
  build(h - ageMax, h, hp.amW, false);
  int rk = 0;
  for (int w = 0; w < W; ++w) {
    if (!((hp.amR.m[w >> 6] >> (w & 63)) & 1)) continue;
    yTabH[rk] = yWord[w];
    yTabH[(size_t)W + rk] = (uint64_t)hp.nY | ((uint64_t)w << 32);  // (the word, for k_phase_a DENSE)
    hp.nY += __builtin_popcountll(yWord[w]);
    ++rk;
  }
  if (rk) GS_TRY(upload(d.yTab, yTabH.data(), yTabH.size() * 8));
  for (size_t k = hp.b; k < hp.e; ++k) {
    const int w = mSlot[k] >> 6;
    hp.amP.m[w >> 6] |= 1ull << (w & 63);
    if (std::find(hp.retireWords.begin(), hp.retireWords.end(), w) == hp.retireWords.end()) hp.retireWords.push_back(w);
  }
  HIPCHECK(hipMemsetAsync(d.pubmask[hp.cur], 0, (size_t)W * 8, stream));
  HIPCHECK(hipMemsetAsync(d.poolCnt + (size_t)hp.cur * d.poolSub * 16, 0, (size_t)d.poolSub * 16 * 8, stream));
  return GS_OK;
}

// Publish to a topic we have not joined: fanout (gossipsub.go:977-994)
int gs_engine::fanoutPublish(const Hop& hp) {
  std::vector<int32_t> pairs;
  std::vector<uint64_t> seenPair;
  for (size_t i = hp.b; i < hp.e; ++i) {
    const int src = mSrc[i], t = mTopic[i];
    if (src < n0 || src >= n1) continue;  // another rank's publisher
    if (routerOf(src) != GS_ROUTER_GOSSIPSUB) continue;  // floodsub / randomsub hosts keep no fanout
    if ((sub[src] >> t) & 1) continue;
    const uint64_t key = ((uint64_t)src << 6) | (uint64_t)t;
    if (std::find(seenPair.begin(), seenPair.end(), key) != seenPair.end()) continue;
    seenPair.push_back(key);
    pairs.push_back(src);
    pairs.push_back(t);
  }
  if (pairs.empty()) return GS_OK;
  const int np = (int)pairs.size() / 2;
  GS_TRY(pairsBuf.reserve(pairs.size()));
  GS_TRY(upload(pairsBuf.p, pairs.data(), pairs.size() * 4));
  TIMED(this, GS_K_FANOUT, (k_fanout_pub<<<np, 64, 0, stream>>>(d, pairsBuf.p, np, hp.h, hp.now)));
  return GS_OK;
}

// Forwarding masks, this hop's publish and old-slot masks, then phase A: the
// owned nodes take in what their peers sent last hop.
int gs_engine::phaseA(const Hop& hp) {
  const int64_t h = hp.h;
  const int cur = hp.cur, no = nOwn();
  const WMask &amR = hp.amR, &amW = hp.amW, &amP = hp.amP;
  if (eOwn && !denseFlood) TIMED(this, GS_K_FWD, (k_fwd<<<nblk(eOwn, 256), 256, 0, stream>>>(d, cur)));
  if (hp.n > 0) k_pubmask<<<nblk(hp.n, 256), 256, 0, stream>>>(d, (int)hp.b, hp.n, cur);
  k_oldmask<<<nblk(S, 256), 256, 0, stream>>>(d, h);
  const int nR = __builtin_popcountll(amR.m[0]) + __builtin_popcountll(amR.m[1]) +
                 __builtin_popcountll(amR.m[2]) + __builtin_popcountll(amR.m[3]);
  // 8-bit (sender, topic) counters when no topic has more than 255 live
  // message slots: a sender delivers each message at most once per hop
  // (E_DOUBLE), so it cannot deliver more copies of one topic than that
  const bool narrow = !topicOver255(h, h);
  if (narrowDlt && !narrow) {  // St <= 254 bounds a topic's live slots by 255: cannot happen
    gs_set_error("internal: 16-bit pending counts without narrow phase-A counters");
    return GS_EDEVICE;
  }
  const size_t nCnt = ((size_t)T * d.maxDeg + 7) & ~(size_t)7;
  const int nYp = (hp.nY + 15) & ~15;
  // the adversarial model (validators, gater, attackers) has its own
  // instantiation: the honest path keeps its LDS budget and code; DENSE
  // (denseGossip) is honest by definition and denseFlood has a kernel of its
  // own, so the four never combine
  enum { PA_FLOOD, PA_ADV, PA_DENSE, PA_PLAIN };
  const bool adv = advModel();
  const int mode = denseFlood ? PA_FLOOD : adv ? PA_ADV : denseGossip ? PA_DENSE : PA_PLAIN;
  const bool hasUnc = d.needAge || (adv && d.pmaskRow != nullptr);
  size_t lds = (narrow ? 2 : 4) * nCnt + 16 * (size_t)nR + ((2 * ((size_t)W + nR) + 15) & ~(size_t)15) +
               (size_t)nYp + (hasUnc ? 4 * nCnt : 0);
  if (adv) lds += 4 * nCnt + 4 * 64 * 4 + 8 * 64 + 8 * (size_t)nR;
  // the young slots grow with the age limits the caller sets (gs_window.h):
  // refuse here what the device cannot hold instead of failing the launch
  if (!denseFlood && no) {
    if (ldsLimit == 0) {
      int lim = 0;
      hipFuncAttributes fa{};
      HIPCHECK(hipDeviceGetAttribute(&lim, hipDeviceAttributeMaxSharedMemoryPerBlock, cfg.device));
      HIPCHECK(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&k_phase_a<1, false, false, false>)));
      ldsLimit = (size_t)lim;
      ldsStaticA = fa.sharedSizeBytes;  // (the same in every instantiation)
    }
    if (lds + ldsStaticA > ldsLimit) {
      gs_set_error("hop " + std::to_string(h) + ": phase A needs " + std::to_string(lds + ldsStaticA) +
                   " bytes of LDS per workgroup for " + std::to_string(hp.nY) + " young message slots, the device has " +
                   std::to_string(ldsLimit) + ": lower max_age_hops or the publish rate");
      return GS_ECAPACITY;
    }
  }
  if (no) GS_TRY(upload(dDev, &d, sizeof(Dev)));
  // denseGossip: the words v's fb row of this parity is written over (this
  // hop's window, and what the row held two hops ago)
  WMask amF{};
  for (int k = 0; k < GS_MAX_WPL; ++k) amF.m[k] = amR.m[k] | amW.m[k] | amWPar[cur].m[k];
  amWPar[cur] = amW;
  if (!no) return GS_OK;
  // (topic windows of different sizes: the instantiations that look a slot's
  // topic up in d.wTopic; the dense pass 1 has one topic)
  TIMED(this, GS_K_PHASE_A, with_consts([&](auto w, auto m, auto nar, auto tab) {
          constexpr int WV = CV(w) + 1;
          constexpr bool ADV = CV(m) == PA_ADV;
          if constexpr (CV(m) == PA_FLOOD)  // (no counters: one kernel for either width)
            k_flood_a<WV><<<no, 64, 0, stream>>>(d, h, cur, amR, amW, amP);
          else
            k_phase_a<WV, CV(nar), ADV, CV(m) == PA_DENSE, CV(tab) && CV(m) != PA_DENSE>
                <<<no, 64, lds, stream>>>(phaseADev<ADV>(), h, cur, head, amR, amW, amP, amF, nR, nYp);
        }, wpl_of(W), Pick<4>{mode}, Flag{narrow}, Flag{!lay.uniform}));
  return GS_OK;
}

// Latency statistics, between phase A and the hop's publishes: the lists and
// bitmaps hold this hop's first deliveries and no own publish yet.  Nothing
// is in flight while amR is empty.  Then the per-message rows of the slots
// this hop's publishes take over are zeroed.
int gs_engine::latencyStats(const Hop& hp) {
  const int bins = latBins();
  const bool inFlight = (hp.amR.m[0] | hp.amR.m[1] | hp.amR.m[2] | hp.amR.m[3]) != 0;
  if (nOwn() && inFlight) {
    const int perBlock = denseFlood ? GS_LAT_BLOCK / 64 : GS_LAT_BLOCK / GS_LAT_GROUP;  // nodes in one pass
    const unsigned grid = std::min(lat.dev.grid, nblk(nOwn(), perBlock));
    TIMED(this, kLatCount, with_consts([&](auto bitmap) {
            k_lat_count<CV(bitmap)><<<grid, GS_LAT_BLOCK, (size_t)S * 4, stream>>>(d, hp.cur, hp.amR);
          }, Flag{denseFlood}));
    TIMED(this, kLatFold, (k_lat_fold<<<nblk(S, 256), 256, 0, stream>>>(d, hp.h, bins, lat.dev.perMsg, lat.dev.hist)));
  }
  if (hp.n > 0) k_lat_clear<<<hp.n, 64, 0, stream>>>(d, (int)hp.b, bins, lat.dev.perMsg);
  return GS_OK;
}

// The retired words' spam tables, then this hop's publishes.
int gs_engine::retireAndPublish(const Hop& hp) {
  const int cur = hp.cur, n = hp.n, b = (int)hp.b;
  if (!hp.retireWords.empty()) {
    const int nw = (int)hp.retireWords.size();
    GS_TRY(retireBuf.reserve(hp.retireWords.size()));
    GS_TRY(upload(retireBuf.p, hp.retireWords.data(), hp.retireWords.size() * 4));
    if (nOwn() && (d.spamRow != nullptr || d.pmaskRow != nullptr))
      k_retire<<<nblk((int64_t)nOwn() * nw, 256), 256, 0, stream>>>(d, cur, retireBuf.p, nw);
  }
  if (n > 0) {
    TIMED(this, GS_K_PUBLISH, (k_publish<<<nblk(n, 256), 256, 0, stream>>>(d, b, n, hp.h, cur, head)));
    if (!denseFlood) k_publist<<<nblk(n, 256), 256, 0, stream>>>(d, b, n, cur);
    if (d.sel) k_publish_rs<<<n, 64, 0, stream>>>(d, b);
  }
  return GS_OK;
}

// Phase B: control messages and gossip of the owned nodes.
int gs_engine::phaseB(const Hop& hp) {
  const int64_t h = hp.h;
  if (scoring) TIMED(this, GS_K_SCORE, (score_rows<2>(d, eOwn, T, nullptr, stream)));
  // MaxIHaveLength cuts are possible only if the messages (phantom ids
  // included) that can sit in one gossip window outnumber MaxIHaveLength:
  // published within HistoryGossip + 1 heartbeats plus the delivery age bound
  // Bit 0: one topic's ids may exceed it (emitGossip's cut of a sender's
  // item); bit 1: a sender's ids over all topics may (handleIHave's iask
  // cut of its wants).  Both run in either phase-B instantiation.
  int cutMode = 0;
  const int64_t lo = h - (int64_t)(gp.HistoryGossip + 1) * H - ageMax - 2;  // (the largest age: an upper bound)
  const auto a = std::lower_bound(mHop.begin(), mHop.end(), lo);
  const auto b2 = std::upper_bound(mHop.begin(), mHop.end(), h);
  if ((int64_t)(b2 - a) > (int64_t)gp.MaxIHaveLength) {
    cutMode |= 2;
    std::vector<int64_t> perT((size_t)T, 0);
    for (auto it = a; it != b2; ++it) perT[(size_t)mTopic[(size_t)(it - mHop.begin())]]++;
    for (int t = 0; t < T; ++t)
      if (perT[(size_t)t] > (int64_t)gp.MaxIHaveLength) cutMode |= 1;
  }
  const size_t ldsB = cutMode ? GS_CUTLDS : 0;
  if (cutMode & 1) HIPCHECK(hipMemsetAsync(d.cutSpN, 0, 8, stream));
  if (!nOwn()) return GS_OK;
  GS_TRY(upload(dDev, &d, sizeof(Dev)));
  // (a phantom id is an attacker's doing even where no node is marked one)
  TIMED(this, GS_K_PHASE_B, with_consts([&](auto w, auto adv) {
          k_phase_b<CV(w) + 1, CV(adv)><<<nOwn(), 64, ldsB, stream>>>(dDev, h, hp.now, hp.cur, head, cutMode);
        }, wpl_of(W), Flag{advModel() || anyPhantom}));
  return GS_OK;
}

// A score refresh when due; otherwise the periodic fold of the pending
// delivery counts.
void gs_engine::refreshOrFold(const Hop& hp) {
  if (refreshDue(hp.now)) {
    const unsigned rb = nblk(eOwn, GS_RG * (GS_RP / T));  // a wave per GS_RG groups of GS_RP / T edges
    const bool laneT = (64 % T) == 0;  // a lane keeps one topic; narrowDlt: St <= 254 and T even
    TIMED(this, GS_K_REFRESH, with_consts([&](auto ndltC, auto churnC, auto laneC) {
            k_refresh_rows<CV(churnC), CV(laneC), CV(ndltC)><<<rb, 64, 0, stream>>>(d, hp.now);
          }, Flag{narrowDlt}, Flag{churnOn}, Flag{laneT}));
    if (churnOn && p6Live() && nOwn()) k_p6<<<nOwn(), 64, 0, stream>>>(d, dP6w);  // expired records
    refreshedHop = hp.h;
    d.lastRefresh = hp.now;  // the kernels launched from here on derive mesh pairs' meshTime from it
    hopsSinceFold = 0;
    foldStart = hp.h + 1;
  } else if (scoring && !narrowDlt && ++hopsSinceFold >= foldEvery) {
    // pending delivery counts are 16-bit: fold them before they can overflow
    k_fold_all<<<nblk(eOwn * T, 256), 256, 0, stream>>>(d);
    hopsSinceFold = 0;
  }
}

// The heartbeat of the owned nodes, then the peertx rebuild.
void gs_engine::heartbeat(const Hop& hp) {
  const int64_t h = hp.h, now = hp.now;
  const int no = nOwn();
  ticks++;
  if (!directPairs.empty() && ticks % gp.DirectConnectTicks == 0) directConnect();  // gossipsub.go:1318
  // right after a refresh S0 holds exact scores: recompute only what hb_pre
  // dirtied; opportunistic grafting (every OGT ticks) ranks every mesh
  // score, so it gets the full exact pass; otherwise the threshold-exact
  // memo pass (k_score_rows<4>), with the Dhi ranking's mesh members marked
  // by hb_pre so it computes their exact scores too
  const bool exactPass = scoring && (refreshedHop == h || ticks % (uint64_t)d.OGT == 0);
  if (no) TIMED(this, GS_K_HB_PRE, (k_hb_pre<<<no, 64, 0, stream>>>(d, now, ticks, scoring && !exactPass ? 1 : 0)));
  if (scoring && refreshedHop == h)
    TIMED(this, GS_K_SCORE, (score_rows<3>(d, eOwn, T, nullptr, stream)));
  else if (scoring && ticks % (uint64_t)d.OGT == 0)
    TIMED(this, GS_K_SCORE, (score_rows<0>(d, eOwn, T, d.score1, stream)));
  else if (scoring)
    TIMED(this, GS_K_SCORE, (score_rows<4>(d, eOwn, T, nullptr, stream)));
  const int newhead = (head + R - 1) % R;
  // nodes of degree <= 32: two topics per wave (one per half-wave)
  if (no)
    TIMED(this, GS_K_HEARTBEAT, with_consts([&](auto half) {
            k_heartbeat<CV(half)><<<no, 64, 0, stream>>>(d, h, now, ticks, hp.cur, head, newhead);
          }, Flag{d.maxDeg <= 32}));
  // the peertx counters of the window that left the cache (pre-shift HL - 1)
  if (no) ptx_rebuild_launch(d, no, (head + d.HL - 1) % R, stream);
  head = newhead;
  heartbeats++;
}

int gs_engine::checkDeviceError() {
  HIPCHECK(hipStreamSynchronize(stream));
  resolveTimings();
  int32_t err = 0;
  HIPCHECK(hipMemcpy(&err, d.err, 4, hipMemcpyDeviceToHost));
  return deviceErrorText(err, -1);
}

// Waits for the last n hops (first one = firstHop) and reports the first whose
// device error flag is set.
int gs_engine::drainErrors(int64_t firstHop, int n) {
  HIPCHECK(hipStreamSynchronize(stream));
  resolveTimings();
  for (int i = 0; i < n; ++i)
    if (errRing[i]) return deviceErrorText(errRing[i], firstHop + i);
  return GS_OK;
}

int gs_engine::deviceErrorText(int32_t err, int64_t atHop) {
  const int rc = deviceErrorCode(err);
  if (rc != GS_OK && atHop >= 0) {
    g_err = "hop " + std::to_string(atHop) + ": " + g_err;
    stickyRc = rc;
    stickyMsg = g_err;
  }
  return rc;
}

int gs_engine::deviceErrorCode(int32_t err) {
  switch (err) {
    case E_NONE: return GS_OK;
    case E_POOL: gs_set_error("IWANT payload arena overflow (max(2^24 / ranks, 4 x owned edges) ids per rank per hop)"); return GS_ECAPACITY;
    case E_PROMISES:
      gs_set_error("per-node promise table overflow (sized degree x (IWantFollowupTime / HeartbeatInterval + 2) "
                   "entries)");
      return GS_ECAPACITY;
    case E_PEERTX:
      gs_set_error("IWANT retransmission overflow table full (gs_set_peertx_capacity: 2^16 entries per rank "
                   "by default, 2^20 with IWANT spammers)");
      return GS_ECAPACITY;
    case E_LATE:
      gs_set_error(std::string("a message was first delivered later than the message window allows; raise "
                               "slots_per_topic") + (windowsSet ? " or its topic's max_age_hops (gs_set_topic_windows)" : ""));
      return GS_ECAPACITY;
    case E_TRUNCATE:
      gs_set_error("the MaxIHaveLength cut table overflowed (more than 64 over-length IHAVE items at a node "
                   "spill into 2^20 entries per rank per hop), or a sender cut arose outside cut mode");
      return GS_ECAPACITY;
    case E_FCAP:
      gs_set_error("more first deliveries (plus own publishes) at one node in one hop than its "
                   "frontier list holds (min(slots + 64, 2^31 / num_nodes) entries)");
      return GS_ECAPACITY;
    case E_DELTA:
      gs_set_error("pending delivery count of one (edge, topic) overflowed 65535 (255 in the 16-bit layout) "
                   "between two folds");
      return GS_ECAPACITY;
    case E_TRACE:
      gs_set_error("more trace events between two gs_trace_read calls than the capacity given to gs_set_trace");
      return GS_ECAPACITY;
    case E_DOUBLE:
      gs_set_error("a peer sent the same message twice in one hop (outside the canonical model)");
      return GS_EUNSUPPORTED;
    case E_STAMP:
      gs_set_error("debug cycle stamp index outside its buffer (GS_STAMPS build)");
      return GS_EDEVICE;
    default: gs_set_error("unknown device error"); return GS_EDEVICE;
  }
}

// ---- end-of-hop exchange of a partitioned engine (gs_exchange.h; every layout
// comes from gs_exchange_wire.h) ----

// End-of-hop exchange: pack what this rank's nodes sent in hop h, hand it to
// the host transport, unpack what the other ranks' nodes sent to ours.
int gs_engine::exchange(int cur, bool hb) {
  Xchg x{cur, hb, d.ibxRec[0] != nullptr};
  GS_TRY(xCount(x));
  GS_TRY(xPackBroadcast(x));
  // the connector's dials of this hop (peer exchange): every rank applies all
  // of them at the next hop's start (each launching the sides it owns)
  x.sp = gsx::planSend(gsx::Readback{xHost, world}, x.xpush, x.bc, x.nPool, hb, x.lists, (int64_t)pxPend.size());
  GS_TRY(xPackRecords(x));
  GS_TRY(xPackPush(x));
  HIPCHECK(hipStreamSynchronize(stream));  // recOff is pageable; the transport reads the buffers
  const auto t0 = std::chrono::steady_clock::now();
  GS_TRY(xAgreeSizes(x));
  GS_TRY(xGatherChunks(x));
  GS_TRY(xGatherDials(x));
  GS_TRY(xSwapRecords(x));
  GS_TRY(xSwapPush(x));
  xMs += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return xUnpack(x);
}

// The owned nodes' frontier lists into xSend: the node header, then the
// entries that fit (the bump counts on past the capacity).
void gs_engine::xPackLists(const Xchg& x) {
  const size_t hdr = gsx::listHeaderBytes(nOwn());
  const int64_t capEnt = (int64_t)((xSend.cap - hdr) / 4);
  if (nOwn() && x.lists)
    k_x_lists<<<nOwn(), 64, 0, stream>>>(d, x.cur, gsx::XCnt{xCnt, world}.bump(), (int64_t*)xSend.p,
                                         (uint32_t*)(xSend.p + hdr), capEnt);
}

// Counts per destination and the lists (into a buffer that usually suffices;
// packed again by xPackBroadcast if not), read back in one host round trip.
int gs_engine::xCount(Xchg& x) {
  const int cur = x.cur;
  const gsx::XCnt cnt{xCnt, world};
  const gsx::Readback rb{xHost, world};
  HIPCHECK(hipMemsetAsync(xCnt, 0, gsx::XCnt::words(world) * 8, stream));
  if (eOwn) k_x_count<<<nblk(eOwn, 256), 256, 0, stream>>>(d, cur, cnt.counts());
  if (x.xpush) {
    HIPCHECK(hipMemsetAsync(xpCnt, 0, gsx::XpCnt::words(world) * 8, stream));
    if (eOwn) k_xp_count<<<nblk(eOwn, 256), 256, 0, stream>>>(d, cur, gsx::XpCnt{xpCnt, world}.counts());
    HIPCHECK(hipMemcpyAsync(rb.push(), xpCnt, gsx::XpCnt::countWords(world) * 8, hipMemcpyDeviceToHost, stream));
  }
  GS_TRY(xSend.reserve(gsx::listHeaderBytes(nOwn()) + (16u << 20)));
  // A receiver reads this rank's frontier lists only where it walks them:
  // without push (T < 4), for an IWANT spammer's re-requests, or for a sender
  // whose copies overflowed its push region (record -1).  Otherwise every
  // cross-rank edge's copies travel as pushed segments and the lists stay home.
  // With push and no IWANT spammers the lists travel only if some sender's
  // push overflowed: that flag rides in this readback (one host round trip
  // per hop), and the lists are packed after it when needed.
  const bool deferLists = x.xpush && d.cSpam[cur] == nullptr;
  if (deferLists) {
    rb.pushOverflow() = 0;
    HIPCHECK(hipMemcpyAsync(&rb.pushOverflow(), d.pushOvf, 4, hipMemcpyDeviceToHost, stream));
  } else {
    xPackLists(x);
  }
  HIPCHECK(hipMemcpyAsync(rb.records(), cnt.counts(), (size_t)world * 8, hipMemcpyDeviceToHost, stream));
  HIPCHECK(hipMemcpyAsync(&rb.entries(), cnt.bump(), 8, hipMemcpyDeviceToHost, stream));
  HIPCHECK(hipMemcpyAsync(&rb.arenaIds(), d.poolCnt + (size_t)cur * d.poolSub * 16, 8, hipMemcpyDeviceToHost,
                          stream));  // (poolSub == 1 when partitioned)
  // this rank's device error word travels with the sizes (xAgreeSizes), so
  // every rank stops at the same hop (a rank returning alone would leave the
  // others waiting in the next hop's collectives)
  rb.error() = 0;
  HIPCHECK(hipMemcpyAsync(&rb.error(), d.err, 4, hipMemcpyDeviceToHost, stream));
  HIPCHECK(hipStreamSynchronize(stream));
  if (deferLists) {
    x.lists = (int32_t)(rb.pushOverflow() & 0xFFFFFFFFu) != 0;
    if (x.lists) {  // (rare: a sender's copies overflowed its push region)
      xPackLists(x);
      HIPCHECK(hipMemcpyAsync(&rb.entries(), cnt.bump(), 8, hipMemcpyDeviceToHost, stream));
      HIPCHECK(hipStreamSynchronize(stream));
    }
  }
  x.nPool = std::min<int64_t>((int64_t)rb.arenaIds(), poolSeg);
  return GS_OK;
}

// This rank's broadcast chunk around the lists already in xSend.  A chunk
// that outgrew the buffer grows it (which keeps nothing) and packs the lists
// again.
int gs_engine::xPackBroadcast(Xchg& x) {
  // randomsub hosts' target masks ride with their list entries (a receiver
  // walking a remote randomsub sender's list filters by them)
  const gsx::Bcast& b = x.bc = gsx::bcastLayout(nOwn(), (int64_t)gsx::Readback{xHost, world}.entries(), x.nPool, W,
                                                x.lists, d.sel != nullptr, x.hb);
  if (b.total > xSend.cap) {
    GS_TRY(xSend.reserve(b.total));
    HIPCHECK(hipMemsetAsync(gsx::XCnt{xCnt, world}.bump(), 0, 8, stream));
    xPackLists(x);
  }
  if (b.masks() && nOwn())
    k_x_sel<<<nOwn(), 64, 0, stream>>>(d, (const int64_t*)xSend.p, (const uint32_t*)(xSend.p + b.ent),
                                       (uint64_t*)(xSend.p + b.sel));
  if (x.nPool)
    HIPCHECK(hipMemcpyAsync(xSend.p + b.arena, d.pool[x.cur] + (int64_t)rank * poolSeg, (size_t)x.nPool * 4,
                            hipMemcpyDeviceToDevice, stream));
  if (b.gwBytes())
    HIPCHECK(hipMemcpyAsync(xSend.p + b.gw, d.gw + (size_t)n0 * W, b.gwBytes(), hipMemcpyDeviceToDevice, stream));
  return GS_OK;
}

// Edge records, one block per destination rank.
int gs_engine::xPackRecords(Xchg& x) {
  GS_TRY(xSendE.reserve((size_t)std::max<int64_t>(x.sp.totRec, 1) * sizeof(XRec)));
  if (x.sp.totRec) {
    HIPCHECK(hipMemcpyAsync(xOff, x.sp.recOff.data(), (size_t)world * 8, hipMemcpyHostToDevice, stream));
    k_x_pack<<<nblk(eOwn, 256), 256, 0, stream>>>(d, x.cur, xOff, gsx::XCnt{xCnt, world}.cursors(), (XRec*)xSendE.p);
  }
  return GS_OK;
}

// Pushed segments of cross-rank edges, one block per destination rank.
int gs_engine::xPackPush(Xchg& x) {
  if (!x.xpush) return GS_OK;
  GS_TRY(xSendP.reserve((size_t)std::max<int64_t>(x.sp.pushTotal, 16)));
  if (!x.sp.pushTotal) return GS_OK;
  std::vector<int64_t> offRec(gsx::XpOff::words(world));
  const gsx::XpOff host{offRec.data(), world}, dev{xpOff, world};
  std::copy(x.sp.pushOff.begin(), x.sp.pushOff.end(), host.blockOff());
  std::copy(x.sp.pushRec.begin(), x.sp.pushRec.end(), host.records());
  HIPCHECK(hipMemcpyAsync(xpOff, offRec.data(), offRec.size() * 8, hipMemcpyHostToDevice, stream));
  unsigned long long* cursors = gsx::XpCnt{xpCnt, world}.cursors();
  HIPCHECK(hipMemsetAsync(cursors, 0, gsx::XpCnt::countWords(world) * 8, stream));
  k_xp_pack<<<nblk(eOwn, 256), 256, 0, stream>>>(d, x.cur, dev.blockOff(), dev.records(), cursors, xSendP.p);
  return GS_OK;
}

// Every rank's size row; any rank's device error stops every rank here.
int gs_engine::xAgreeSizes(Xchg& x) {
  const int nS = gsx::SizeRow::count(world);
  x.all.resize((size_t)nS * world);
  if (tr.allgather_i64(tr.user, x.sp.row.data(), nS, x.all.data()) != 0) {
    gs_set_error("transport allgather_i64 failed");
    return GS_EDEVICE;
  }
  const int32_t myErr = (int32_t)gsx::SizeRow{x.sp.row.data(), world}.error();
  if (myErr) return deviceErrorText(myErr, hop);
  for (int r = 0; r < world; ++r) {
    const int32_t err = (int32_t)gsx::SizeRow::of(x.all, world, r).error();
    if (!err) continue;
    const int rc = deviceErrorCode(err);  // the failing rank's code and text
    g_err = "hop " + std::to_string(hop) + ": rank " + std::to_string(r) + ": " + g_err;
    stickyRc = rc;
    stickyMsg = g_err;
    return rc;
  }
  x.rp = gsx::planRecv(x.all, world, rank, x.xpush);
  return GS_OK;
}

// All-gather of the broadcast chunks.
int gs_engine::xGatherChunks(Xchg& x) {
  GS_TRY(xSend.reserve((size_t)x.rp.chunk, x.bc.total));  // the transport reads `chunk` bytes
  GS_TRY(xRecv.reserve((size_t)x.rp.chunk * world));
  if (tr.allgather(tr.user, xSend.p, xRecv.p, x.rp.chunk) != 0) {
    gs_set_error("transport allgather failed");
    return GS_EDEVICE;
  }
  return GS_OK;
}

// Every rank's dials of this hop replace this rank's own in pxPend.
int gs_engine::xGatherDials(Xchg& x) {
  const int64_t maxD = x.rp.maxDials;
  if (maxD <= 0) return GS_OK;
  const std::vector<int64_t> dm = gsx::packDials(pxPend, maxD);
  std::vector<int64_t> da((size_t)maxD * world);
  if (tr.allgather_i64(tr.user, dm.data(), (int32_t)maxD, da.data()) != 0) {
    gs_set_error("transport allgather_i64 failed (dials)");
    return GS_EDEVICE;
  }
  pxPend = gsx::unpackDials(da);
  return GS_OK;
}

// All-to-all-v of the edge records.
int gs_engine::xSwapRecords(Xchg& x) {
  GS_TRY(xRecvE.reserve((size_t)std::max<int64_t>(x.rp.recTotal, 1)));
  if (tr.alltoallv(tr.user, xSendE.p, x.sp.recBytes.data(), xRecvE.p, x.rp.recBytes.data()) != 0) {
    gs_set_error("transport alltoallv failed");
    return GS_EDEVICE;
  }
  return GS_OK;
}

// All-to-all-v of the push blocks: they land behind the owned senders' regions
// of ibx[cur].
int gs_engine::xSwapPush(Xchg& x) {
  if (!x.xpush) return GS_OK;
  const int cur = x.cur;
  const size_t own = (size_t)ibxOwnSlots * 2;
  // grow this parity's arena where needed, keeping the owned regions (this
  // hop's segments for local receivers)
  GS_TRY(ibx[cur].reserve(own + (size_t)x.rp.pushTotal, own));
  d.ibx[cur] = reinterpret_cast<uint16_t*>(ibx[cur].p);
  if (tr.alltoallv(tr.user, xSendP.p, x.sp.pushBytes.data(), ibx[cur].p + own, x.rp.pushBytes.data()) != 0) {
    gs_set_error("transport alltoallv failed (pushed segments)");
    return GS_EDEVICE;
  }
  xBytes += x.rp.pushTotal;
  return GS_OK;
}

// The other ranks' parts into the mirrors.
int gs_engine::xUnpack(Xchg& x) {
  const int cur = x.cur;
  const gsx::RecvPlan& rp = x.rp;
  for (int r = 0; r < world; ++r) {
    if (r == rank) continue;
    const int nr = part[r + 1] - part[r];
    const gsx::SizeRow a = gsx::SizeRow::of(x.all, world, r);
    const gsx::Bcast b = gsx::bcastLayout(a, nr, W, d.sel != nullptr);
    const uint8_t* c = xRecv.p + (size_t)r * rp.chunk;
    xBytes += a.bcastBytes();
    if (nr && a.lists())
      k_x_unlists<<<nr, 64, 0, stream>>>(d, cur, (const int64_t*)c, (const uint32_t*)(c + b.ent),
                                         b.masks() ? (const uint64_t*)(c + b.sel) : nullptr, part[r]);
    if (a.arenaIds())
      HIPCHECK(hipMemcpyAsync(d.pool[cur] + (size_t)r * poolSeg, c + b.arena, (size_t)a.arenaIds() * 4,
                              hipMemcpyDeviceToDevice, stream));
    if (a.heartbeat() && nr)
      HIPCHECK(hipMemcpyAsync(d.gw + (size_t)part[r] * W, c + b.gw, b.gwBytes(), hipMemcpyDeviceToDevice, stream));
  }
  xBytes += rp.recTotal;
  if (rp.recTotal) {
    const int64_t n = rp.recTotal / (int64_t)sizeof(XRec);
    k_x_unpack<<<nblk(n, 256), 256, 0, stream>>>(d, cur, (const XRec*)xRecvE.p, n);
  }
  for (int r = 0; r < world; ++r) {
    if (!rp.pushRec[r]) continue;
    const uint8_t* blk = reinterpret_cast<const uint8_t*>(d.ibx[cur]) + (size_t)ibxOwnSlots * 2 + rp.pushOff[r];
    k_xp_unpack<<<nblk(rp.pushRec[r], 256), 256, 0, stream>>>(
        d, cur, (const PRec*)blk, rp.pushRec[r], gsx::pushSlotBase(ibxOwnSlots, rp.pushOff[r], rp.pushRec[r]));
  }
  HIPCHECK(hipGetLastError());
  return GS_OK;
}

// Moves the device's trace records to tracePending in canonical order.  The
// kernels record every delivered copy (GS_TRACE_COPY); the copy from the
// first deliverer of a fresh message is its DeliverMessage, every other copy
// a DuplicateMessage (pubsub.go:1010-1013).
int gs_engine::drainTrace() {
  if (!started || !d.traceN) return GS_OK;
  unsigned long long cnt = 0;
  HIPCHECK(hipStreamSynchronize(stream));
  HIPCHECK(hipMemcpy(&cnt, d.traceN, 8, hipMemcpyDeviceToHost));
  const int64_t k = std::min<int64_t>((int64_t)cnt, traceCap);
  std::vector<gs_trace_event> ev((size_t)k);
  if (k) HIPCHECK(hipMemcpy(ev.data(), d.trace, (size_t)k * sizeof(gs_trace_event), hipMemcpyDeviceToHost));
  // on the engine's stream: the next hop's appends are queued there too, and a
  // null-stream memset is not ordered against a non-blocking stream
  HIPCHECK(hipMemsetAsync(d.traceN, 0, 8, stream));
  struct Key {
    int64_t hop, msg;
    int32_t node, peer;
    bool operator<(const Key& o) const {
      return std::tie(hop, msg, node, peer) < std::tie(o.hop, o.msg, o.node, o.peer);
    }
  };
  // a copy is the delivering one (DeliverMessage), a rejected first copy or a
  // copy dropped by a full validation queue (RejectMessage), or else a duplicate
  std::vector<Key> delivered;
  for (const auto& e : ev)
    if ((e.type == GS_TRACE_DELIVER_MESSAGE || e.type == GS_TRACE_REJECT_MESSAGE) && e.phase == 2)
      delivered.push_back(Key{e.hop, e.msg, e.node, e.peer});
  std::sort(delivered.begin(), delivered.end());
  std::vector<gs_trace_event> keep(tracePending.begin() + traceOut, tracePending.end());
  std::vector<gs_trace_event> all;
  all.swap(traceFuture);
  for (auto e : ev) {
    if (e.type == GS_TRACE_COPY) {
      if (std::binary_search(delivered.begin(), delivered.end(), Key{e.hop, e.msg, e.node, e.peer})) continue;
      e.type = GS_TRACE_DUPLICATE_MESSAGE;
    }
    all.push_back(e);
  }
  // RPC blocks: a RECV stamped with a hop that has not run yet waits for it;
  // one whose connection closed at the start of its hop was lost in flight
  for (size_t i = 0; i < all.size();) {
    size_t j = i + 1;
    if (gs_trace_is_rpc(all[i]))
      while (j < all.size() && all[j].type == GS_TRACE_RPC_ITEM) ++j;
    const gs_trace_event& hd = all[i];
    bool drop = false;
    if (hd.hop >= hop) {
      traceFuture.insert(traceFuture.end(), all.begin() + i, all.begin() + j);
      drop = true;
    } else if (hd.type == GS_TRACE_RECV_RPC) {
      const std::array<int64_t, 3> k{hd.hop, hd.node, hd.peer};
      drop = std::find(rpcDowns.begin(), rpcDowns.end(), k) != rpcDowns.end();
    }
    if (!drop) keep.insert(keep.end(), all.begin() + i, all.begin() + j);
    i = j;
  }
  gs_trace_canonical(keep, cfg.seed, gp.MaxIHaveLength);
  tracePending.swap(keep);
  traceOut = 0;
  return GS_OK;
}

// Per-(edge, topic) arrays are edge-major rows [e*T + t] on the device (tix
// in gs_device.h); readbacks return them topic-major [t*E + e].
template <class X>
static int copy_back_pairs(gs_engine* g, X* dst, const X* src) {
  const size_t E = (size_t)g->E, T = (size_t)g->T;
  if (!g->started) {
    std::memset(dst, 0, T * E * sizeof(X));
    return GS_OK;
  }
  // only the owned edges [e0, e1) have per-(edge, topic) state on this rank
  const size_t e0 = (size_t)g->e0, e1 = (size_t)g->e1;
  std::vector<X> tmp(T * (e1 - e0));
  HIPCHECK(hipStreamSynchronize(g->stream));
  HIPCHECK(hipMemcpy(tmp.data(), src + e0 * T, tmp.size() * sizeof(X), hipMemcpyDeviceToHost));
  std::memset(dst, 0, T * E * sizeof(X));
  for (size_t e = e0; e < e1; ++e)
    for (size_t t = 0; t < T; ++t) dst[t * E + e] = tmp[(e - e0) * T + t];
  return GS_OK;
}
extern "C" {

const char* gs_last_error(void) { return g_err.c_str(); }

int gs_engine_create(const gs_config* cfg, const gs_gossipsub_params* gsp, const gs_peer_score_params* psp,
                     const gs_topic_score_params* topics, const uint8_t* topic_scored,
                     const gs_peer_score_thresholds* thr, const gs_peer_gater_params* gater, gs_engine** out) {
  if (!cfg || !out) { gs_set_error("null argument"); return GS_EINVAL; }
  if (cfg->num_nodes <= 0 || cfg->num_topics <= 0 || cfg->num_topics > 64 || cfg->hop_ns <= 0) {
    gs_set_error("invalid config: num_nodes > 0, 1 <= num_topics <= 64, hop_ns > 0 required");
    return GS_EINVAL;
  }
  if (cfg->router < 0 || cfg->router > 2) { gs_set_error("unknown router"); return GS_EINVAL; }
  if (cfg->slots_per_topic <= 0 || cfg->slots_per_topic % 64 != 0) {
    gs_set_error("slots_per_topic must be a positive multiple of 64");
    return GS_EINVAL;
  }
  if (gater) {
    if (cfg->router != GS_ROUTER_GOSSIPSUB) { gs_set_error("pubsub router is not gossipsub"); return GS_EINVAL; }
    GS_TRY(gs_validate_peer_gater_params(gater));
    if (gater->DecayInterval % cfg->hop_ns != 0) {
      gs_set_error("gater DecayInterval must be a multiple of hop_ns");
      return GS_EUNSUPPORTED;
    }
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    gs_set_error("no HIP device available: the gossip engine needs an MI355X (gfx950)");
    return GS_EDEVICE;
  }
  if (cfg->device < 0 || cfg->device >= ndev) { gs_set_error("bad device ordinal"); return GS_EINVAL; }
  std::unique_ptr<gs_engine> g(new gs_engine());
  g->cfg = *cfg;
  if (gater) {
    g->gaterOn = true;
    g->gaterP = *gater;
  }
  g->N = cfg->num_nodes;
  g->T = cfg->num_topics;
  if ((int64_t)g->T * cfg->slots_per_topic > gsw::kMaxSlots) {
    gs_set_error("num_topics * slots_per_topic must be <= 16384 in this build");
    return GS_EUNSUPPORTED;
  }
  g->setLayout(gsw::uniformLayout(g->T, cfg->slots_per_topic));
  g->userAge.assign(g->T, 0);
  if (gsp) g->gp = *gsp; else gs_default_gossipsub_params(&g->gp);
  g->scoring = (cfg->flags & GS_FLAG_SCORING) != 0 && cfg->router == GS_ROUTER_GOSSIPSUB;
  g->floodPublish = (cfg->flags & GS_FLAG_FLOOD_PUBLISH) != 0;
  g->doPX = (cfg->flags & GS_FLAG_PEER_EXCHANGE) != 0 && cfg->router == GS_ROUTER_GOSSIPSUB;
  g->record = (cfg->flags & GS_FLAG_RECORD_DELIVERIES) != 0;
  g->tps.assign(g->T, gs_topic_score_params{});
  g->tscored.assign(g->T, 0);
  if (cfg->router == GS_ROUTER_GOSSIPSUB) {
    const gs_gossipsub_params& p = g->gp;
    if (p.HistoryGossip > p.HistoryLength || p.HistoryLength < 1) {
      gs_set_error("invalid parameters for message cache; gossip slots cannot be larger than history slots");
      return GS_EINVAL;
    }
    if (p.HeartbeatInterval % cfg->hop_ns != 0 || p.HeartbeatInterval < 2 * cfg->hop_ns ||
        p.HeartbeatInitialDelay % cfg->hop_ns != 0 || p.HeartbeatInitialDelay < cfg->hop_ns) {
      gs_set_error("HeartbeatInterval must be a multiple of hop_ns and >= 2 hops; "
                   "HeartbeatInitialDelay a multiple of hop_ns and >= 1 hop");
      return GS_EUNSUPPORTED;
    }
    if (p.DirectConnectTicks == 0) {  // heartbeatTicks % DirectConnectTicks (gossipsub.go:1597)
      gs_set_error("DirectConnectTicks must be > 0");
      return GS_EINVAL;
    }
    if (p.GossipRetransmission < 0 || p.MaxIHaveMessages < 0 || p.D < 0 || p.Dhi < 0 || p.Dscore < 0 ||
        p.Dscore > p.D || p.D > p.Dhi) {
      gs_set_error("invalid gossipsub degree parameters");
      return GS_EINVAL;
    }
    g->H = (int)(p.HeartbeatInterval / cfg->hop_ns);
    g->R = p.HistoryLength + 1;  // + the ghost slot holding the just-shifted window
  } else {
    g->R = 1;
  }
  g->setWindow();
  if (g->maxAge > 30000) { gs_set_error("heartbeat interval too long in hops"); return GS_EUNSUPPORTED; }
  if (g->scoring) {
    if (!psp || !topics || !topic_scored || !thr) {
      gs_set_error("scoring needs score params and thresholds");
      return GS_EINVAL;
    }
    GS_TRY(gs_validate_peer_score_params(psp, topics, topic_scored, g->T));
    GS_TRY(gs_validate_thresholds(thr));
    if (psp->DecayInterval % cfg->hop_ns != 0) {
      gs_set_error("DecayInterval must be a multiple of hop_ns");
      return GS_EUNSUPPORTED;
    }
    g->sp = *psp;
    g->thr = *thr;
    for (int t = 0; t < g->T; ++t) { g->tps[t] = topics[t]; g->tscored[t] = topic_scored[t]; }
  }
  g->topicCounter.assign(g->T, 0);
  g->topicLive.assign(g->T, 0);
  g->slotOwnerHop.assign(g->S, INT64_MIN);
  g->slotOwnerId.assign(g->S, -1);
  *out = g.release();
  return GS_OK;
}

int gs_engine_destroy(gs_engine* eng) {
  delete eng;
  return GS_OK;
}

int gs_set_graph(gs_engine* g, const int64_t* rowptr, const int32_t* col, const uint8_t* outbound,
                 const uint8_t* direct) {
  return gs_set_graph_ex(g, rowptr, col, outbound, direct, nullptr);
}

int gs_set_routers(gs_engine* g, const uint8_t* router) {
  if (g->started) { gs_set_error("routers must be set before the first step"); return GS_ESTATE; }
  g->routerH.clear();
  if (router) {
    for (int u = 0; u < g->N; ++u)
      if (router[u] > GS_ROUTER_GOSSIPSUB_V10) { gs_set_error("unknown router"); return GS_EINVAL; }
    g->routerH.assign(router, router + g->N);
  }
  return GS_OK;
}

int gs_set_graph_ex(gs_engine* g, const int64_t* rowptr, const int32_t* col, const uint8_t* outbound,
                    const uint8_t* direct, const uint8_t* proto) {
  if (g->started) { gs_set_error("graph must be set before the first step"); return GS_ESTATE; }
  g->rowptr.assign(rowptr, rowptr + g->N + 1);
  g->E = g->rowptr[g->N];
  g->col.assign(col, col + g->E);
  for (int u = 0; u < g->N; ++u)
    for (int64_t e = g->rowptr[u]; e < g->rowptr[u + 1]; ++e) {
      const int v = g->col[e];
      if (v < 0 || v >= g->N || v == u || (e > g->rowptr[u] && g->col[e - 1] >= v)) {
        gs_set_error("graph rows must hold strictly ascending neighbour ids != self");
        return GS_EINVAL;
      }
    }
  g->outbound.assign(g->E, 0);
  g->direct.assign(g->E, 0);
  if (outbound) g->outbound.assign(outbound, outbound + g->E);
  if (direct) g->direct.assign(direct, direct + g->E);
  g->protoH.clear();
  g->protoGiven = false;
  if (proto) {
    for (int64_t e = 0; e < g->E; ++e)
      if (proto[e] > GS_PROTO_GOSSIPSUB_V11) { gs_set_error("unknown protocol"); return GS_EINVAL; }
    g->protoH.assign(proto, proto + g->E);
    g->protoGiven = true;
  }
  g->graphSet = true;
  return GS_OK;
}

int gs_set_subscriptions(gs_engine* g, const uint64_t* sub_mask) {
  if (g->started) { gs_set_error("subscriptions must be set before the first step"); return GS_ESTATE; }
  g->sub.assign(sub_mask, sub_mask + g->N);
  return GS_OK;
}

int gs_set_peer_attrs(gs_engine* g, const double* app_score, const uint32_t* ipv4) {
  if (g->started) { gs_set_error("peer attributes must be set before the first step"); return GS_ESTATE; }
  if (app_score) g->app.assign(app_score, app_score + g->N);
  if (ipv4) g->ipv4.assign(ipv4, ipv4 + g->N);
  return GS_OK;
}

int gs_set_ip_whitelist(gs_engine* g, int32_t n, const uint32_t* net, const uint32_t* mask) {
  if (g->started) { gs_set_error("whitelist must be set before the first step"); return GS_ESTATE; }
  g->whitelist.clear();
  for (int i = 0; i < n; ++i) g->whitelist.push_back({net[i], mask[i]});
  return GS_OK;
}

int gs_publish(gs_engine* g, int32_t n, const int32_t* src, const int32_t* topic, const int64_t* hop,
               int64_t* ids_out) {
  return gs_publish_ex(g, n, src, topic, hop, nullptr, ids_out);
}

int gs_publish_ex(gs_engine* g, int32_t n, const int32_t* src, const int32_t* topic, const int64_t* hop,
                  const uint8_t* kind, int64_t* ids_out) {
  int64_t last = g->mHop.empty() ? g->hop : std::max(g->hop, g->mHop.back());
  for (int i = 0; i < n; ++i) {
    if (src[i] < 0 || src[i] >= g->N || topic[i] < 0 || topic[i] >= g->T || hop[i] < last ||
        (kind && kind[i] > GS_MSG_PHANTOM)) {
      gs_set_error("publish: bad src/topic/kind or hop not non-decreasing from the current hop");
      return GS_EINVAL;
    }
    last = hop[i];
  }
  // assign message-window slots; a slot is recycled only after its topic's retire horizon
  std::vector<int64_t> cnt = g->topicCounter, owner = g->slotOwnerHop;
  std::vector<int32_t> slots(n);
  for (int i = 0; i < n; ++i) {
    const int t = topic[i];
    const int slot = g->lay.slotOf(t, cnt[t]);
    cnt[t]++;
    if (!gsw::slotFree(owner[slot], hop[i], g->retireOf(t))) {
      gs_set_error(gsw::guardText(t, g->lay.slots[t], g->retireOf(t), g->windowsSet));
      return GS_ECAPACITY;
    }
    owner[slot] = hop[i];
    slots[i] = slot;
    if (kind && kind[i] == GS_MSG_PHANTOM) g->anyPhantom = true;
  }
  g->topicCounter = cnt;
  g->slotOwnerHop = owner;
  for (int i = 0; i < n; ++i) {
    const int64_t id = (int64_t)g->mSrc.size();
    g->mSrc.push_back(src[i]);
    g->mTopic.push_back(topic[i]);
    g->mSlot.push_back(slots[i]);
    g->mId.push_back(id);
    g->mHop.push_back(hop[i]);
    g->mKind.push_back(kind ? kind[i] : (uint8_t)GS_MSG_VALID);
    g->slotOwnerId[slots[i]] = id;
    if (ids_out) ids_out[i] = id;
  }
  return g->uploadMessages();
}

// ---- topic windows (include/gs_window.h)
int gs_set_topic_windows(gs_engine* g, const int32_t* slots, const int32_t* max_age_hops) {
  if (g->started || !g->mId.empty()) {
    gs_set_error("topic windows must be set before the first publish and the first step");
    return GS_ESTATE;
  }
  std::vector<int32_t> s((size_t)g->T, g->cfg.slots_per_topic), a((size_t)g->T, 0);
  if (slots) s.assign(slots, slots + g->T);
  if (max_age_hops) a.assign(max_age_hops, max_age_hops + g->T);
  std::string why = gsw::checkSlots(s.data(), g->T);
  if (!why.empty()) {
    gs_set_error(why);
    return why.find("16384") != std::string::npos ? GS_EUNSUPPORTED : GS_EINVAL;
  }
  why = gsw::checkAges(a.data(), g->T);
  if (!why.empty()) { gs_set_error(why); return GS_EINVAL; }
  g->setLayout(gsw::makeLayout(s.data(), g->T));
  g->userAge = a;
  g->windowsSet = true;
  g->setWindow();
  g->slotOwnerHop.assign(g->S, INT64_MIN);
  g->slotOwnerId.assign(g->S, -1);
  return GS_OK;
}

int gs_read_topic_windows(const gs_engine* g, int32_t* slots, int32_t* max_age_hops, int32_t* retire_hops) {
  for (int t = 0; t < g->T; ++t) {
    if (slots) slots[t] = g->lay.slots[t];
    if (max_age_hops) max_age_hops[t] = g->ageOf(t);
    if (retire_hops) retire_hops[t] = (int32_t)g->retireOf(t);
  }
  return GS_OK;
}

int gs_set_validation(gs_engine* g, const uint8_t* topic_validator, int32_t queue_per_hop) {
  if (g->started || !g->mId.empty()) {
    gs_set_error("validation must be set before the first publish");
    return GS_ESTATE;
  }
  if (queue_per_hop < 0) { gs_set_error("queue_per_hop must be >= 0"); return GS_EINVAL; }
  g->topicVal = 0;
  if (topic_validator)
    for (int t = 0; t < g->T; ++t)
      if (topic_validator[t]) g->topicVal |= 1ull << t;
  g->valQueue = queue_per_hop;
  g->setWindow();
  return GS_OK;
}

int gs_schedule_events(gs_engine* g, int32_t n, const int32_t* kind, const int32_t* a, const int32_t* b,
                       const int64_t* hop) {
  if (n < 0 || (n > 0 && (!kind || !a || !b || !hop))) { gs_set_error("gs_schedule_events: bad arguments"); return GS_EINVAL; }
  if (!g->graphSet) { gs_set_error("graph not set"); return GS_ESTATE; }
  if (n > 0 && !g->churnWindow && !g->mId.empty()) {
    // late joiners catch up through gossip: the wide message window is chosen
    // when the first churn is scheduled, and it cannot change once messages
    // hold slots (gs_set_behaviour / gs_set_validation have the same rule)
    gs_set_error("connection churn must first be scheduled before the first publish");
    return GS_ESTATE;
  }
  int64_t last = g->events.empty() ? std::max<int64_t>(1, g->hop) : std::max(g->hop, g->events.back().hop);
  auto isEdge = [&](int x, int y) {
    auto bgn = g->col.begin() + g->rowptr[x], fin = g->col.begin() + g->rowptr[x + 1];
    auto it = std::lower_bound(bgn, fin, y);
    return it != fin && *it == y;
  };
  for (int32_t i = 0; i < n; ++i) {
    bool ok = hop[i] >= last && hop[i] >= 1 && kind[i] >= GS_EV_DISCONNECT && kind[i] <= GS_EV_JOIN &&
              a[i] >= 0 && a[i] < g->N;
    if (ok && kind[i] <= GS_EV_CONNECT) ok = b[i] >= 0 && b[i] < g->N && isEdge(a[i], b[i]);
    if (ok && kind[i] >= GS_EV_LEAVE) ok = b[i] >= 0 && b[i] < g->T;
    if (!ok) { gs_set_error("gs_schedule_events: bad event (kind, nodes, topic or hop order)"); return GS_EINVAL; }
    last = hop[i];
  }
  for (int32_t i = 0; i < n; ++i) g->events.push_back({hop[i], kind[i], a[i], b[i]});
  if (n > 0 && !g->started && g->mId.empty()) {
    g->churnWindow = true;  // late joiners catch up through gossip: the wide message window
    g->setWindow();
  }
  if (g->started && n > 0) return g->enableChurn();
  return GS_OK;
}

int gs_set_behaviour(gs_engine* g, const uint8_t* behaviour) {
  if (g->started || !g->mId.empty()) {
    gs_set_error("behaviours must be set before the first publish");
    return GS_ESTATE;
  }
  g->behaveH.clear();
  g->behaveAll = 0;
  if (behaviour) {
    g->behaveH.assign(behaviour, behaviour + g->N);
    for (uint8_t b : g->behaveH) g->behaveAll |= b;
    if (g->behaveAll & ~(uint8_t)(GS_BEHAVE_NO_FORWARD | GS_BEHAVE_IWANT_SPAM | GS_BEHAVE_GRAFT_SPAM |
                                  GS_BEHAVE_IHAVE_SPAM)) {
      gs_set_error("unknown behaviour bit");
      return GS_EINVAL;
    }
  }
  g->setWindow();
  return GS_OK;
}

int gs_step(gs_engine* g, int64_t hops) {
  if (!g->graphSet) { gs_set_error("graph not set"); return GS_ESTATE; }
  if (!g->started) {
    GS_TRY(g->start());
  }
  if (g->stickyRc) {
    gs_set_error(g->stickyMsg);
    return g->stickyRc;
  }
  if (!g->errRing)
    HIPCHECK(hipHostMalloc((void**)&g->errRing, gs_engine::kErrRing * sizeof(int32_t), hipHostMallocDefault));
  int64_t first = g->hop;
  int n = 0;
  for (int64_t i = 0; i < hops; ++i) {
    GS_TRY(g->stepOne());
    HIPCHECK(hipMemcpyAsync(g->errRing + n, g->d.err, 4, hipMemcpyDeviceToHost, g->stream));
    if (++n == gs_engine::kErrRing || g->pendKid.size() > 4096) {
      GS_TRY(g->drainErrors(first, n));
      first = g->hop;
      n = 0;
    }
  }
  return g->drainErrors(first, n);
}

int gs_sync(gs_engine* g) {
  if (!g->started) return GS_OK;
  HIPCHECK(hipStreamSynchronize(g->stream));
  return GS_OK;
}

int gs_set_topic_score_params(gs_engine* g, int32_t topic, const gs_topic_score_params* p) {
  if (topic < 0 || topic >= g->T) { gs_set_error("bad topic"); return GS_EINVAL; }
  GS_TRY(gs_validate_topic_score_params(p));
  if (g->started && g->scoring && !g->d.needAge &&
      p->MeshMessageDeliveriesWindow < g->retireOf(topic) * g->cfg.hop_ns) {
    gs_set_error("MeshMessageDeliveriesWindow shorter than the message lifetime can only be set "
                 "before the first step (per-message first-delivery hops are not kept)");
    return GS_EUNSUPPORTED;
  }
  const bool existed = g->tscored[topic] != 0;
  const gs_topic_score_params old = g->tps[topic];
  g->tps[topic] = *p;
  g->tscored[topic] = 1;
  if (!g->started) return GS_OK;
  TopicP tp = to_dev(*p, g->scoring);
  if (g->scoring) k_fold<<<nblk(g->E, 256), 256, 0, g->stream>>>(g->d, topic);  // with the old caps
  HIPCHECK(hipMemcpyAsync(g->dTp + topic, &tp, sizeof(TopicP), hipMemcpyHostToDevice, g->stream));
  HIPCHECK(hipMemsetAsync(g->d.sdirty + g->e0, 1, (size_t)g->eOwn, g->stream));  // every score may have changed
  if (existed && g->scoring &&
      (p->FirstMessageDeliveriesCap < old.FirstMessageDeliveriesCap ||
       p->MeshMessageDeliveriesCap < old.MeshMessageDeliveriesCap))
    k_recap<<<nblk(g->E, 256), 256, 0, g->stream>>>(g->d, topic, p->FirstMessageDeliveriesCap,
                                                    p->MeshMessageDeliveriesCap);
  HIPCHECK(hipStreamSynchronize(g->stream));
  return GS_OK;
}

int gs_set_partition(gs_engine* g, int32_t rank, int32_t world, const gs_transport* tr) {
  if (g->started) { gs_set_error("the partition must be set before the first step"); return GS_ESTATE; }
  if (world < 1 || world > 255 || rank < 0 || rank >= world) { gs_set_error("bad rank / world"); return GS_EINVAL; }
  // (bandwidth before mesh reach: the order these refusals have always been tried in)
  for (const Ticker* tk : {&g->insp.tk, &g->mesh.tk, &g->bw.tk, &g->reach.tk})
    if (world > 1 && tk->on && tk->oneRank) {
      gs_set_error(std::string(tk->what) + ": not on a partitioned engine");
      return GS_EUNSUPPORTED;
    }
  if (world > 1 && (!tr || !tr->allgather_i64 || !tr->allgather || !tr->alltoallv)) {
    gs_set_error("a partitioned engine needs a transport with allgather_i64, allgather and alltoallv");
    return GS_EINVAL;
  }
  g->rank = rank;
  g->world = world;
  if (tr) g->tr = *tr;
  return GS_OK;
}

int gs_partition_range(const gs_engine* g, int32_t* node_begin, int32_t* node_end) {
  if (!g->graphSet) { gs_set_error("graph not set"); return GS_ESTATE; }
  const std::vector<int32_t> part = partition_bounds(g->rowptr, g->N, g->world);
  *node_begin = part[g->rank];
  *node_end = part[g->rank + 1];
  return GS_OK;
}

int gs_set_rpc_accounting(gs_engine* g, const int32_t* msg_size, int32_t id_len, const int32_t* topic_len) {
  if (g->started) { gs_set_error("gs_set_rpc_accounting: before the first step"); return GS_ESTATE; }
  if (!msg_size || !topic_len || id_len < 0) { gs_set_error("gs_set_rpc_accounting: bad arguments"); return GS_EINVAL; }
  for (int t = 0; t < g->T; ++t)
    if (msg_size[t] < 0 || topic_len[t] < 0) { gs_set_error("gs_set_rpc_accounting: negative size"); return GS_EINVAL; }
  g->acctOn = true;
  g->acctMsg.assign(msg_size, msg_size + g->T);
  g->acctTl.assign(topic_len, topic_len + g->T);
  g->acctIdLen = id_len;
  return GS_OK;
}

int gs_set_rpc_px_sizes(gs_engine* g, int32_t peer_id_len, int32_t record_len) {
  if (g->started) { gs_set_error("gs_set_rpc_px_sizes: before the first step"); return GS_ESTATE; }
  if (peer_id_len < 0 || record_len < 0) { gs_set_error("gs_set_rpc_px_sizes: negative size"); return GS_EINVAL; }
  g->acctPidLen = peer_id_len;
  g->acctRecLen = record_len;
  return GS_OK;
}

int gs_read_rpc_bytes(gs_engine* g, int64_t* bytes, int64_t* rpcs) {
  if (!g->acctOn) { gs_set_error("gs_read_rpc_bytes: accounting is off"); return GS_ESTATE; }
  const int64_t E = g->E;
  if (!g->started) {
    for (int64_t e = 0; e < E; ++e) {
      if (bytes) bytes[e] = 0;
      if (rpcs) rpcs[e] = 0;
    }
    return GS_OK;
  }
  std::vector<unsigned long long> b(E), n(E);
  HIPCHECK(hipStreamSynchronize(g->stream));
  // (owned edges only on the device, Dev::rxi)
  HIPCHECK(hipMemcpy(b.data() + g->e0, g->d.rpcB + g->e0, (size_t)g->eOwn * 8, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(n.data() + g->e0, g->d.rpcN + g->e0, (size_t)g->eOwn * 8, hipMemcpyDeviceToHost));
  for (int64_t e = 0; e < E; ++e) {
    const bool own = e >= g->e0 && e < g->e1;  // a partitioned rank reports its own edges
    if (bytes) bytes[e] = own ? (int64_t)b[e] : 0;
    if (rpcs) rpcs[e] = own ? (int64_t)n[e] : 0;
  }
  return GS_OK;
}

int gs_set_trace(gs_engine* g, const uint8_t* node_mask, int64_t capacity) {
  if (g->started) { gs_set_error("tracing must be set before the first step"); return GS_ESTATE; }
  if (node_mask && capacity <= 0) { gs_set_error("trace capacity must be positive"); return GS_EINVAL; }
  if (node_mask) g->traceMask.assign(node_mask, node_mask + g->N);
  else g->traceMask.clear();
  g->traceCap = capacity;
  return GS_OK;
}

int gs_set_dormant(gs_engine* g, int32_t n, const int32_t* a, const int32_t* b) {
  if (g->started) { gs_set_error("gs_set_dormant: before the first step"); return GS_ESTATE; }
  if (!g->graphSet) { gs_set_error("graph not set"); return GS_ESTATE; }
  if (n < 0 || (n > 0 && (!a || !b))) { gs_set_error("gs_set_dormant: bad arguments"); return GS_EINVAL; }
  for (int32_t i = 0; i < n; ++i) {
    bool ok = a[i] >= 0 && a[i] < g->N && b[i] >= 0 && b[i] < g->N;
    if (ok) {
      auto bgn = g->col.begin() + g->rowptr[a[i]], fin = g->col.begin() + g->rowptr[a[i] + 1];
      auto it = std::lower_bound(bgn, fin, b[i]);
      ok = it != fin && *it == b[i];
    }
    if (!ok) { gs_set_error("gs_set_dormant: not an edge of the graph"); return GS_EINVAL; }
    g->dormant.insert({std::min(a[i], b[i]), std::max(a[i], b[i])});
  }
  return GS_OK;
}

int gs_set_peertx_capacity(gs_engine* g, int32_t home_bits, int32_t overflow_bits) {
  if (g->started) { gs_set_error("the peertx capacity must be set before the first step"); return GS_ESTATE; }
  if (home_bits < 2 || home_bits > 16 || overflow_bits < 8 || overflow_bits > 30) {
    gs_set_error("gs_set_peertx_capacity: home_bits in [2, 16], overflow_bits in [8, 30]");
    return GS_EINVAL;
  }
  g->ptxHomeBits = home_bits;
  g->ptxOvfBits = overflow_bits;
  return GS_OK;
}

int gs_set_frontier_mode(gs_engine* g, int32_t mode) {
  if (g->started) { gs_set_error("the frontier mode must be set before the first step"); return GS_ESTATE; }
  if (mode != GS_FRONTIER_AUTO && mode != GS_FRONTIER_LISTS && mode != GS_FRONTIER_BITMAPS) {
    gs_set_error("gs_set_frontier_mode: GS_FRONTIER_AUTO, GS_FRONTIER_LISTS or GS_FRONTIER_BITMAPS");
    return GS_EINVAL;
  }
  g->frontierMode = mode;
  return GS_OK;
}

int gs_frontier_dense(const gs_engine* g) { return g->started && (g->denseFlood || g->denseGossip) ? 1 : 0; }

int gs_set_trace_rpc(gs_engine* g, int32_t on) {
  if (g->started) { gs_set_error("tracing must be set before the first step"); return GS_ESTATE; }
  g->traceRpc = on != 0;
  return GS_OK;
}

int gs_trace_read(gs_engine* g, gs_trace_event* out, int64_t cap, int64_t* n) {
  *n = 0;
  if (g->traceOut == 0 || g->traceOut == g->tracePending.size()) {
    GS_TRY(g->drainTrace());
  }
  const int64_t k = std::min<int64_t>(cap, (int64_t)(g->tracePending.size() - g->traceOut));
  std::copy(g->tracePending.begin() + g->traceOut, g->tracePending.begin() + g->traceOut + k, out);
  g->traceOut += (size_t)k;
  if (g->traceOut == g->tracePending.size()) {
    g->tracePending.clear();
    g->traceOut = 0;
  }
  *n = k;
  return GS_OK;
}

int gs_read_exchange_stats(gs_engine* g, double* host_ms, int64_t* bytes_in) {
  *host_ms = g->xMs;
  *bytes_in = g->xBytes;
  return GS_OK;
}

int64_t gs_num_edges(const gs_engine* g) { return g->E; }
int64_t gs_current_hop(const gs_engine* g) { return g->hop; }

int gs_read_counters(gs_engine* g, gs_counters* out) {
  std::memset(out, 0, sizeof(*out));
  if (g->started) {
    std::vector<unsigned long long> all((size_t)C_NCOUNTERS * GS_CTR_SPREAD);
    HIPCHECK(hipStreamSynchronize(g->stream));
    HIPCHECK(hipMemcpy(all.data(), g->d.ctr, all.size() * 8, hipMemcpyDeviceToHost));
    unsigned long long c[C_NCOUNTERS] = {};
    for (int s = 0; s < GS_CTR_SPREAD; ++s)
      for (int k = 0; k < C_NCOUNTERS; ++k) c[k] += all[(size_t)s * C_NCOUNTERS + k];
    out->published = (int64_t)c[C_PUBLISHED];
    out->deliveries = (int64_t)c[C_DELIVERIES];
    out->duplicates = (int64_t)c[C_DUPLICATES];
    out->transmissions = (int64_t)c[C_TRANSMISSIONS];
    out->grafts_sent = (int64_t)c[C_GRAFTS];
    out->prunes_sent = (int64_t)c[C_PRUNES];
    out->ihave_sent = (int64_t)c[C_IHAVE];
    out->iwant_sent = (int64_t)c[C_IWANT_SENT];
    out->iwant_served = (int64_t)c[C_IWANT_SERVED];
    out->promises_broken = (int64_t)c[C_PROMISES_BROKEN];
    out->graylisted = (int64_t)c[C_GRAYLISTED];
    out->rejected = (int64_t)c[C_REJECTED];
    out->throttled = (int64_t)c[C_THROTTLED];
    out->gated = (int64_t)c[C_GATED];
  }
  out->hops = g->hop;
  out->heartbeats = g->heartbeats;
  return GS_OK;
}

#define NEED_STARTED(g)                        \
  do {                                         \
    if (!(g)->started) {                       \
      GS_TRY((g)->start());                    \
    }                                          \
  } while (0)

int gs_read_scores(gs_engine* g, double* score) {
  if (!g->graphSet) { gs_set_error("graph not set"); return GS_ESTATE; }
  NEED_STARTED(g);
  score_rows<0>(g->d, g->eOwn, g->d.T, g->dScoreTmp, g->stream);
  // the owned edges (a partitioned rank's others read 0)
  std::memset(score, 0, (size_t)g->E * 8);
  HIPCHECK(hipMemcpyAsync(score + g->e0, g->dScoreTmp + g->e0, (size_t)g->eOwn * 8, hipMemcpyDeviceToHost, g->stream));
  HIPCHECK(hipStreamSynchronize(g->stream));
  if (g->mixed)  // only gossipsub hosts keep a peerScore (floodsub / randomsub: none, score 0)
    for (int u = 0; u < g->N; ++u)
      if (g->routerOf(u) != GS_ROUTER_GOSSIPSUB)
        for (int64_t e = g->rowptr[u]; e < g->rowptr[u + 1]; ++e) score[e] = 0.0;
  return GS_OK;
}

// A per-edge array (owned edges [e0, e1) on the device, Dev::rxi) into a
// host array of E entries; a partitioned rank's other entries read 0.
}  // extern "C"
template <class X>
static int copy_back_edges(gs_engine* g, X* dst, const X* src) {
  std::memset(dst, 0, (size_t)g->E * sizeof(X));
  if (!g->started) return GS_OK;
  HIPCHECK(hipStreamSynchronize(g->stream));
  HIPCHECK(hipMemcpy(dst + g->e0, src + g->e0, (size_t)g->eOwn * sizeof(X), hipMemcpyDeviceToHost));
  return GS_OK;
}
extern "C" {

int gs_read_mesh(gs_engine* g, uint64_t* mesh) { return copy_back_edges(g, mesh, g->d.mesh); }
int gs_read_fanout(gs_engine* g, uint64_t* fanout) { return copy_back_edges(g, fanout, g->d.fanout); }
int gs_read_backoff(gs_engine* g, int64_t* expire) { return copy_back_pairs(g, expire, g->d.backoff); }
int gs_read_topic_stats(gs_engine* g, double* fmd, double* mmd, double* mfp, double* imd, int64_t* mesh_time,
                        int64_t* graft_time, uint8_t* flags) {
  if (g->started && g->scoring) k_fold_all<<<nblk((int64_t)g->E * g->T, 256), 256, 0, g->stream>>>(g->d);
  GS_TRY(copy_back_pairs(g, fmd, g->d.fmd));
  GS_TRY(copy_back_pairs(g, mmd, g->d.mmd));
  GS_TRY(copy_back_pairs(g, mfp, g->d.mfp));
  GS_TRY(copy_back_pairs(g, imd, g->d.imd));
  GS_TRY(copy_back_pairs(g, mesh_time, (const int64_t*)g->d.meshTime));
  GS_TRY(copy_back_pairs(g, graft_time, (const int64_t*)g->d.graftTime));
  GS_TRY(copy_back_pairs(g, flags, (const uint8_t*)g->d.flags));
  // a mesh pair's meshTime is derived (mesh_time_of, gs_device.h)
  const int64_t lr = g->d.lastRefresh;
  for (int64_t i = 0; i < (int64_t)g->E * g->T; ++i) {
    if (flags[i] & 1) mesh_time[i] = graft_time[i] <= lr ? lr - graft_time[i] : 0;
    flags[i] &= GS_FL_PUB;  // (GS_FL_MFP is the engine's own)
  }
  return GS_OK;
}
int gs_read_behaviour_penalty(gs_engine* g, double* bp) { return copy_back_edges(g, bp, g->d.bp); }

// PubSubRouter.EnoughPeers of every owned host (gossip_engine.h), on the host
// from the mesh readback and the host mirrors of the announced subscriptions
// (subA), the connection states (aliveH) and the protocols.  A topic no peer
// announced counts as empty (the reference's missing p.topics entry).
int gs_enough_peers(gs_engine* g, int32_t topic, int32_t suggested, uint8_t* out) {
  if (topic < 0 || topic >= g->T || suggested < 0 || !out) { gs_set_error("gs_enough_peers: bad arguments"); return GS_EINVAL; }
  if (!g->started) { gs_set_error("gs_enough_peers: no state before the first step"); return GS_ESTATE; }
  std::vector<uint64_t> mesh((size_t)g->E);
  GS_TRY(copy_back_edges(g, mesh.data(), g->d.mesh));
  const uint64_t bit = 1ull << topic;
  std::memset(out, 0, (size_t)g->N);
  for (int u = g->n0; u < g->n1; ++u) {
    int fs = 0, rs = 0, gsn = 0, any = 0;
    for (int64_t e = g->rowptr[u]; e < g->rowptr[u + 1]; ++e) {
      if (!g->aliveH.empty() && !g->aliveH[e]) continue;
      if (!(g->subA[g->col[e]] & bit)) continue;
      const int pr = g->protoH[e];
      any++;
      fs += pr == GS_PROTO_FLOODSUB;
      rs += pr == GS_PROTO_RANDOMSUB;
      gsn += (mesh[e] & bit) != 0;
    }
    bool ok;
    switch (g->routerOf(u)) {
      case GS_ROUTER_GOSSIPSUB:  // gossipsub.go:549-576: floodsub peers = not mesh-capable
        ok = (fs + rs) + gsn >= (suggested ? suggested : g->gp.Dlo) || gsn >= g->gp.Dhi;
        break;
      case GS_ROUTER_RANDOMSUB:  // randomsub.go:59-89 (RandomSubD = 6)
        ok = fs + rs >= (suggested ? suggested : 6) || rs >= 6;
        break;
      default:  // floodsub.go:52-66 (FloodSubTopicSearchSize = 5)
        ok = any >= (suggested ? suggested : 5);
        break;
    }
    out[u] = ok ? 1 : 0;
  }
  return GS_OK;
}

int gs_read_topic_stats_edges(gs_engine* g, int64_t n, const int64_t* edges, double* fmd, double* mmd,
                              double* mfp, double* imd, int64_t* mesh_time, int64_t* graft_time,
                              uint8_t* flags) {
  if (n < 0 || (n > 0 && (!edges || !fmd || !mmd || !mfp || !imd || !mesh_time || !graft_time || !flags))) {
    gs_set_error("gs_read_topic_stats_edges: bad arguments");
    return GS_EINVAL;
  }
  for (int64_t i = 0; i < n; ++i)
    if (edges[i] < 0 || edges[i] >= g->E) { gs_set_error("gs_read_topic_stats_edges: edge out of range"); return GS_EINVAL; }
  const int64_t nk = n * g->T;
  if (!g->started || nk == 0) {
    std::fill(fmd, fmd + nk, 0.0); std::fill(mmd, mmd + nk, 0.0);
    std::fill(mfp, mfp + nk, 0.0); std::fill(imd, imd + nk, 0.0);
    std::fill(mesh_time, mesh_time + nk, 0); std::fill(graft_time, graft_time + nk, 0);
    std::fill(flags, flags + nk, 0);
    return GS_OK;
  }
  DevScratch<int64_t> dE((size_t)n);
  DevScratch<uint8_t> dOut((size_t)nk * 49);
  if (!dE.p || !dOut.p) {
    gs_set_error("device allocation failed (gs_read_topic_stats_edges)");
    return GS_ENOMEM;
  }
  std::vector<uint8_t> h((size_t)nk * 49);
  HIPCHECK(hipMemcpyAsync(dE.p, edges, (size_t)n * 8, hipMemcpyHostToDevice, g->stream));
  k_gather_pairs<<<nblk(nk, 256), 256, 0, g->stream>>>(g->d, dE.p, n, dOut.p);
  HIPCHECK(hipMemcpyAsync(h.data(), dOut.p, h.size(), hipMemcpyDeviceToHost, g->stream));
  HIPCHECK(hipStreamSynchronize(g->stream));
  const size_t b8 = (size_t)nk * 8;
  std::memcpy(fmd, h.data(), b8);
  std::memcpy(mmd, h.data() + b8, b8);
  std::memcpy(mfp, h.data() + 2 * b8, b8);
  std::memcpy(imd, h.data() + 3 * b8, b8);
  std::memcpy(mesh_time, h.data() + 4 * b8, b8);
  std::memcpy(graft_time, h.data() + 5 * b8, b8);
  std::memcpy(flags, h.data() + 6 * b8, (size_t)nk);
  return GS_OK;
}

int gs_read_backoff_edges(gs_engine* g, int64_t n, const int64_t* edges, int64_t* expire) {
  if (n < 0 || (n > 0 && (!edges || !expire))) { gs_set_error("gs_read_backoff_edges: bad arguments"); return GS_EINVAL; }
  for (int64_t i = 0; i < n; ++i)
    if (edges[i] < 0 || edges[i] >= g->E) { gs_set_error("gs_read_backoff_edges: edge out of range"); return GS_EINVAL; }
  const int64_t nk = n * g->T;
  if (!g->started || nk == 0) {
    std::fill(expire, expire + nk, 0);
    return GS_OK;
  }
  DevScratch<int64_t> dE((size_t)n), dOut((size_t)nk);
  if (!dE.p || !dOut.p) {
    gs_set_error("device allocation failed (gs_read_backoff_edges)");
    return GS_ENOMEM;
  }
  HIPCHECK(hipMemcpyAsync(dE.p, edges, (size_t)n * 8, hipMemcpyHostToDevice, g->stream));
  k_gather_backoff<<<nblk(nk, 256), 256, 0, g->stream>>>(g->d, dE.p, n, dOut.p);
  HIPCHECK(hipMemcpyAsync(expire, dOut.p, (size_t)nk * 8, hipMemcpyDeviceToHost, g->stream));
  HIPCHECK(hipStreamSynchronize(g->stream));
  return GS_OK;
}

int gs_read_deliveries(gs_engine* g, int64_t id, int32_t* hop, int32_t* from) {
  if (!g->record) { gs_set_error("GS_FLAG_RECORD_DELIVERIES not set"); return GS_ESTATE; }
  if (id < 0 || id >= (int64_t)g->mId.size()) { gs_set_error("unknown message id"); return GS_EINVAL; }
  const int slot = g->mSlot[id];
  if (g->slotOwnerId[slot] != id) {
    gs_set_error("message slot already recycled (window moved on)");
    return GS_ESTATE;
  }
  if (!g->started || g->mHop[id] >= g->hop) {
    for (int v = 0; v < g->N; ++v) { hop[v] = -1; from[v] = -1; }
    return GS_OK;
  }
  k_read_deliv<<<nblk(g->N, 256), 256, 0, g->stream>>>(g->d, slot, g->mHop[id], g->dHopOut, g->dFromOut);
  HIPCHECK(hipMemcpyAsync(hop, g->dHopOut, (size_t)g->N * 4, hipMemcpyDeviceToHost, g->stream));
  HIPCHECK(hipMemcpyAsync(from, g->dFromOut, (size_t)g->N * 4, hipMemcpyDeviceToHost, g->stream));
  HIPCHECK(hipStreamSynchronize(g->stream));
  return GS_OK;
}

// ---- latency statistics (include/gs_latency.h)
int gs_set_latency_stats(gs_engine* g, int32_t on) {
  if (g->started) { gs_set_error("latency statistics must be set before the first step"); return GS_ESTATE; }
  g->lat.on = on != 0;
  return GS_OK;
}

// The time and launches of the n kernel ids from `first` since the last
// gs_set_profiling, what is pending on a started engine's stream included.
static int readKernelStats(gs_engine* g, int first, int n, double* total_ms, int64_t* launches) {
  if (g->started) {
    HIPCHECK(hipStreamSynchronize(g->stream));
    g->resolveTimings();
  }
  for (int i = 0; i < n; ++i) {
    total_ms[i] = g->kMs[first + i];
    launches[i] = g->kLaunches[first + i];
  }
  return GS_OK;
}

static int latency_ready(const gs_engine* g) {
  if (!g->lat.on) { gs_set_error("latency statistics are off (gs_set_latency_stats)"); return GS_ESTATE; }
  if (!g->started) { gs_set_error("latency statistics: the engine has not started"); return GS_ESTATE; }
  return GS_OK;
}

int gs_latency_bins(const gs_engine* g) {
  GS_TRY(latency_ready(g));
  return g->latBins();
}

static int latency_bins_ok(const gs_engine* g, int32_t bins) {
  GS_TRY(latency_ready(g));
  if (bins != g->latBins()) {
    gs_set_error("latency statistics: bins must be gs_latency_bins() = " + std::to_string(g->latBins()));
    return GS_EINVAL;
  }
  return GS_OK;
}

int gs_read_latency_hist(gs_engine* g, int64_t* hist, int32_t bins) {
  GS_TRY(latency_bins_ok(g, bins));
  HIPCHECK(hipMemcpyAsync(hist, g->lat.dev.hist, (size_t)g->T * bins * 8, hipMemcpyDeviceToHost, g->stream));
  HIPCHECK(hipStreamSynchronize(g->stream));
  return GS_OK;
}

int gs_reset_latency_stats(gs_engine* g) {
  GS_TRY(latency_ready(g));
  HIPCHECK(hipMemsetAsync(g->lat.dev.hist, 0, (size_t)g->T * g->latBins() * 8, g->stream));
  return GS_OK;
}

int gs_read_message_latency(gs_engine* g, int64_t n, const int64_t* ids, uint32_t* hist, int32_t bins) {
  GS_TRY(latency_bins_ok(g, bins));
  for (int64_t i = 0; i < n; ++i) {
    if (ids[i] < 0 || ids[i] >= (int64_t)g->mId.size()) { gs_set_error("unknown message id"); return GS_EINVAL; }
    if (g->slotOwnerId[g->mSlot[ids[i]]] != ids[i]) {
      gs_set_error("message slot already recycled (window moved on)");
      return GS_ESTATE;
    }
  }
  for (int64_t i = 0; i < n; ++i) {
    uint32_t* row = hist + i * bins;
    if (g->mHop[ids[i]] >= g->hop)  // not yet published: its slot may still hold the earlier owner's row
      std::fill(row, row + bins, 0u);
    else
      HIPCHECK(hipMemcpyAsync(row, g->lat.dev.perMsg + (size_t)g->mSlot[ids[i]] * bins, (size_t)bins * 4,
                              hipMemcpyDeviceToHost, g->stream));
  }
  HIPCHECK(hipStreamSynchronize(g->stream));
  return GS_OK;
}

int gs_read_latency_kernel_stats(gs_engine* g, double* total_ms, int64_t* launches) {
  GS_TRY(latency_ready(g));
  return readKernelStats(g, gs_engine::kLatCount, gs_engine::kLatEnd - gs_engine::kLatCount, total_ms, launches);
}

// ---- WithPeerScoreInspect (include/gs_inspect.h)
int gs_set_score_inspect(gs_engine* g, const gs_inspect_config* c) {
  GS_TRY(g->insp.tk.configure(g, c, Ticker::kGossipsub | Ticker::kScoring));
  if (c->num_bounds < 0 || c->num_bounds > GS_INSPECT_MAX_BOUNDS || (c->num_bounds > 0 && !c->bounds)) {
    gs_set_error("score inspection: num_bounds must be 0.." + std::to_string(GS_INSPECT_MAX_BOUNDS));
    return GS_EINVAL;
  }
  for (int i = 0; i < c->num_bounds; ++i)
    if (!std::isfinite(c->bounds[i]) || (i > 0 && !(c->bounds[i - 1] < c->bounds[i]))) {
      gs_set_error("score inspection: bounds must be finite and strictly ascending");
      return GS_EINVAL;
    }
  g->insp.bounds.assign(c->bounds, c->bounds + c->num_bounds);
  g->insp.mask.clear();
  if (c->node_mask) g->insp.mask.assign(c->node_mask, c->node_mask + g->N);
  g->insp.ext = c->extended != 0;
  g->insp.tk.arm(c);
  return GS_OK;
}

int64_t gs_inspect_ticks(const gs_engine* g) { return g->insp.tk.ticksTaken(); }

int gs_inspect_num_edges(const gs_engine* g, int64_t* n) {
  GS_TRY(g->insp.tk.on_check());
  if (!g->started) { gs_set_error("score inspection: the engine has not started"); return GS_ESTATE; }
  *n = (int64_t)g->insp.dev.edges.size();
  return GS_OK;
}

int gs_inspect_edges(gs_engine* g, int64_t* edges, int64_t cap) {
  int64_t n = 0;
  GS_TRY(gs_inspect_num_edges(g, &n));
  if (cap < n || (n > 0 && !edges)) { gs_set_error("score inspection: edge buffer too small"); return GS_EINVAL; }
  std::copy(g->insp.dev.edges.begin(), g->insp.dev.edges.end(), edges);
  return GS_OK;
}

int gs_read_inspect_row(gs_engine* g, int64_t tick, int64_t* hop, int64_t* score_hist, int64_t* mesh_deg) {
  const Ticker& tk = g->insp.tk;
  GS_TRY(tk.tickOk(tick));
  if (hop) *hop = tk.hopOf(tick);
  const size_t nh = g->insp.bounds.size() + 1;
  const unsigned long long* row = g->insp.dev.rows + tk.slotOf(tick) * g->inspRowLen();
  if (score_hist) HIPCHECK(hipMemcpyAsync(score_hist, row, nh * 8, hipMemcpyDeviceToHost, g->stream));
  if (mesh_deg)
    HIPCHECK(hipMemcpyAsync(mesh_deg, row + nh, (size_t)g->T * GS_INSPECT_DEG_BINS * 8, hipMemcpyDeviceToHost,
                            g->stream));
  HIPCHECK(hipStreamSynchronize(g->stream));
  return GS_OK;
}

int gs_read_inspect_scores(gs_engine* g, int64_t tick, double* score) {
  GS_TRY(g->insp.tk.tickOk(tick));
  const size_t nS = g->insp.dev.edges.size();
  if (nS)
    HIPCHECK(hipMemcpyAsync(score, g->insp.dev.score + g->insp.tk.slotOf(tick) * nS, nS * 8, hipMemcpyDeviceToHost,
                            g->stream));
  HIPCHECK(hipStreamSynchronize(g->stream));
  return GS_OK;
}

int gs_read_inspect_snapshot(gs_engine* g, int64_t tick, double* app, double* ip_colocation,
                             double* behaviour_penalty, int64_t* time_in_mesh, double* fmd, double* mmd,
                             double* imd) {
  GS_TRY(g->insp.tk.tickOk(tick));
  if (!g->insp.ext) { gs_set_error("score inspection: the snapshot fields are not kept (extended = 0)"); return GS_ESTATE; }
  const size_t nS = g->insp.dev.edges.size(), nk = nS * (size_t)g->T;
  if (nS) {
    const double* x = g->insp.dev.ext + g->insp.tk.slotOf(tick) * g->inspExtLen();
    void* const dst[7] = {app, ip_colocation, behaviour_penalty, time_in_mesh, fmd, mmd, imd};
    size_t off = 0;
    for (int f = 0; f < 7; ++f) {
      const size_t len = f < 3 ? nS : nk;
      if (dst[f]) HIPCHECK(hipMemcpyAsync(dst[f], x + off, len * 8, hipMemcpyDeviceToHost, g->stream));
      off += len;
    }
  }
  HIPCHECK(hipStreamSynchronize(g->stream));
  return GS_OK;
}

int gs_read_inspect_kernel_stats(gs_engine* g, double* total_ms, int64_t* launches) {
  GS_TRY(g->insp.tk.on_check());
  return readKernelStats(g, gs_engine::kInspScore, gs_engine::kInspEnd - gs_engine::kInspScore, total_ms, launches);
}

// ---- mesh health (include/gs_mesh_health.h)
int gs_set_mesh_health(gs_engine* g, const gs_mesh_health_config* c) {
  GS_TRY(g->mesh.tk.configure(g, c, Ticker::kGossipsub));
  g->mesh.mask.clear();
  if (c->include) g->mesh.mask.assign(c->include, c->include + g->N);
  g->mesh.labels = c->labels != 0;
  g->mesh.tk.arm(c);
  return GS_OK;
}

int64_t gs_mesh_health_ticks(const gs_engine* g) { return g->mesh.tk.ticksTaken(); }

int gs_read_mesh_health_row(gs_engine* g, int64_t tick, int64_t* hop, int64_t* row, int64_t* comp_hist) {
  const Ticker& tk = g->mesh.tk;
  GS_TRY(tk.tickOk(tick));
  if (hop) *hop = tk.hopOf(tick);
  const size_t nf = (size_t)g->T * GS_MESH_ROW_FIELDS;
  const unsigned long long* src = g->mesh.dev.rows + tk.slotOf(tick) * (size_t)mesh_row_len(g->T);
  if (row) HIPCHECK(hipMemcpyAsync(row, src, nf * 8, hipMemcpyDeviceToHost, g->stream));
  if (comp_hist)
    HIPCHECK(hipMemcpyAsync(comp_hist, src + nf, (size_t)g->T * GS_MESH_SIZE_BINS * 8, hipMemcpyDeviceToHost,
                            g->stream));
  HIPCHECK(hipStreamSynchronize(g->stream));
  return GS_OK;
}

// The label table is the newest tick's until the next tick starts over.
int gs_read_mesh_labels(gs_engine* g, int64_t* tick, int32_t* labels) {
  GS_TRY(g->mesh.tk.on_check());
  if (!g->mesh.labels) { gs_set_error("mesh health: the label table is not kept (labels = 0)"); return GS_ESTATE; }
  if (g->mesh.tk.taken == 0) { gs_set_error("mesh health: no tick taken yet"); return GS_EINVAL; }
  if (tick) *tick = g->mesh.tk.taken - 1;
  if (labels)  // GS_MESH_NONE reads -1
    HIPCHECK(hipMemcpyAsync(labels, g->mesh.dev.L, (size_t)g->N * (size_t)g->T * 4, hipMemcpyDeviceToHost, g->stream));
  HIPCHECK(hipStreamSynchronize(g->stream));
  return GS_OK;
}

int gs_read_mesh_health_kernel_stats(gs_engine* g, double* total_ms, int64_t* launches) {
  GS_TRY(g->mesh.tk.on_check());
  GS_TRY(readKernelStats(g, gs_engine::kMeshInit, GS_MESH_ST_ITERS, total_ms, launches));
  total_ms[GS_MESH_ST_ITERS] = total_ms[GS_MESH_ST_BYTES] = 0.0;
  launches[GS_MESH_ST_ITERS] = g->mesh.iters;
  launches[GS_MESH_ST_BYTES] = g->mesh.bytes;
  return GS_OK;
}

// ---- bandwidth statistics (include/gs_bandwidth.h)
int gs_set_bandwidth_stats(gs_engine* g, const gs_bandwidth_config* c) {
  GS_TRY(g->bw.tk.configure(g, c, Ticker::kAccounting));
  if (c->num_bounds < 0 || c->num_bounds > GS_BW_MAX_BOUNDS || (c->num_bounds > 0 && !c->bounds)) {
    gs_set_error("bandwidth statistics: num_bounds must be 0.." + std::to_string(GS_BW_MAX_BOUNDS));
    return GS_EINVAL;
  }
  for (int i = 0; i < c->num_bounds; ++i)
    if (c->bounds[i] <= 0 || (i > 0 && !(c->bounds[i - 1] < c->bounds[i]))) {
      gs_set_error("bandwidth statistics: bounds must be positive and strictly ascending");
      return GS_EINVAL;
    }
  g->bw.bounds.assign(c->bounds, c->bounds + c->num_bounds);
  g->bw.nodes.clear();
  if (c->node_mask)
    for (int u = 0; u < g->N; ++u)
      if (c->node_mask[u]) g->bw.nodes.push_back(u);
  g->bw.tk.arm(c);
  return GS_OK;
}

int64_t gs_bandwidth_ticks(const gs_engine* g) { return g->bw.tk.ticksTaken(); }

int gs_bandwidth_num_nodes(const gs_engine* g, int64_t* n) {
  GS_TRY(g->bw.tk.on_check());
  *n = (int64_t)g->bw.nodes.size();
  return GS_OK;
}

int gs_bandwidth_nodes(gs_engine* g, int32_t* nodes, int64_t cap) {
  int64_t n = 0;
  GS_TRY(gs_bandwidth_num_nodes(g, &n));
  if (cap < n || (n > 0 && !nodes)) { gs_set_error("bandwidth statistics: node buffer too small"); return GS_EINVAL; }
  std::copy(g->bw.nodes.begin(), g->bw.nodes.end(), nodes);
  return GS_OK;
}

int gs_read_bandwidth_row(gs_engine* g, int64_t tick, int64_t* hop, int64_t* total, int64_t* total_rpcs,
                          int64_t* hist, int64_t* max, int64_t* argmax) {
  const Ticker& tk = g->bw.tk;
  GS_TRY(tk.tickOk(tick));
  if (hop) *hop = tk.hopOf(tick);
  const unsigned long long* row = g->bw.dev.rows + tk.slotOf(tick) * g->bwRowLen();
  const size_t nw = (size_t)GS_BW_DIRS * GS_BW_CLASSES;
  const auto get = [&](int64_t* dst, size_t at, size_t n) {
    return dst ? hipMemcpyAsync(dst, row + at, n * 8, hipMemcpyDeviceToHost, g->stream) : hipSuccess;
  };
  HIPCHECK(get(total, 0, GS_BW_CLASSES));
  HIPCHECK(get(total_rpcs, GS_BW_CLASSES, 1));
  HIPCHECK(get(max, GS_BW_ROW_MAX, nw));
  HIPCHECK(get(argmax, GS_BW_ROW_ARG, nw));
  HIPCHECK(get(hist, GS_BW_ROW_HIST, nw * (g->bw.bounds.size() + 1)));
  HIPCHECK(hipStreamSynchronize(g->stream));
  return GS_OK;
}

int gs_read_bandwidth_nodes(gs_engine* g, int64_t tick, int64_t* bytes, int64_t* rpcs) {
  GS_TRY(g->bw.tk.tickOk(tick));
  const size_t nS = g->bw.nodes.size(), slot = g->bw.tk.slotOf(tick);
  if (nS && bytes)
    HIPCHECK(hipMemcpyAsync(bytes, g->bw.dev.bytes + slot * nS * GS_BW_NODE_WORDS, nS * GS_BW_NODE_WORDS * 8,
                            hipMemcpyDeviceToHost, g->stream));
  if (nS && rpcs)
    HIPCHECK(hipMemcpyAsync(rpcs, g->bw.dev.rpcs + slot * nS * GS_BW_DIRS, nS * GS_BW_DIRS * 8, hipMemcpyDeviceToHost,
                            g->stream));
  HIPCHECK(hipStreamSynchronize(g->stream));
  return GS_OK;
}

int gs_read_bandwidth_kernel_stats(gs_engine* g, double* total_ms, int64_t* launches) {
  GS_TRY(g->bw.tk.on_check());
  return readKernelStats(g, gs_engine::kBwTick, GS_BW_NUM_STATS, total_ms, launches);
}

// ---- mesh reach (include/gs_mesh_reach.h)
int gs_set_mesh_reach(gs_engine* g, const gs_mesh_reach_config* c) {
  GS_TRY(g->reach.tk.configure(g, c, Ticker::kGossipsub));
  if (c->num_sources < 1 || c->num_sources > GS_REACH_MAX_SOURCES) {
    gs_set_error("mesh reach: num_sources must be 1 .. " + std::to_string(GS_REACH_MAX_SOURCES));
    return GS_EINVAL;
  }
  if (!c->sources) { gs_set_error("mesh reach: no sources given"); return GS_EINVAL; }
  std::vector<int32_t> src(c->sources, c->sources + c->num_sources), sorted(src);
  std::sort(sorted.begin(), sorted.end());
  if (sorted.front() < 0 || sorted.back() >= g->N) {
    gs_set_error("mesh reach: a source is outside 0 .. " + std::to_string(g->N - 1));
    return GS_EINVAL;
  }
  const auto dup = std::adjacent_find(sorted.begin(), sorted.end());
  if (dup != sorted.end()) {
    gs_set_error("mesh reach: source " + std::to_string(*dup) + " is given twice");
    return GS_EINVAL;
  }
  g->reach.src = std::move(src);
  g->reach.mask.clear();
  if (c->include) g->reach.mask.assign(c->include, c->include + g->N);
  g->reach.depths = c->depths != 0;
  g->reach.tk.arm(c);
  return GS_OK;
}

int64_t gs_mesh_reach_ticks(const gs_engine* g) { return g->reach.tk.ticksTaken(); }

int gs_read_mesh_reach_row(gs_engine* g, int64_t tick, int64_t* hop, int64_t* row, int64_t* depth_hist) {
  const Ticker& tk = g->reach.tk;
  GS_TRY(tk.tickOk(tick));
  if (hop) *hop = tk.hopOf(tick);
  const int K = (int)g->reach.src.size();
  const size_t nf = (size_t)K * g->T * GS_REACH_ROW_FIELDS;
  const unsigned long long* src = g->reach.dev.rows + tk.slotOf(tick) * (size_t)reach_row_len(K, g->T);
  if (row) HIPCHECK(hipMemcpyAsync(row, src, nf * 8, hipMemcpyDeviceToHost, g->stream));
  if (depth_hist)
    HIPCHECK(hipMemcpyAsync(depth_hist, src + nf, (size_t)K * g->T * GS_REACH_DEPTH_BINS * 8, hipMemcpyDeviceToHost,
                            g->stream));
  HIPCHECK(hipStreamSynchronize(g->stream));
  return GS_OK;
}

// The depth table is the newest tick's until the next tick starts over.
int gs_read_mesh_reach_depths(gs_engine* g, int64_t* tick, uint8_t* depths) {
  GS_TRY(g->reach.tk.on_check());
  if (!g->reach.depths) { gs_set_error("mesh reach: the depth table is not kept (depths = 0)"); return GS_ESTATE; }
  if (g->reach.tk.taken == 0) { gs_set_error("mesh reach: no tick taken yet"); return GS_EINVAL; }
  if (tick) *tick = g->reach.tk.taken - 1;
  if (depths)
    HIPCHECK(hipMemcpyAsync(depths, g->reach.dev.depths, g->reach.src.size() * (size_t)g->N * (size_t)g->T,
                            hipMemcpyDeviceToHost, g->stream));
  HIPCHECK(hipStreamSynchronize(g->stream));
  return GS_OK;
}

int gs_read_mesh_reach_kernel_stats(gs_engine* g, double* total_ms, int64_t* launches) {
  GS_TRY(g->reach.tk.on_check());
  GS_TRY(readKernelStats(g, gs_engine::kReachMembers, GS_REACH_ST_PASSES, total_ms, launches));
  total_ms[GS_REACH_ST_PASSES] = total_ms[GS_REACH_ST_LEVELS] = total_ms[GS_REACH_ST_BYTES] = 0.0;
  launches[GS_REACH_ST_PASSES] = g->reach.passes;
  launches[GS_REACH_ST_LEVELS] = g->reach.levels;
  launches[GS_REACH_ST_BYTES] = g->reach.bytes;
  return GS_OK;
}

#ifdef GS_STAMPS
// Debug build: phase-A cycle stamps of the sampled nodes of the last hop.
int gs_debug_stamps(gs_engine* g, unsigned long long* out, int n) {
  HIPCHECK(hipStreamSynchronize(g->stream));
  HIPCHECK(hipMemcpy(out, g->d.stamps, (size_t)n * 8, hipMemcpyDeviceToHost));
  return GS_OK;
}
// Debug build: the peertx entry count of every owned node.
int gs_debug_ptxn(gs_engine* g, int32_t* out, int n) {
  HIPCHECK(hipStreamSynchronize(g->stream));
  HIPCHECK(hipMemcpy(out, g->d.ptxN + g->n0, (size_t)n * 4, hipMemcpyDeviceToHost));
  return GS_OK;
}
#endif

int gs_set_profiling(gs_engine* g, int on) {
  if (g->started) {
    HIPCHECK(hipStreamSynchronize(g->stream));
    g->resolveTimings();
  }
  g->profiling = on != 0;
  for (int i = 0; i < gs_engine::kTimed; ++i) { g->kMs[i] = 0; g->kLaunches[i] = 0; }
  g->mesh.iters = g->mesh.bytes = 0;
  g->reach.passes = g->reach.levels = g->reach.bytes = 0;
  return GS_OK;
}

int gs_read_kernel_stats(gs_engine* g, double* total_ms, int64_t* launches) {
  return readKernelStats(g, 0, GS_NUM_KERNELS, total_ms, launches);
}

}  // extern "C"
