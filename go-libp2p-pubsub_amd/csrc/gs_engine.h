// gs_engine.h — the engine record behind the C-ABI handle and its device
// memory layer: the error macros, the growable and the scope-bound device
// buffers, and struct gs_engine with its allocators.  Included by
// gs_engine.hip only (the kernels below are non-inline definitions).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "../../include/gossip_engine.h"
#include "../../include/gs_proto.h"
#include "../../include/gs_rpcsize.h"
#include "../../include/gs_trace.h"
#include "../../include/gs_latency.h"
#include "../../include/gs_inspect.h"
#include "../../include/gs_mesh_health.h"
#include "../../include/gs_mesh_reach.h"
#include "../../include/gs_bandwidth.h"
#include "../../include/gs_window.h"
#include "gs_window_layout.h"
#include "gs_host.h"
#include "gs_kernels.h"
#include "gs_kernels_ctl.h"
#include "gs_kernels_lat.h"
#include "gs_kernels_insp.h"
#include "gs_kernels_mesh.h"
#include "gs_kernels_reach.h"
#include "gs_kernels_bw.h"
#include "gs_exchange.h"

#define HIPCHECK(expr)                                                        \
  do {                                                                        \
    hipError_t _e = (expr);                                                   \
    if (_e != hipSuccess) {                                                   \
      gs_set_error(std::string("HIP error: ") + hipGetErrorString(_e) + " at " #expr); \
      return GS_EDEVICE;                                                      \
    }                                                                         \
  } while (0)

// Returns a failing GS_* code of `expr` to the caller.
#define GS_TRY(expr)           \
  do {                         \
    const int _rc = (expr);    \
    if (_rc) return _rc;       \
  } while (0)

static const int64_t kSec = 1000000000LL;

// A growable device buffer.  reserve(n) leaves room for n elements: it grows
// by at least half the capacity (1024 elements at first), keeps the first
// `keep` elements, and frees the outgrown buffer only after the engine's
// stream has drained, since queued kernels may still hold its address.
template <class X>
struct DevBuf {
  hipStream_t* stream;
  const char* what;  // names the buffer in the out-of-memory message
  X* p = nullptr;
  size_t cap = 0;
  DevBuf(hipStream_t* s, const char* w) : stream(s), what(w) {}
  DevBuf(const DevBuf&) = delete;
  ~DevBuf() { free(); }
  void free() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  int reserve(size_t n, size_t keep = 0) {
    if (n <= cap) return GS_OK;
    const size_t ncap = std::max({n, cap + cap / 2, (size_t)1024});
    X* q = nullptr;
    if (hipMalloc(&q, ncap * sizeof(X)) != hipSuccess) {
      gs_set_error(std::string("device allocation failed (") + what + ")");
      return GS_ENOMEM;
    }
    if (p && keep) HIPCHECK(hipMemcpyAsync(q, p, std::min(keep, cap) * sizeof(X), hipMemcpyDeviceToDevice, *stream));
    if (p) {
      HIPCHECK(hipStreamSynchronize(*stream));
      HIPCHECK(hipFree(p));
    }
    p = q;
    cap = ncap;
    return GS_OK;
  }
};

// Device scratch of one call, released when it leaves scope (p stays null if
// the allocation failed).
template <class X>
struct DevScratch {
  X* p = nullptr;
  explicit DevScratch(size_t n) {
    if (hipMalloc(&p, std::max<size_t>(n * sizeof(X), 16)) != hipSuccess) p = nullptr;
  }
  DevScratch(const DevScratch&) = delete;
  ~DevScratch() { (void)hipFree(p); }
};

struct gs_engine {
  gs_config cfg{};
  gs_gossipsub_params gp{};
  gs_peer_score_params sp{};
  gs_peer_score_thresholds thr{};
  std::vector<gs_topic_score_params> tps;
  std::vector<uint8_t> tscored;
  bool scoring = false, floodPublish = false, record = false;
  int N = 0, T = 0, St = 0, Wt = 0, W = 0, S = 0, R = 0;
  int64_t E = 0;
  int H = 16;  // hops per heartbeat (or a nominal 16 for floodsub/randomsub)
  int64_t retireHops = 0;  // the policy's (setWindow); a topic's own: retireOf(t)
  // topic windows (gs_window.h): the layout (St / Wt: the largest topic's), the
  // caller's age limits (0: the policy's) and the largest age in force
  gsw::Layout lay;
  std::vector<int32_t> userAge;
  int ageMax = 0;
  bool windowsSet = false;  // gs_set_topic_windows was called: the publish guard names the topic
  bool agesSet() const { return std::any_of(userAge.begin(), userAge.end(), [](int32_t a) { return a > 0; }); }
  int ageOf(int t) const { return userAge[(size_t)t] > 0 ? userAge[(size_t)t] : maxAge; }
  int64_t retireOf(int t) const {
    return gsw::retireHops(ageOf(t), cfg.router == GS_ROUTER_GOSSIPSUB, gp.HistoryLength, H);
  }
  void setLayout(const gsw::Layout& L) {
    lay = L;
    St = L.maxSlots; Wt = L.maxWords(); W = L.W; S = L.S;
  }
  std::vector<int32_t> topicLive;  // per-topic live message count (phase-A counter width)
  int64_t hopsSinceFold = 0, foldEvery = 1;  // pending-delivery fold cadence (dlt)
  int64_t eOwn = 0;                          // owned edges e1 - e0 (Dev::eOwn)
  // the 16-bit pending counts (Dev::dltN): counts accumulate from foldStart;
  // a pair's count is bounded by the messages of its topic that can be
  // delivered since then, so the host folds before that bound could pass 255
  bool narrowDlt = false;
  int64_t foldStart = 0;
  // Does some topic t have more than 255 messages published in [from - retireOf(t), hi]
  // (its own retire horizon before `from`)?
  bool topicOver255(int64_t from, int64_t hi) {
    int64_t back = 0;
    for (int t = 0; t < T; ++t) back = std::max(back, retireOf(t));
    auto it = std::lower_bound(mHop.begin(), mHop.end(), from - back);
    std::fill(topicLive.begin(), topicLive.end(), 0);
    for (size_t k = (size_t)(it - mHop.begin()); k < mHop.size() && mHop[k] <= hi; ++k)
      if (mHop[k] >= from - retireOf(mTopic[k]) && ++topicLive[mTopic[k]] > 255) return true;
    return false;
  }
  bool narrowFoldDue(int64_t h) { return topicOver255(foldStart, h); }
  std::vector<uint64_t> yWord, yTabH;          // phase A young-slot tables (per hop)
  size_t ldsLimit = 0, ldsStaticA = 0;         // LDS per workgroup of the device; phase A's static share
  int64_t refreshedHop = -1;                 // hop of the last refreshScores (S0 exact after it)
  int maxAge = 0;
  // host graph / attributes
  std::vector<int64_t> rowptr;
  std::vector<int32_t> col, rev, esrc;
  std::vector<uint8_t> outbound, direct;
  // mixed networks (gs_set_routers / gs_set_graph_ex): the router of every
  // host and the protocol of every connection (protoGiven: the caller's;
  // otherwise validateMixed fills in the negotiated ones)
  std::vector<uint8_t> routerH, protoH;
  bool mixed = false, protoGiven = false;
  int validateMixed();
  int routerOf(int u) const {  // GS_ROUTER_* with the v1.0 variant folded into gossipsub
    const int r = routerH.empty() ? cfg.router : (int)routerH[u];
    return r == GS_ROUTER_GOSSIPSUB_V10 ? GS_ROUTER_GOSSIPSUB : r;
  }
  std::vector<uint64_t> sub;
  std::vector<double> app;
  std::vector<uint32_t> ipv4;
  std::vector<std::pair<uint32_t, uint32_t>> whitelist;
  // connection churn and subscription changes (gs_schedule_events)
  struct Event { int64_t hop; int32_t kind, a, b; };
  std::vector<Event> events;
  size_t nextEv = 0;
  struct Ann { int node, topic; bool sub; };
  std::vector<Ann> pendAnn;            // announcements arriving next hop
  std::vector<uint64_t> subA;          // announced subscriptions (host copy of d.subA)
  std::vector<uint8_t> aliveH;         // [E] host copy of d.alive
  bool churnOn = false;
  // push (k_push + phase A reading per-edge segments) pays where an edge
  // forwards a fraction of its sender's list: several topics.  With one topic
  // a forwarding edge carries the whole list and phase A reads the lists.
  bool pushOn = false;
  // floodsub on dense frontiers (k_flood_a): a single-router floodsub engine
  // with nothing that needs a per-copy record (trace, RPC accounting, churn,
  // dormant slots, validators, attackers) on one rank
  bool denseFlood = false;
  // gossipsub on one topic (config3's shape): phase A pass 1 ORs the senders'
  // frontier bitmaps (k_phase_a DENSE); the lists stay for every other reader
  bool denseGossip = false;
  int frontierMode = 0;                // gs_set_frontier_mode: 0 auto, 1 lists only
  WMask amWPar[2]{};                   // denseGossip: amW of the last hop of each parity
  bool churnWindow = false;            // events scheduled before the first publish: wide window
  uint64_t* dSubA = nullptr;
  uint64_t* dSubOwn = nullptr;
  double* dP6w = nullptr;              // writable view of d.p6 (k_p6)
  bool p6Live() const { return scoring && sp.IPColocationFactorWeight != 0 && !ipv4.empty(); }
  int enableChurn();
  int applyEvents(int64_t h);
  int uploadList(const std::vector<int32_t>& v);
  bool graphSet = false, started = false;
  // schedule
  int64_t hop = 0;
  uint64_t ticks = 0;
  int head = 0;
  int64_t heartbeats = 0;
  std::vector<int32_t> mSrc, mTopic, mSlot;
  std::vector<int64_t> mId, mHop;
  std::vector<uint8_t> mKind;          // GS_MSG_* per message
  // adversarial model (gs_set_validation / gs_set_behaviour / WithPeerGater)
  uint64_t topicVal = 0;
  int32_t valQueue = 0;
  std::vector<uint8_t> behaveH;
  std::vector<int32_t> spamRowH;  // host copy of Dev::spamRow
  uint8_t behaveAll = 0;               // OR of every node's bits
  bool anyPhantom = false;             // a published id is advertised only (GS_MSG_PHANTOM)
  bool gaterOn = false;
  gs_peer_gater_params gaterP{};
  // validators, the gater or attackers: the kernels' ADV instantiations
  bool advModel() const { return topicVal != 0 || gaterOn || behaveAll != 0; }
  bool gaterDecayDue(int64_t t) const { return gaterOn && t > 0 && t % gaterP.DecayInterval == 0; }
  size_t uploaded = 0, nextMsg = 0;
  std::vector<int64_t> topicCounter, slotOwnerHop, slotOwnerId;
  // device
  Dev d{};
  hipStream_t stream = nullptr;
  TopicP* dTp = nullptr;
  double* dScoreTmp = nullptr;
  int32_t *dHopOut = nullptr, *dFromOut = nullptr;
  // partition (gs_set_partition; world == 1: the whole graph)
  int rank = 0, world = 1;
  gs_transport tr{};
  std::vector<int32_t> part;  // [world + 1] node boundaries
  int32_t n0 = 0, n1 = 0;
  int64_t e0 = 0, e1 = 0, poolSeg = 0;
  int nOwn() const { return n1 - n0; }

  // ---- device memory layer ----
  // Fixed-size allocations live until release(); a failed one sets allocFailed
  // and returns null, and the stage that made it reports through allocFail().
  std::vector<void*> allocs;
  bool allocFailed = false;
  template <class X>
  X* dalloc(size_t n, int fill = 0) {
    void* p = nullptr;
    size_t bytes = std::max<size_t>(n * sizeof(X), 16);
    if (hipMalloc(&p, bytes) != hipSuccess) {
      allocFailed = true;
      return nullptr;
    }
    allocs.push_back(p);
    (void)hipMemsetAsync(p, fill, bytes, stream);
    return (X*)p;
  }
  int allocFail(const char* group, const char* hint = "") {  // GS_ENOMEM if an allocation has failed since the last call
    if (!allocFailed) return GS_OK;
    allocFailed = false;
    gs_set_error(std::string("device allocation failed (") + group + ")" + hint);
    return GS_ENOMEM;
  }
  // Per-edge device arrays (Dev::rxi): a sender-indexed array holds `rows`
  // values of the owned edges [e0, e1), a receiver-indexed one (outbox, fwdIn,
  // ibxRec) also the stage [e1, e1 + eOwn) on a partitioned rank; both through
  // a base shifted by e0.  Unpartitioned: [0, E), as before.
  template <class X>
  X* ealloc(int fill = 0, size_t rows = 1) {
    X* p = dalloc<X>(rows * (size_t)std::max<int64_t>(eOwn, 1), fill);
    return p ? p - e0 : nullptr;
  }
  template <class X>
  X* ralloc(int fill = 0) {
    X* p = dalloc<X>((size_t)std::max<int64_t>(world > 1 ? 2 * eOwn : eOwn, 1), fill);
    return p ? p - e0 : nullptr;
  }
  // Rows of the owned nodes [n0, n1), n elements each, through a base shifted
  // by n0 rows; rows of the owned (edge, topic) pairs e*T + t (and 64 of slack),
  // through a base shifted by e0*T.
  template <class X>
  X* nalloc(size_t n, int fill = 0) {
    X* p = dalloc<X>((size_t)nOwn() * n, fill);
    return p ? p - (size_t)n0 * n : nullptr;
  }
  template <class X>
  X* palloc(int fill = 0) {
    X* p = dalloc<X>((size_t)T * (size_t)eOwn + 64, fill);
    return p ? p - e0 * T : nullptr;
  }
  // One-shot uploads from pageable host memory, skipped after a failed
  // allocation (the stage's allocFail reports it).  putNow returns once the
  // stream has drained, so src may die; after put alone it must live until
  // then.
  template <class X>
  int put(const X* dst, const X* src, size_t n) {
    if (allocFailed || !n) return GS_OK;
    HIPCHECK(hipMemcpyAsync(const_cast<X*>(dst), src, n * sizeof(X), hipMemcpyHostToDevice, stream));
    return GS_OK;
  }
  template <class X>
  int putNow(const X* dst, const X* src, size_t n) {
    GS_TRY(put(dst, src, n));
    HIPCHECK(hipStreamSynchronize(stream));
    return GS_OK;
  }
  template <class X>
  int putEdges(const X* dst, const std::vector<X>& src) {  // the owned edges [e0, e1) of a per-edge array
    return putNow(dst + e0, src.data() + e0, (size_t)eOwn);
  }
  DevBuf<int32_t> evBuf{&stream, "event list"}, pairsBuf{&stream, "fanout pairs"}, retireBuf{&stream, "retired words"};
  DevBuf<int64_t> acctBuf{&stream, "RPC accounting list"};
  // the published messages (Dev::mSrc ...): five arrays reserved together
  DevBuf<int32_t> msgSrc{&stream, "messages"}, msgTopic{&stream, "messages"}, msgSlot{&stream, "messages"};
  DevBuf<int64_t> msgId{&stream, "messages"};
  DevBuf<uint8_t> msgKind{&stream, "messages"};
  // exchange buffers (device) and the pinned host staging of the counts
  DevBuf<uint8_t> xSend{&stream, "exchange buffer"}, xRecv{&stream, "exchange buffer"},
      xSendE{&stream, "exchange buffer"}, xRecvE{&stream, "exchange buffer"};
  unsigned long long* xCnt = nullptr;  // device: gsx::XCnt
  int64_t* xOff = nullptr;             // device: [world] first record per destination (SendPlan::recOff)
  unsigned long long* xHost = nullptr; // pinned: gsx::Readback
  // cross-rank push (gs_exchange.h k_xp_*): send blocks, device counters
  // (gsx::XpCnt), k_xp_pack's offsets (gsx::XpOff); a parity's push arena
  // ibx[k] (bytes) receives the blocks past the owned senders' regions
  // (ibxOwnSlots)
  DevBuf<uint8_t> xSendP{&stream, "exchange buffer"};
  DevBuf<uint8_t> ibx[2]{{&stream, "exchange buffer"}, {&stream, "exchange buffer"}};
  unsigned long long* xpCnt = nullptr;
  int64_t* xpOff = nullptr;
  int64_t ibxOwnSlots = 0;
  double xMs = 0.0;                    // host wall time spent in exchanges
  int64_t xBytes = 0;                  // bytes received by this rank
  // One hop's exchange (gs_exchange.h, layouts in gs_exchange_wire.h): what its
  // steps hand on.
  struct Xchg {
    int cur;
    bool hb;
    bool xpush;          // k_push ran: cross-rank edges' segments travel too
    bool lists = true;   // the frontier lists travel this hop
    int64_t nPool = 0;   // arena ids of this rank's segment
    gsx::Bcast bc{};     // this rank's chunk
    gsx::SendPlan sp;
    std::vector<int64_t> all;  // every rank's SizeRow
    gsx::RecvPlan rp;
  };
  int exchange(int cur, bool hb);
  void xPackLists(const Xchg& x);
  int xCount(Xchg& x), xPackBroadcast(Xchg& x), xPackRecords(Xchg& x), xPackPush(Xchg& x);
  int xAgreeSizes(Xchg& x);
  int xGatherChunks(Xchg& x), xGatherDials(Xchg& x), xSwapRecords(Xchg& x), xSwapPush(Xchg& x);
  int xUnpack(Xchg& x);
  // trace events (gs_set_trace / gs_trace_read)
  std::vector<uint8_t> traceMask;
  int64_t traceCap = 0;
  // RPC byte accounting (gs_set_rpc_accounting)
  bool acctOn = false;
  std::vector<int32_t> acctMsg, acctTl;
  int32_t acctIdLen = 0;
  int32_t acctPidLen = 38, acctRecLen = 0;  // PX PeerInfo (gs_set_rpc_px_sizes)
  std::vector<int64_t> acctPend;        // (edge, bytes) pairs sent by the host side this hop
  int64_t helloBytes(uint64_t subs) const {  // getHelloPacket: one SubOpts per subscribed topic
    int64_t b = 0;
    for (int t = 0; t < T; ++t)
      if ((subs >> t) & 1) b += gs_pb_field(gs_pb_subopts(acctTl[t]));
    return b;
  }
  int flushAcct();
  std::vector<gs_trace_event> tracePending;  // converted, canonical order from traceOut
  // RPC events (gs_set_trace_rpc): RECV blocks of hops not run yet, and the
  // connections closed at the start of a hop (their in-flight RPCs are lost)
  bool traceRpc = false;
  int ptxHomeBits = -1, ptxOvfBits = -1;  // gs_set_peertx_capacity (-1: defaults)
  // peer exchange (GS_FLAG_PEER_EXCHANGE) and connections down at the start
  bool doPX = false;
  std::set<std::pair<int, int>> dormant;       // gs_set_dormant (a < b)
  std::vector<std::pair<int, int>> pxPend;     // dials of the previous hop (connected at this hop's start)
  std::vector<unsigned long long> pxqH;
  int readPx();
  // direct peers (gossipsub.go:492-502, 1594-1616): the (host, direct peer)
  // edges, dialled by the connector when down
  std::vector<std::pair<int, int>> directPairs;
  int64_t directInitHop = 0;
  void directConnect() {
    for (auto& pr : directPairs) {
      const auto bgn = col.begin() + rowptr[pr.first], fin = col.begin() + rowptr[pr.first + 1];
      if (!aliveH.empty() && !aliveH[std::lower_bound(bgn, fin, pr.second) - col.begin()])
        pxPend.push_back({std::min(pr.first, pr.second), std::max(pr.first, pr.second)});
    }
  }
  std::vector<gs_trace_event> traceFuture;
  std::vector<std::array<int64_t, 3>> rpcDowns;  // (hop, receiver, sender)
  // an RPC block recorded on the host: hello packets and announcements
  void hostRpc(int type, int node, int peer, int64_t h, int64_t ord, int topicSub, uint64_t subs, int subFlag) {
    if (!traceRpc || traceMask.empty() || !traceMask[node] || node < n0 || node >= n1) return;
    tracePending.push_back(gs_trace_event{h, ord, type, node, peer, -1, 0, 0});
    for (int t = 0; t < T; ++t)
      if (((subs >> t) & 1) || t == topicSub)
        tracePending.push_back(gs_trace_event{h, t == topicSub ? subFlag : 1, GS_TRACE_RPC_ITEM, node, peer,
                                              (int16_t)t, 0, GS_RPC_ITEM_SUB});
  }
  size_t traceOut = 0;
  int drainTrace();
  // latency statistics (gs_latency.h): the per-message and per-topic tables
  // ([S][bins] and [T][bins], bins = the largest age limit + 1; Dev::latCnt holds a hop's
  // counts) and the grid of k_lat_count
  bool latOn = false;
  uint32_t* dLatM = nullptr;
  unsigned long long* dLatH = nullptr;
  unsigned latGrid = 0;
  int latBins() const { return ageMax + 1; }
  // WithPeerScoreInspect (gs_inspect.h): a ring of inspCap ticks, each a row
  // (insp_row_len: score_hist, then mesh_deg), the sampled edges' scores and,
  // extended, their snapshot fields (k_inspect_gather's layout)
  bool inspOn = false, inspExt = false;
  int64_t inspPeriod = 0, inspTaken = 0;
  int inspCap = 0;
  std::vector<double> inspBounds;
  std::vector<uint8_t> inspMask;     // [N] observers, or empty
  std::vector<int64_t> inspEdges;    // the sampled edges of this rank, ascending
  unsigned long long* dInspRows = nullptr;
  double *dInspBounds = nullptr, *dInspScore = nullptr, *dInspExt = nullptr;
  int64_t* dInspEdges = nullptr;
  unsigned inspGrid = 0;
  int inspRowLen() const { return insp_row_len((int)inspBounds.size(), T); }
  size_t inspExtLen() const { return inspEdges.size() * (3 + 4 * (size_t)T); }  // 8-byte words per tick
  // mesh health (gs_mesh_health.h): the label and size tables (uint32 [N][T]),
  // a ring of meshCap rows (mesh_row_len), the batch's flags and the word count
  bool meshOn = false, meshLabels = false;
  int64_t meshPeriod = 0, meshTaken = 0;
  int meshCap = 0;
  std::vector<uint8_t> meshMask;     // [N] the hosts counted, or empty for all
  uint8_t* dMeshMask = nullptr;
  uint32_t *dMeshL = nullptr, *dMeshZ = nullptr, *dMeshFlag = nullptr;  // flags: [GS_MESH_BATCH + 1]
  unsigned long long *dMeshRows = nullptr, *dMeshWords = nullptr;
  unsigned meshGrid = 0;
  int64_t meshIters = 0, meshBytes = 0;  // since the start or the last gs_set_profiling
  // mesh reach (gs_mesh_reach.h): the two bit tables (uint64 [N][T]), a ring of
  // reachCap rows (reach_row_len), the members per topic, the batch's flags,
  // the byte counters and, when asked for, the depth table (uint8 [K][N][T])
  bool reachOn = false, reachDepths = false;
  int64_t reachPeriod = 0, reachTaken = 0;
  int reachCap = 0;
  std::vector<int32_t> reachSrc;      // [K] the sources
  std::vector<uint8_t> reachMask;     // [N] the hosts that can be targets, or empty for all
  int32_t* dReachSrc = nullptr;
  uint8_t *dReachMask = nullptr, *dReachDepths = nullptr;
  uint64_t* dReachR[2] = {nullptr, nullptr};
  uint32_t *dReachMembers = nullptr, *dReachFlag = nullptr;  // flags: [GS_REACH_BATCH + 1]
  unsigned long long *dReachRows = nullptr, *dReachWords = nullptr;
  unsigned reachGrid = 0;
  int64_t reachPasses = 0, reachLevels = 0, reachBytes = 0;  // since the start or the last gs_set_profiling
  // bandwidth statistics (gs_bandwidth.h): the per-node tables (uint64 [N][8]:
  // the cumulative sums at the previous tick, this tick's deltas), a ring of
  // bwCap rows (bw_row_len) and the sampled nodes' values (k_bw_gather's layout)
  bool bwOn = false;
  int64_t bwPeriod = 0, bwTaken = 0;
  int bwCap = 0;
  std::vector<int64_t> bwBounds;
  std::vector<int32_t> bwNodes;      // the sampled nodes, ascending
  long long* dBwBounds = nullptr;
  int32_t* dBwNodes = nullptr;
  unsigned long long *dBwPrev = nullptr, *dBwDelta = nullptr, *dBwRows = nullptr, *dBwBytes = nullptr, *dBwRpcs = nullptr;
  unsigned bwGrid = 0;
  int bwRowLen() const { return bw_row_len((int)bwBounds.size()); }
  // kernel timing: (kernel id, start event, end event) pending until a sync
  bool profiling = false;
  std::vector<hipEvent_t> evPool;
  size_t evUsed = 0;
  std::vector<int> pendKid;
  // (past the public kernel ids: the latency kernels, gs_read_latency_kernel_stats, and the
  // inspection's three passes, gs_read_inspect_kernel_stats; mesh health's four,
  // gs_read_mesh_health_kernel_stats; mesh reach's four, gs_read_mesh_reach_kernel_stats; the
  // bandwidth statistics' three, gs_read_bandwidth_kernel_stats)
  static constexpr int kLatCount = GS_NUM_KERNELS, kLatFold = GS_NUM_KERNELS + 1;
  static constexpr int kInspScore = GS_NUM_KERNELS + 2, kInspReduce = GS_NUM_KERNELS + 3;
  static constexpr int kInspGather = GS_NUM_KERNELS + 4, kMeshInit = GS_NUM_KERNELS + 5;
  static constexpr int kReachMembers = kMeshInit + 4;  // (kMeshInit + GS_MESH_K_*)
  static constexpr int kBwTick = kReachMembers + 4;    // (kReachMembers + GS_REACH_K_*)
  static constexpr int kTimed = kBwTick + GS_BW_NUM_STATS;  // (kBwTick + GS_BW_K_*)
  double kMs[kTimed] = {0};
  int64_t kLaunches[kTimed] = {0};
  hipEvent_t nextEvent() {
    if (evUsed == evPool.size()) {
      hipEvent_t ev;
      (void)hipEventCreate(&ev);
      evPool.push_back(ev);
    }
    return evPool[evUsed++];
  }
  void resolveTimings() {  // call after a stream sync
    for (size_t i = 0; i < pendKid.size(); ++i) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, evPool[2 * i], evPool[2 * i + 1]) == hipSuccess) kMs[pendKid[i]] += ms;
      kLaunches[pendKid[i]]++;
    }
    pendKid.clear();
    evUsed = 0;
  }

  // Pinned staging ring for the per-hop host-to-device uploads: the copy is
  // asynchronous on the engine stream and the host goes on preparing the next
  // hop; a slot is refilled only after the copy that used it has completed.
  struct Stage {
    void* p = nullptr;
    size_t cap = 0;
    hipEvent_t ev = nullptr;
    bool used = false;
  };
  static constexpr int kStages = 16;
  Dev* dDev = nullptr;  // device copy of d for the kernels that take it by pointer (k_phase_a / k_phase_b)
  Stage stages[kStages];
  int stageNext = 0;
  // uploads above kStageMax (the full N x 8 subscription rows of an
  // announcement hop: 80 MB at 10M peers) share one pinned buffer instead of
  // growing every ring slot to their size
  static constexpr size_t kStageMax = (size_t)4 << 20;
  Stage bigStage;
  int upload(void* dst, const void* src, size_t bytes) {
    if (!bytes) return GS_OK;
    Stage& st = bytes > kStageMax ? bigStage : stages[stageNext];
    if (&st != &bigStage) stageNext = (stageNext + 1) % kStages;
    if (st.used) HIPCHECK(hipEventSynchronize(st.ev));
    if (st.cap < bytes) {
      if (st.p) HIPCHECK(hipHostFree(st.p));
      st.p = nullptr;
      st.cap = std::max<size_t>(bytes, (size_t)1 << 16);
      HIPCHECK(hipHostMalloc(&st.p, st.cap, hipHostMallocDefault));
    }
    if (!st.ev) HIPCHECK(hipEventCreateWithFlags(&st.ev, hipEventDisableTiming));
    std::memcpy(st.p, src, bytes);
    HIPCHECK(hipMemcpyAsync(dst, st.p, bytes, hipMemcpyHostToDevice, stream));
    HIPCHECK(hipEventRecord(st.ev, stream));
    st.used = true;
    return GS_OK;
  }

  // Gives back the stream and everything allocated on or for the device and
  // forgets the device state: the destructor, and a start() that failed part
  // way (the next one then begins clean).
  void release() {
    if (stream) (void)hipStreamSynchronize(stream);  // staged uploads in flight
    auto dropStage = [](Stage& st) {
      if (st.ev) (void)hipEventDestroy(st.ev);
      if (st.p) (void)hipHostFree(st.p);
      st = Stage{};
    };
    dropStage(bigStage);
    for (Stage& st : stages) dropStage(st);
    for (hipEvent_t ev : evPool) (void)hipEventDestroy(ev);
    evPool.clear();
    pendKid.clear();
    evUsed = 0;
    [](auto&... b) { (b.free(), ...); }(evBuf, pairsBuf, retireBuf, acctBuf, msgSrc, msgTopic, msgSlot, msgId, msgKind,
                                        xSend, xRecv, xSendE, xRecvE, xSendP, ibx[0], ibx[1]);
    if (xHost) (void)hipHostFree(xHost);
    if (errRing) (void)hipHostFree(errRing);
    xHost = nullptr;
    errRing = nullptr;
    for (void* p : allocs) (void)hipFree(p);
    allocs.clear();
    if (stream) (void)hipStreamDestroy(stream);
    stream = nullptr;
    d = Dev{};
    dDev = nullptr;
    dLatM = nullptr;
    dLatH = nullptr;
    dInspRows = nullptr;
    dInspBounds = dInspScore = dInspExt = nullptr;
    dInspEdges = nullptr;
    inspEdges.clear();
    inspTaken = 0;
    dMeshMask = nullptr;
    dMeshL = dMeshZ = dMeshFlag = nullptr;
    dMeshRows = dMeshWords = nullptr;
    meshTaken = 0;
    dReachSrc = nullptr;
    dReachMask = dReachDepths = nullptr;
    dReachR[0] = dReachR[1] = nullptr;
    dReachMembers = dReachFlag = nullptr;
    dReachRows = dReachWords = nullptr;
    reachTaken = 0;
    dBwBounds = nullptr;
    dBwNodes = nullptr;
    dBwPrev = dBwDelta = dBwRows = dBwBytes = dBwRpcs = nullptr;
    bwTaken = 0;
    started = churnOn = allocFailed = false;
    uploaded = 0;
    aliveH.clear();
    tracePending.clear();  // the time-0 events start() recorded
  }
  ~gs_engine() { release(); }
  bool ageWindowNeeded() const {
    for (int t = 0; t < T; ++t)
      if (tscored[t] && tps[t].MeshMessageDeliveriesWindow < retireOf(t) * cfg.hop_ns) return true;
    return false;
  }
  bool heartbeatDue(int64_t t) const {
    if (cfg.router != GS_ROUTER_GOSSIPSUB) return false;
    if (t < gp.HeartbeatInitialDelay) return false;
    return (t - gp.HeartbeatInitialDelay) % gp.HeartbeatInterval == 0;
  }
  bool refreshDue(int64_t t) const { return scoring && t > 0 && t % sp.DecayInterval == 0; }
  // Message-window policy: a message must be first delivered within maxAge
  // hops of its publish (phase A tracks first deliverers for those "young"
  // slots only), and its slot is recycled only after retireHops.  (A topic
  // may have an age limit of its own, gs_window.h: ageOf / retireOf.)  Honest
  // runs deliver everything within a few hops (3 heartbeats is ample); with
  // the adversarial model (validation drops, the gater, spam) messages can
  // arrive much later through gossip, so the window then spans the gossip
  // history twice over.
  void setWindow() {
    // (churn too: a peer that joins or reconnects late catches up through gossip)
    const bool adv = advModel() || churnWindow;
    maxAge = (adv ? gp.HistoryLength + gp.HistoryGossip + 3 : 3) * H;
    retireHops = maxAge + (int64_t)(gp.HistoryLength + 2) * H;
    if (cfg.router != GS_ROUTER_GOSSIPSUB) retireHops = maxAge + 2;
    ageMax = 0;  // (userAge: [T] from creation on)
    for (int t = 0; t < T; ++t) ageMax = std::max(ageMax, ageOf(t));
  }

  // start(): what the host works out before the device is touched (every
  // refusal is made there), then the device state in stages
  struct Plan {
    bool anyRandom = false;          // some host runs randomsub (d.sel)
    int maxdeg = 0;
    std::vector<uint8_t> downH;      // [E] connections down at the start (empty: none)
    std::vector<double> p6;          // [E] P6 colocation factors
    std::vector<int32_t> pmaskRowH;  // [N] drec.peers rows of the owned IWANT spammers
    int nSpam = 0;
    int64_t nSpamEdges = 0;          // owned edges whose peer is an IWANT spammer
    bool isDown(int64_t e) const { return !downH.empty() && downH[e]; }
  };
  int start(), chooseModes(Plan& pl), hostGraph(Plan& pl), planCapacities(Plan& pl), buildDevice(const Plan& pl);
  void setDevScalars(const Plan& pl);
  int allocGraph(const Plan& pl), allocNodeState(), allocFrontiers(), allocNodeTables(const Plan& pl);
  int allocEdgeState(), allocIwantPool(), allocAdversary(const Plan& pl), allocGater(const Plan& pl);
  int allocReadback(), allocTrace(), allocPartition(), initConnections(const Plan& pl), allocAcct(const Plan& pl);

  // stepOne(): one hop as stages, in launch order
  struct Hop {
    int64_t h, now;
    int cur;
    size_t b = 0, e = 0;     // this hop's local publishes [b, e)
    int n = 0;
    // active word windows: amW = words of messages published in [h - maxAge, h]
    // (what this hop's frontier may hold), amR = the previous hop's (what the
    // senders' frontiers hold), amP = words of the slots published this hop
    // (phase A clears their old seen bits)
    WMask amR{}, amW{}, amP{};
    int nY = 0;              // phase A's young slots (the messages of amR)
    std::vector<int32_t> retireWords;
  };
  int stepOne(), hopWindow(Hop& hp), fanoutPublish(const Hop& hp), phaseA(const Hop& hp);
  int retireAndPublish(const Hop& hp), phaseB(const Hop& hp);
  int allocLatency(), latencyStats(const Hop& hp);
  int allocInspect(), inspectTick();
  int allocMeshHealth(), meshTick();
  int allocMeshReach(), reachTick();
  int allocBandwidth(), bandwidthTick();
  void refreshOrFold(const Hop& hp), heartbeat(const Hop& hp);
  template <bool ADV>
  PhaseADev<ADV> phaseADev() const {
    if constexpr (ADV) return dDev;
    else return d;
  }
  int uploadMessages();
  int checkDeviceError();
  // Device error flags, copied to pinned memory after every hop so the first
  // failing hop is named; an error is sticky (the state after it is not the
  // reference's), every later gs_step returns it again.
  static constexpr int kErrRing = 64;
  int32_t* errRing = nullptr;
  int stickyRc = GS_OK;
  std::string stickyMsg;
  int drainErrors(int64_t firstHop, int n);
  int deviceErrorCode(int32_t err);
  int deviceErrorText(int32_t err, int64_t atHop);
};
