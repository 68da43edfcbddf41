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

// The schedule of a periodic inspector (DESIGN.md §6n "The ticker"): every
// `period` hops a tick goes into a ring of `cap` slots, tick k (k = 0, 1, ...)
// when the hop counter becomes hopOf(k).  A read of tick k is valid while
// taken - cap <= k < taken.  `what` prefixes the messages, `title` names the
// option in the set-up refusals, `off` is said while it is not on.
struct gs_engine;
struct Ticker {
  const char *what, *title, *off;
  bool oneRank;  // not on a partitioned engine
  bool on = false;
  int64_t period = 0, taken = 0;
  int cap = 0;
  bool due(int64_t hop) const { return on && hop % period == 0; }
  size_t slot() const { return (size_t)(taken % cap); }  // of the tick being taken
  size_t slotOf(int64_t tick) const { return (size_t)(tick % cap); }
  int64_t hopOf(int64_t tick) const { return (tick + 1) * period; }
  int on_check() const {
    if (on) return GS_OK;
    gs_set_error(off);
    return GS_ESTATE;
  }
  int64_t ticksTaken() const {  // (a negative GS_* code while off)
    GS_TRY(on_check());
    return taken;
  }
  int tickOk(int64_t tick) const {
    GS_TRY(on_check());
    if (tick < 0 || tick >= taken) {
      gs_set_error(std::string(what) + ": tick " + std::to_string(tick) + " not taken yet (" + std::to_string(taken) +
                   " so far)");
      return GS_EINVAL;
    }
    if (tick < taken - cap) {
      gs_set_error(std::string(what) + ": tick " + std::to_string(tick) + " already overwritten (ring of " +
                   std::to_string(cap) + ")");
      return GS_ESTATE;
    }
    return GS_OK;
  }
  // The refusals every gs_set_* of an inspector begins with, in their order;
  // `c` is its config record (null: refused as a bad period).  Sets nothing:
  // the caller arms the ticker once its own checks have passed too.
  enum Needs : unsigned { kGossipsub = 1, kScoring = 2, kAccounting = 4 };
  template <class Config>
  int configure(const gs_engine* g, const Config* c, unsigned needs) const;
  template <class Config>
  void arm(const Config* c) {
    period = c->period_hops;
    cap = c->ticks;
    on = true;
  }
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
  // A stage with a failure group of its own: a failure among the allocations
  // `body` makes is reported here, under the group's name; an earlier stage's
  // pending failure stays pending for that stage's allocFail.
  template <class Body>
  int allocGroup(const char* group, const char* hint, Body&& body) {
    const bool before = allocFailed;
    allocFailed = false;
    body();
    if (allocFailed) return allocFail(group, hint);
    allocFailed = before;
    return GS_OK;
  }
  unsigned cus = 1;  // the device's compute units (buildDevice): the capped grids are multiples of it
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
  // The observers below: each keeps what the caller configured, which outlives
  // release(), apart from its `dev`: what start() allocates and derives, which
  // release() forgets by assigning a fresh one.
  //
  // latency statistics (gs_latency.h): the per-message and per-topic tables
  // ([S][bins] and [T][bins], bins = the largest age limit + 1; Dev::latCnt holds a hop's
  // counts) and the grid of k_lat_count
  struct {
    bool on = false;
    struct {
      uint32_t* perMsg = nullptr;
      unsigned long long* hist = nullptr;
      unsigned grid = 0;
    } dev;
  } lat;
  int latBins() const { return ageMax + 1; }
  // WithPeerScoreInspect (gs_inspect.h): a ring of ticks, each a row
  // (insp_row_len: score_hist, then mesh_deg), the sampled edges' scores and,
  // extended, their snapshot fields (k_inspect_gather's layout)
  struct {
    Ticker tk{"score inspection", "peer score inspector", "score inspection is off (gs_set_score_inspect)", false};
    bool ext = false;
    std::vector<double> bounds;
    std::vector<uint8_t> mask;     // [N] observers, or empty
    struct {
      std::vector<int64_t> edges;  // the sampled edges of this rank, ascending
      unsigned long long* rows = nullptr;
      double *bounds = nullptr, *score = nullptr, *ext = nullptr;
      int64_t* edgeList = nullptr;
      unsigned grid = 0;
    } dev;
  } insp;
  int inspRowLen() const { return insp_row_len((int)insp.bounds.size(), T); }
  size_t inspExtLen() const { return insp.dev.edges.size() * (3 + 4 * (size_t)T); }  // 8-byte words per tick
  // mesh health (gs_mesh_health.h): the label and size tables (uint32 [N][T]),
  // a ring of rows (mesh_row_len), the batch's flags and the word count
  struct {
    Ticker tk{"mesh health", "mesh health inspector", "mesh health is off (gs_set_mesh_health)", true};
    bool labels = false;
    std::vector<uint8_t> mask;     // [N] the hosts counted, or empty for all
    int64_t iters = 0, bytes = 0;  // since the start or the last gs_set_profiling
    struct {
      uint8_t* mask = nullptr;
      uint32_t *L = nullptr, *Z = nullptr, *flag = nullptr;  // flags: [GS_MESH_BATCH + 1]
      unsigned long long *rows = nullptr, *words = nullptr;
      unsigned grid = 0;
    } dev;
  } mesh;
  // mesh reach (gs_mesh_reach.h): the two bit tables (uint64 [N][T]), a ring of
  // rows (reach_row_len), the members per topic, the batch's flags, the byte
  // counters and, when asked for, the depth table (uint8 [K][N][T])
  struct {
    Ticker tk{"mesh reach", "mesh reach inspector", "mesh reach is off (gs_set_mesh_reach)", true};
    bool depths = false;
    std::vector<int32_t> src;      // [K] the sources
    std::vector<uint8_t> mask;     // [N] the hosts that can be targets, or empty for all
    int64_t passes = 0, levels = 0, bytes = 0;  // since the start or the last gs_set_profiling
    struct {
      int32_t* src = nullptr;
      uint8_t *mask = nullptr, *depths = nullptr;
      uint64_t* R[2] = {nullptr, nullptr};
      uint32_t *members = nullptr, *flag = nullptr;  // flags: [GS_REACH_BATCH + 1]
      unsigned long long *rows = nullptr, *words = nullptr;
      unsigned grid = 0;
    } dev;
  } reach;
  // bandwidth statistics (gs_bandwidth.h): the per-node tables (uint64 [N][8]:
  // the cumulative sums at the previous tick, this tick's deltas), a ring of
  // rows (bw_row_len) and the sampled nodes' values (k_bw_gather's layout)
  struct {
    Ticker tk{"bandwidth statistics", "bandwidth statistics",
              "the bandwidth statistics are off (gs_set_bandwidth_stats)", true};
    std::vector<int64_t> bounds;
    std::vector<int32_t> nodes;    // the sampled nodes, ascending
    struct {
      long long* bounds = nullptr;
      int32_t* nodes = nullptr;
      unsigned long long *prev = nullptr, *delta = nullptr, *rows = nullptr, *bytes = nullptr, *rpcs = nullptr;
      unsigned grid = 0;
    } dev;
  } bw;
  int bwRowLen() const { return bw_row_len((int)bw.bounds.size()); }
  // The tickers in the order their ticks run at the end of a hop (DESIGN.md
  // §6p: mesh reach after the other two inspectors).
  struct Tick {
    Ticker* tk;
    int (gs_engine::*take)();
  };
  const Tick tickers[4] = {{&insp.tk, &gs_engine::inspectTick},
                           {&mesh.tk, &gs_engine::meshTick},
                           {&reach.tk, &gs_engine::reachTick},
                           {&bw.tk, &gs_engine::bandwidthTick}};
  // kernel timing: (kernel id, start event, end event) pending until a sync
  bool profiling = false;
  std::vector<hipEvent_t> evPool;
  size_t evUsed = 0;
  std::vector<int> pendKid;
  // Past the public kernel ids, each feature's range follows the one before it:
  // the latency kernels (gs_read_latency_kernel_stats), the inspection's three
  // passes (gs_read_inspect_kernel_stats), then kMeshInit + GS_MESH_K_*,
  // kReachMembers + GS_REACH_K_* and kBwTick + GS_BW_K_* (their gs_read_*_kernel_stats)
  enum : int { kLatCount = GS_NUM_KERNELS, kLatFold, kLatEnd };
  enum : int { kInspScore = kLatEnd, kInspReduce, kInspGather, kInspEnd };
  static constexpr int kMeshInit = kInspEnd;
  static constexpr int kReachMembers = kMeshInit + GS_MESH_ST_ITERS;
  static constexpr int kBwTick = kReachMembers + GS_REACH_ST_PASSES;
  static constexpr int kTimed = kBwTick + GS_BW_NUM_STATS;
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
    lat.dev = {};
    insp.dev = {};
    mesh.dev = {};
    reach.dev = {};
    bw.dev = {};
    for (const Tick& t : tickers) t.tk->taken = 0;
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
  // A fixed point bounded on the host (DESIGN.md §6n "The fixed-point driver"):
  // iterations go out in batches of `batch`, launch(i, ran) issuing the batch's
  // iteration i against dFlag + i (`ran`: the iterations that ran before this
  // batch).  An iteration runs if its flag is set and sets the next one if it
  // changed anything; the batch's first flag is set here.  After a batch the
  // host reads the flags: flag[i] != 0 counts iteration i as run, the flag
  // past the batch's last clear ends the loop.  More than `limit` iterations
  // fail with failText, *ran, failUnit and the hop.
  template <class Launch>
  int runBatched(int batch, uint32_t* dFlag, int64_t limit, const char* failText, const char* failUnit,
                 Launch&& launch, int64_t* ran) {
    std::vector<uint32_t> flag((size_t)batch + 1);
    *ran = 0;
    for (bool ended = false; !ended;) {
      const int n = (int)std::min<int64_t>(batch, limit - *ran);
      if (n <= 0) {
        gs_set_error(failText + std::to_string(*ran) + failUnit + " (hop " + std::to_string(hop) + ")");
        return GS_EDEVICE;
      }
      HIPCHECK(hipMemsetAsync(dFlag, 0, flag.size() * 4, stream));
      HIPCHECK(hipMemsetAsync(dFlag, 1, 4, stream));  // non-zero: the batch's first iteration runs
      for (int i = 0; i < n; ++i) launch(i, *ran);
      HIPCHECK(hipMemcpyAsync(flag.data(), dFlag, flag.size() * 4, hipMemcpyDeviceToHost, stream));
      HIPCHECK(hipStreamSynchronize(stream));
      for (int i = 0; i < n; ++i) *ran += flag[i] != 0u;
      ended = flag[n] == 0u;
    }
    return GS_OK;
  }
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

template <class Config>
int Ticker::configure(const gs_engine* g, const Config* c, unsigned needs) const {
  const auto refuse = [](const std::string& text, int code) {
    gs_set_error(text);
    return code;
  };
  const std::string w = what, t = title;
  if (g->started) return refuse("the " + t + " must be set before the first step", GS_ESTATE);
  if (on) return refuse("duplicate " + t, GS_ESTATE);
  if ((needs & kGossipsub) && g->cfg.router != GS_ROUTER_GOSSIPSUB)
    return refuse("pubsub router is not gossipsub", GS_EUNSUPPORTED);
  if ((needs & kScoring) && !g->scoring) return refuse("peer scoring is not enabled", GS_EUNSUPPORTED);
  if ((needs & kAccounting) && !g->acctOn) return refuse(w + ": RPC accounting is off", GS_ESTATE);
  if (oneRank && g->world > 1) return refuse(w + ": not on a partitioned engine", GS_EUNSUPPORTED);
  if (!c || c->period_hops <= 0) return refuse(w + ": period_hops must be positive", GS_EINVAL);
  if (c->ticks < 1) return refuse(w + ": ticks must be at least 1", GS_EINVAL);
  return GS_OK;
}
