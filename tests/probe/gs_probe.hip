// gs_probe.hip — test-only probe of the device primitives the kernels are made
// of (tests/probe.py loads it; the product never does).  One small __global__
// wrapper per primitive family calls the helpers of csrc/gs_device.h,
// gs_kernels.h and gs_kernels_ctl.h exactly as the kernels do, and extern "C"
// entry points take host pointers, do their own hipMalloc / copies /
// hipDeviceSynchronize and return the HIP error code (0 = ok).
//
// Every wrapper launches blocks of exactly 64 threads (one wave: select_kth
// and select_kth_est use __syncthreads and are wave-uniform calls), one case
// per block, all cases of a test in one launch.  Every loop is bounded by the
// wrapper's inputs.  Two entry points launch kernels of the product itself,
// in the engine's geometry: gsp_ptx_rebuild (the heartbeat's peertx rebuild,
// through the engine's own ptx_rebuild_launch) and gsp_spam (k_retire).
#include "../../go-libp2p-pubsub_amd/csrc/gs_device.h"
#include "../../go-libp2p-pubsub_amd/csrc/gs_kernels.h"
#include "../../go-libp2p-pubsub_amd/csrc/gs_kernels_ctl.h"

#include <cstring>
#include <vector>

namespace {

// device copies of host arrays, freed on scope exit; the first HIP error sticks
struct Bufs {
  std::vector<void*> ptrs;
  hipError_t err = hipSuccess;
  ~Bufs() {
    for (void* p : ptrs) (void)hipFree(p);
  }
  bool ok() const { return err == hipSuccess; }
  void note(hipError_t e) {
    if (err == hipSuccess && e != hipSuccess) err = e;
  }
  // n elements, copied from src when src != nullptr, else zeroed
  template <class T>
  T* dev(const T* src, size_t n) {
    if (!ok()) return nullptr;
    void* p = nullptr;
    const size_t bytes = (n ? n : 1) * sizeof(T);
    note(hipMalloc(&p, bytes));
    if (!ok()) return nullptr;
    ptrs.push_back(p);
    if (src != nullptr && n) note(hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice));
    else note(hipMemset(p, 0, bytes));
    return (T*)p;
  }
  template <class T>
  void back(T* dst, const T* src, size_t n) {
    if (ok() && n) note(hipMemcpy(dst, src, n * sizeof(T), hipMemcpyDeviceToHost));
  }
  void sync() {
    if (!ok()) return;
    note(hipGetLastError());
    note(hipDeviceSynchronize());
  }
};

// ---- select_k, select_k_half, grp_select ---------------------------------
// mode 0 select_k, 1 select_k_half, 2 grp_select<false>, 3 grp_select<true>,
// 4 select_k_half called inside `if (lane < 32)`, 5 inside `if (lane >= 32)`.
// out[case] = ballot of the returned flag (lanes that made no call: 0).
__global__ __launch_bounds__(64) void kp_select_k(int mode, const uint8_t* cand, const uint64_t* key, const int32_t* k,
                                                  uint64_t* out) {
  const int lane = lane_id();
  const int64_t i = (int64_t)blockIdx.x * 64 + lane;
  const bool c = cand[i] != 0;
  const uint64_t ky = key[i];
  const int kk = k[i];
  bool r = false;
  switch (mode) {
    case 0: r = select_k(c, ky, kk); break;
    case 1: r = select_k_half(c, ky, kk); break;
    case 2: r = grp_select<false>(c, ky, kk); break;
    case 3: r = grp_select<true>(c, ky, kk); break;
    case 4:
      if (lane < 32) r = select_k_half(c, ky, kk);
      break;
    default:
      if (lane >= 32) r = select_k_half(c, ky, kk);
      break;
  }
  const unsigned long long m = __ballot(r);
  if (lane == 0) out[blockIdx.x] = m;
}

// ---- select_kth, select_kth_est ------------------------------------------
// Case c owns candidates [off[c], off[c + 1]) of keys / ids; lane l's share is
// the sub-range [laneOff[65 c + l], laneOff[65 c + l + 1]) of it (unequal
// shares, empty ones included), re-run on every call of each() as at the real
// call sites.  est != 0: select_kth_est with n = nArg[c].
__global__ __launch_bounds__(64) void kp_select_kth(int est, const int64_t* off, const int32_t* laneOff,
                                                    const unsigned long long* keys, const long long* ids,
                                                    const int32_t* k, const int32_t* nArg, unsigned long long* Kout,
                                                    long long* Mout) {
  __shared__ uint32_t hist[256];
  __shared__ unsigned long long cand[2 * GS_SEL_CAP + 1];
  const int lane = lane_id();
  const int c = blockIdx.x;
  const int64_t base = off[c];
  const int a = laneOff[65 * c + lane], b = laneOff[65 * c + lane + 1];
  auto each = [&](auto&& fn) {
    for (int j = a; j < b; ++j) fn(keys[base + j], ids[base + j]);
  };
  unsigned long long K = 0;
  long long M = 0;
  if (est) select_kth_est(each, k[c], nArg[c], hist, cand, K, M);
  else select_kth(each, k[c], hist, K, M);
  if (lane == 0) {
    Kout[c] = K;
    Mout[c] = M;
  }
}

// ---- the lane primitives -------------------------------------------------
enum {
  OP_INCL_SUM = 0, OP_LANE_PREFIX, OP_WAVE_LAST, OP_SUM_INT, OP_SUM_LL, OP_LANE_RANK, OP_XOR32_U32, OP_XOR32_U64,
  OP_XOR32_F64, OP_LANE_GET64, OP_LANE_GETF, OP_TRANSPOSE, OP_TRANSPOSE2, OP_KTH_BIT, OP_COUNT
};
// a[64 case + lane] is the lane's operand (an int as its low 32 bits, a double
// as its bit pattern), b the second one (source lane, k: the source lane is
// the case's lane-0 value, wave-uniform as at the call sites); o1 / o2 results.
__global__ __launch_bounds__(64) void kp_lanes(int op, const uint64_t* a, const int32_t* b, uint64_t* o1, uint64_t* o2) {
  const int lane = lane_id();
  const int64_t i = (int64_t)blockIdx.x * 64 + lane;
  const uint64_t x = a[i];
  const int xi = (int)(uint32_t)x;
  const int src = __builtin_amdgcn_readfirstlane(b[(int64_t)blockIdx.x * 64]) & 63;
  uint64_t r1 = 0, r2 = 0;
  switch (op) {
    case OP_INCL_SUM: r1 = (uint32_t)wave_incl_sum(xi); break;
    case OP_LANE_PREFIX: {
      int total = 0;
      r1 = (uint32_t)lane_prefix(xi, &total);
      r2 = (uint32_t)total;
      break;
    }
    case OP_WAVE_LAST: r1 = (uint32_t)wave_last(xi); break;
    case OP_SUM_INT: r1 = (uint32_t)wave_sum_int(xi); break;
    case OP_SUM_LL: r1 = wave_sum_ll((long long)x); break;
    case OP_LANE_RANK: r1 = (uint32_t)lane_rank(x); break;
    case OP_XOR32_U32: r1 = xor32_u32((uint32_t)x); break;
    case OP_XOR32_U64: r1 = xor32_u64(x); break;
    case OP_XOR32_F64: r1 = (uint64_t)__double_as_longlong(xor32_f64(__longlong_as_double((long long)x))); break;
    case OP_LANE_GET64: r1 = lane_get64(x, src); break;
    case OP_LANE_GETF: r1 = (uint64_t)__double_as_longlong(lane_getf(__longlong_as_double((long long)x), src)); break;
    case OP_TRANSPOSE: r1 = wave_transpose64(x); break;
    case OP_TRANSPOSE2: r1 = wave_transpose64(wave_transpose64(x)); break;
    case OP_KTH_BIT: r1 = (uint32_t)kth_bit(x, b[i]); break;
    default: break;
  }
  o1[i] = r1;
  o2[i] = r2;
}

// item_sender over the case's 64-entry exclusive prefix table (in LDS, as at
// the call sites), for every item index b < nItems[case]
__global__ __launch_bounds__(64) void kp_item_sender(const int32_t* sIt, const int32_t* nItems, int maxItems,
                                                     int32_t* sender, int32_t* within) {
  __shared__ int sTab[64];
  const int lane = lane_id();
  sTab[lane] = sIt[(int64_t)blockIdx.x * 64 + lane];
  __syncthreads();
  const int n = min(nItems[blockIdx.x], maxItems);
  for (int b = lane; b < n; b += 64) {
    int k = -1;
    const int i = item_sender(sTab, b, k);
    sender[(int64_t)blockIdx.x * maxItems + b] = i;
    within[(int64_t)blockIdx.x * maxItems + b] = k;
  }
}

// dlt_put then dlt_get of pair i in the layout the Dev selects
__global__ __launch_bounds__(64) void kp_dlt(Dev d, int n, const uint32_t* q, uint32_t* got) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  dlt_put(d, i, q[i]);
  got[i] = dlt_get(d, i);
}

// ---- the headers shared with the host, compiled for the device ------------
__global__ __launch_bounds__(64) void kp_philox(int n, const uint32_t* ctr, const uint32_t* key, uint32_t* out) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t c[4] = {ctr[4 * i], ctr[4 * i + 1], ctr[4 * i + 2], ctr[4 * i + 3]};
  uint32_t k[2] = {key[2 * i], key[2 * i + 1]};
  uint32_t o[4];
  gs_philox4x32_10(c, k, o);
  for (int j = 0; j < 4; ++j) out[4 * i + j] = o[j];
}
// args[6 i ..] = seed, site, a, b, c, d
__global__ __launch_bounds__(64) void kp_keys(int n, const uint32_t* args, uint64_t* k64, uint64_t* kmid, uint64_t* kx2,
                                              uint64_t* unit) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const uint32_t* g = args + 6 * i;
  const uint64_t k = gs_key64(g[0], g[1], g[2], g[3], g[4], g[5]);
  k64[i] = k;
  kmid[i] = gs_key64_mid(g[0], g[1], g[2], g[3], g[4], g[5]);
  uint64_t two[2];
  gs_key64x2(g[0], g[1], g[2], g[3], g[4], g[5], two);
  kx2[2 * i] = two[0];
  kx2[2 * i + 1] = two[1];
  unit[i] = (uint64_t)__double_as_longlong(gs_key_to_unit(k));
}
__global__ __launch_bounds__(64) void kp_quantum_div(int n, const int64_t* mt, const int64_t* q, const uint64_t* magic,
                                                     int64_t* out) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  out[i] = gs_quantum_div(mt[i], q[i], magic[i]);
}
__global__ __launch_bounds__(64) void kp_add_ones(int n, const double* x, const int64_t* steps, const double* cap,
                                                  double* plain, double* capped) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  plain[i] = gs_add_ones(x[i], steps[i]);
  capped[i] = gs_add_ones_capped(x[i], steps[i], cap[i]);
}

// ---- the peertx hash tables ----------------------------------------------
__global__ __launch_bounds__(64) void kp_ptx_hash(int n, const uint32_t* keys, int hbits, int32_t* out) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i < n) out[i] = ptx_hash(keys[i], hbits);
}
// one round of increments: thread i does ++count of key[i] in node node[i]'s
// table the way handleIWant's pass does (first CAS at the home slot, then
// ptx_settle); node < 0: no request.  The caller keeps the keys of one node
// distinct within a round (no two increments of one key race).
__global__ __launch_bounds__(64) void kp_ptx_round(Dev d, int n, const int32_t* node, const uint32_t* key, int32_t* ret,
                                                   uint8_t* insOut) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n || node[i] < 0) return;
  const int v = node[i];
  uint32_t* prow = ptx_row(d, v);
  const int hs = ptx_hash(key[i], d.ptxBits);
  const uint32_t pv = atomicCAS(&prow[hs], 0u, key[i] | 1u);
  bool ins = false;
  ret[i] = ptx_settle(d, v, prow, key[i], hs, pv, ins);
  insOut[i] = ins ? 1 : 0;
}
__global__ __launch_bounds__(64) void kp_ptx_count(Dev d, int n, const int32_t* node, const uint32_t* key, int32_t* cntG,
                                                   int32_t* cntO) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n || node[i] < 0) return;
  cntG[i] = ptx_count_g(d, node[i], ptx_row(d, node[i]), key[i]);
  cntO[i] = ptxo_count(d, node[i], key[i]);
}

// ---- the spammers' nibble counters ---------------------------------------
// one round: thread i does spam_incr(row[i], slot[i]); row < 0: no request.
// The caller keeps (row, slot) distinct within a round, as the call sites do.
__global__ __launch_bounds__(64) void kp_spam_round(Dev d, int n, const int32_t* row, const int32_t* slot, int32_t* ret) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n || row[i] < 0) return;
  ret[i] = spam_incr(d, row[i], slot[i]);
}

// ---- pool_take -----------------------------------------------------------
// lane 0 of block b asks for n[b] ids, as the kernels' one lane per wave does;
// n[b] == 0: the block asks for nothing (no call site ever asks for 0 ids)
__global__ __launch_bounds__(64) void kp_pool_take(Dev d, int cur, const unsigned long long* n, unsigned long long* out) {
  if (threadIdx.x == 0 && n[blockIdx.x] != 0ull) out[blockIdx.x] = pool_take(d, cur, n[blockIdx.x]);
}

inline int blocks_of(int64_t n) { return (int)((n + 63) / 64); }

}  // namespace

extern "C" {

// the constants the references need: out[0] = GS_SEL_WIN, [1] = GS_SEL_CAP,
// [2] = E_PEERTX, [3] = number of gsp_lanes ops, [4] = E_POOL
int gsp_consts(int32_t* out) {
  out[0] = GS_SEL_WIN;
  out[1] = GS_SEL_CAP;
  out[2] = E_PEERTX;
  out[3] = OP_COUNT;
  out[4] = E_POOL;
  return 0;
}

int gsp_select_k(int mode, int ncase, const uint8_t* cand, const uint64_t* key, const int32_t* k, uint64_t* out) {
  if (ncase <= 0) return 0;
  Bufs B;
  const size_t n = (size_t)ncase * 64;
  auto* dc = B.dev(cand, n);
  auto* dk = B.dev(key, n);
  auto* dn = B.dev(k, n);
  auto* dout = B.dev<uint64_t>(nullptr, ncase);
  if (B.ok()) hipLaunchKernelGGL(kp_select_k, dim3(ncase), dim3(64), 0, 0, mode, dc, dk, dn, dout);
  B.sync();
  B.back(out, dout, ncase);
  return (int)B.err;
}

int gsp_select_kth(int est, int ncase, const int64_t* off, const int32_t* laneOff, const uint64_t* keys,
                   const int64_t* ids, const int32_t* k, const int32_t* nArg, uint64_t* K, int64_t* M) {
  if (ncase <= 0) return 0;
  for (int c = 0; c < ncase; ++c) {  // every lane's share lies inside its case
    const int64_t n = off[c + 1] - off[c];
    if (off[c] < 0 || n < 0 || laneOff[65 * c] < 0 || laneOff[65 * c + 64] > n) return (int)hipErrorInvalidValue;
    for (int l = 0; l < 64; ++l)
      if (laneOff[65 * c + l] > laneOff[65 * c + l + 1]) return (int)hipErrorInvalidValue;
  }
  Bufs B;
  const size_t total = (size_t)off[ncase];
  auto* doff = B.dev(off, (size_t)ncase + 1);
  auto* dlo = B.dev(laneOff, (size_t)ncase * 65);
  auto* dkeys = B.dev((const unsigned long long*)keys, total);
  auto* dids = B.dev((const long long*)ids, total);
  auto* dk = B.dev(k, ncase);
  auto* dn = B.dev(nArg, ncase);
  auto* dK = B.dev<unsigned long long>(nullptr, ncase);
  auto* dM = B.dev<long long>(nullptr, ncase);
  if (B.ok()) hipLaunchKernelGGL(kp_select_kth, dim3(ncase), dim3(64), 0, 0, est, doff, dlo, dkeys, dids, dk, dn, dK, dM);
  B.sync();
  B.back((unsigned long long*)K, dK, ncase);
  B.back((long long*)M, dM, ncase);
  return (int)B.err;
}

int gsp_lanes(int op, int ncase, const uint64_t* a, const int32_t* b, uint64_t* o1, uint64_t* o2) {
  if (ncase <= 0) return 0;
  if (op < 0 || op >= OP_COUNT) return (int)hipErrorInvalidValue;
  const size_t n = (size_t)ncase * 64;
  if (op == OP_KTH_BIT)  // kth_bit loops k times
    for (size_t i = 0; i < n; ++i)
      if (b[i] < 0 || b[i] > 64) return (int)hipErrorInvalidValue;
  Bufs B;
  auto* da = B.dev(a, n);
  auto* db = B.dev(b, n);
  auto* d1 = B.dev<uint64_t>(nullptr, n);
  auto* d2 = B.dev<uint64_t>(nullptr, n);
  if (B.ok()) hipLaunchKernelGGL(kp_lanes, dim3(ncase), dim3(64), 0, 0, op, da, db, d1, d2);
  B.sync();
  B.back(o1, d1, n);
  B.back(o2, d2, n);
  return (int)B.err;
}

int gsp_item_sender(int ncase, const int32_t* sIt, const int32_t* nItems, int maxItems, int32_t* sender,
                    int32_t* within) {
  if (ncase <= 0 || maxItems <= 0) return 0;
  Bufs B;
  const size_t nOut = (size_t)ncase * maxItems;
  auto* ds = B.dev(sIt, (size_t)ncase * 64);
  auto* dn = B.dev(nItems, ncase);
  auto* d1 = B.dev<int32_t>(nullptr, nOut);
  auto* d2 = B.dev<int32_t>(nullptr, nOut);
  if (B.ok()) hipLaunchKernelGGL(kp_item_sender, dim3(ncase), dim3(64), 0, 0, ds, dn, maxItems, d1, d2);
  B.sync();
  B.back(sender, d1, nOut);
  B.back(within, d2, nOut);
  return (int)B.err;
}

int gsp_dlt(int narrow, int n, const uint32_t* q, uint32_t* got) {
  if (n <= 0) return 0;
  Bufs B;
  Dev d;
  std::memset(&d, 0, sizeof(d));
  if (narrow) d.dltN = B.dev<uint16_t>(nullptr, n);
  else d.dlt = B.dev<uint32_t>(nullptr, n);
  auto* dq = B.dev(q, n);
  auto* dg = B.dev<uint32_t>(nullptr, n);
  if (B.ok()) hipLaunchKernelGGL(kp_dlt, dim3(blocks_of(n)), dim3(64), 0, 0, d, n, dq, dg);
  B.sync();
  B.back(got, dg, n);
  return (int)B.err;
}

int gsp_philox(int n, const uint32_t* ctr, const uint32_t* key, uint32_t* out) {
  if (n <= 0) return 0;
  Bufs B;
  auto* dc = B.dev(ctr, (size_t)n * 4);
  auto* dk = B.dev(key, (size_t)n * 2);
  auto* dout = B.dev<uint32_t>(nullptr, (size_t)n * 4);
  if (B.ok()) hipLaunchKernelGGL(kp_philox, dim3(blocks_of(n)), dim3(64), 0, 0, n, dc, dk, dout);
  B.sync();
  B.back(out, dout, (size_t)n * 4);
  return (int)B.err;
}

int gsp_keys(int n, const uint32_t* args, uint64_t* k64, uint64_t* kmid, uint64_t* kx2, uint64_t* unit) {
  if (n <= 0) return 0;
  Bufs B;
  auto* da = B.dev(args, (size_t)n * 6);
  auto* d1 = B.dev<uint64_t>(nullptr, n);
  auto* d2 = B.dev<uint64_t>(nullptr, n);
  auto* d3 = B.dev<uint64_t>(nullptr, (size_t)n * 2);
  auto* d4 = B.dev<uint64_t>(nullptr, n);
  if (B.ok()) hipLaunchKernelGGL(kp_keys, dim3(blocks_of(n)), dim3(64), 0, 0, n, da, d1, d2, d3, d4);
  B.sync();
  B.back(k64, d1, n);
  B.back(kmid, d2, n);
  B.back(kx2, d3, (size_t)n * 2);
  B.back(unit, d4, n);
  return (int)B.err;
}

int gsp_quantum_div(int n, const int64_t* mt, const int64_t* q, const uint64_t* magic, int64_t* out) {
  if (n <= 0) return 0;
  Bufs B;
  auto* dm = B.dev(mt, n);
  auto* dq = B.dev(q, n);
  auto* dg = B.dev(magic, n);
  auto* dout = B.dev<int64_t>(nullptr, n);
  if (B.ok()) hipLaunchKernelGGL(kp_quantum_div, dim3(blocks_of(n)), dim3(64), 0, 0, n, dm, dq, dg, dout);
  B.sync();
  B.back(out, dout, n);
  return (int)B.err;
}

int gsp_add_ones(int n, const double* x, const int64_t* steps, const double* cap, double* plain, double* capped) {
  if (n <= 0) return 0;
  Bufs B;
  auto* dx = B.dev(x, n);
  auto* ds = B.dev(steps, n);
  auto* dc = B.dev(cap, n);
  auto* d1 = B.dev<double>(nullptr, n);
  auto* d2 = B.dev<double>(nullptr, n);
  if (B.ok()) hipLaunchKernelGGL(kp_add_ones, dim3(blocks_of(n)), dim3(64), 0, 0, n, dx, ds, dc, d1, d2);
  B.sync();
  B.back(plain, d1, n);
  B.back(capped, d2, n);
  return (int)B.err;
}

int gsp_ptx_hash(int n, const uint32_t* keys, int hbits, int32_t* out) {
  if (n <= 0) return 0;
  if (hbits < 1 || hbits > 31) return (int)hipErrorInvalidValue;
  Bufs B;
  auto* dk = B.dev(keys, n);
  auto* dout = B.dev<int32_t>(nullptr, n);
  if (B.ok()) hipLaunchKernelGGL(kp_ptx_hash, dim3(blocks_of(n)), dim3(64), 0, 0, n, dk, hbits, dout);
  B.sync();
  B.back(out, dout, n);
  return (int)B.err;
}

// nRounds rounds of perRound increments (one launch per round), then nQ
// lookups.  rows [nNodes << ptxBits], ovf [1 << ptxOBits], ocnt [3] and err [1]
// are in/out: the tables' state before, and after.  The Dev holds only the
// fields the peertx helpers read.
int gsp_peertx(int ptxBits, int ptxOBits, int GR, int nNodes, uint32_t* rows, uint64_t* ovf, uint32_t* ocnt,
               int32_t* err, int nRounds, int perRound, const int32_t* node, const uint32_t* key, int32_t* ret,
               uint8_t* ins, int nQ, const int32_t* qNode, const uint32_t* qKey, int32_t* cntG, int32_t* cntO) {
  if (ptxBits < 1 || ptxBits > 16 || ptxOBits < 1 || ptxOBits > 20 || nNodes < 1 || nRounds < 0 || perRound < 0 || nQ < 0)
    return (int)hipErrorInvalidValue;
  const size_t nOps = (size_t)nRounds * perRound;
  for (size_t i = 0; i < nOps; ++i)
    if (node[i] >= nNodes) return (int)hipErrorInvalidValue;
  for (int i = 0; i < nQ; ++i)
    if (qNode[i] >= nNodes) return (int)hipErrorInvalidValue;
  Bufs B;
  const size_t nRow = (size_t)nNodes << ptxBits, nOvf = (size_t)1 << ptxOBits;
  Dev d;
  std::memset(&d, 0, sizeof(d));
  d.ptxBits = ptxBits;
  d.ptxOBits = ptxOBits;
  d.GR = GR;
  d.ptxT = B.dev(rows, nRow);
  d.ptxO = (unsigned long long*)B.dev(ovf, nOvf);
  d.ptxOCnt = B.dev(ocnt, 3);
  d.err = B.dev(err, 1);
  auto* dnode = B.dev(node, nOps);
  auto* dkey = B.dev(key, nOps);
  auto* dret = B.dev<int32_t>(nullptr, nOps);
  auto* dins = B.dev<uint8_t>(nullptr, nOps);
  auto* dqn = B.dev(qNode, nQ);
  auto* dqk = B.dev(qKey, nQ);
  auto* dcg = B.dev<int32_t>(nullptr, nQ);
  auto* dco = B.dev<int32_t>(nullptr, nQ);
  for (int r = 0; r < nRounds && perRound > 0 && B.ok(); ++r) {
    const size_t o = (size_t)r * perRound;
    hipLaunchKernelGGL(kp_ptx_round, dim3(blocks_of(perRound)), dim3(64), 0, 0, d, perRound, dnode + o, dkey + o, dret + o,
                       dins + o);
    B.sync();  // the barrier between rounds
  }
  if (B.ok() && nQ > 0) hipLaunchKernelGGL(kp_ptx_count, dim3(blocks_of(nQ)), dim3(64), 0, 0, d, nQ, dqn, dqk, dcg, dco);
  B.sync();
  B.back(rows, d.ptxT, nRow);
  B.back((unsigned long long*)ovf, d.ptxO, nOvf);
  B.back(ocnt, d.ptxOCnt, 3);
  B.back(err, d.err, 1);
  B.back(ret, dret, nOps);
  B.back(ins, dins, nOps);
  B.back(cntG, dcg, nQ);
  B.back(cntO, dco, nQ);
  return (int)B.err;
}

// hipDeviceAttributeMaxSharedMemoryPerBlock of the current device: what bounds
// gs_set_peertx_capacity's home_bits (the rebuild's 4 << ptxBits bytes of LDS)
int gsp_lds_limit(int32_t* out) {
  int dev = 0, lim = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&lim, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
  out[0] = lim;
  return (int)e;
}

// The heartbeat's peertx rebuild, once: k_ptx_rebuild, k_ptxo_collect,
// k_ptxo_reinsert, k_ptxo_fin through ptx_rebuild_launch, the engine's own
// launch function, over nNodes owned nodes (n0 = 0, nOwnH = nNodes).  rows
// [nNodes << ptxBits], ptxN [nNodes], ovf [1 << ptxOBits] and ocnt [3] are
// in/out (the layout of gsp_peertx); hist is the mcache ring [R][nNodes][W]
// and `last` the ring row of the window leaving the cache.  Refused before any
// launch: a row that does not fit the device's LDS, an entry whose slot lies
// outside hist's W words or whose node tag is not a node, and counters that
// would let the staging index start above 0 (the stage holds 1 << ptxOBits).
int gsp_ptx_rebuild(int ptxBits, int ptxOBits, int nNodes, uint32_t* rows, int32_t* ptxN, uint64_t* ovf, uint32_t* ocnt,
                    int R, int W, int last, const uint64_t* hist) {
  if (ptxBits < 2 || ptxBits > 16 || ptxOBits < 1 || ptxOBits > 20 || nNodes < 1 || nNodes > (1 << 20) || R < 1 || W < 1 ||
      W > 256 || last < 0 || last >= R || ocnt[1] != 0u || ocnt[2] != 0u)
    return (int)hipErrorInvalidValue;
  int32_t lim = 0;
  if (const int e = gsp_lds_limit(&lim)) return e;
  if (ptx_rebuild_lds(ptxBits) > (size_t)lim) return (int)hipErrorInvalidValue;
  const size_t nRow = (size_t)nNodes << ptxBits, nOvf = (size_t)1 << ptxOBits;
  const uint32_t nSlots = (uint32_t)W * 64u;
  for (size_t i = 0; i < nRow; ++i)
    if (rows[i] != 0u && (rows[i] >> 14) >= nSlots) return (int)hipErrorInvalidValue;
  for (size_t i = 0; i < nOvf; ++i) {
    if (ovf[i] == 0ull) continue;
    const uint64_t tag = ovf[i] >> 32;
    if (tag < 1 || tag > (uint64_t)nNodes || ((uint32_t)ovf[i] >> 14) >= nSlots) return (int)hipErrorInvalidValue;
  }
  Bufs B;
  Dev d;
  std::memset(&d, 0, sizeof(d));
  d.ptxBits = ptxBits;
  d.ptxOBits = ptxOBits;
  d.n0 = 0;
  d.n1 = d.N = d.nOwnH = nNodes;
  d.W = W;
  d.R = R;
  d.ptxT = B.dev(rows, nRow);
  d.ptxN = B.dev(ptxN, nNodes);
  d.ptxO = (unsigned long long*)B.dev(ovf, nOvf);
  d.ptxOStage = B.dev<unsigned long long>(nullptr, nOvf);
  d.ptxOCnt = B.dev(ocnt, 3);
  d.hist = B.dev(hist, (size_t)R * nNodes * W);
  if (B.ok()) ptx_rebuild_launch(d, nNodes, last, 0);
  B.sync();
  B.back(rows, d.ptxT, nRow);
  B.back(ptxN, d.ptxN, nNodes);
  B.back((unsigned long long*)ovf, d.ptxO, nOvf);
  B.back(ocnt, d.ptxOCnt, 3);
  return (int)B.err;
}

// nRounds rounds of perRound spam_incr(row, slot) calls (one launch per round;
// row < 0: no request), then with doRetire one launch of k_retire alone, in
// the engine's geometry, over the CSR rowptr [nNodes + 1] / spamRow [edges]
// with pubmask[cur] = pubmask [S / 64] and the words[] list.  spamCnt
// [nRows][S / 8] and pmask [nPm][S] are in/out.  spamRow or pmaskRow
// [nNodes] == nullptr leaves that half of k_retire off, as in the engine.
int gsp_spam(int S, int GR, int nRows, uint32_t* spamCnt, int nRounds, int perRound, const int32_t* row,
             const int32_t* slot, int32_t* ret, int doRetire, int cur, int nNodes, const int64_t* rowptr,
             const int32_t* spamRow, const uint64_t* pubmask, int nwords, const int32_t* words, const int32_t* pmaskRow,
             int nPm, uint64_t* pmask) {
  if (S < 64 || S % 64 != 0 || S > (1 << 14) || GR < 0 || GR > 13 || nRows < 1 || nRounds < 0 || perRound < 0)
    return (int)hipErrorInvalidValue;
  const size_t nOps = (size_t)nRounds * perRound;
  for (size_t i = 0; i < nOps; ++i)
    if (row[i] >= nRows || (row[i] >= 0 && (slot[i] < 0 || slot[i] >= S))) return (int)hipErrorInvalidValue;
  int64_t nEdges = 0;
  if (doRetire) {
    if (cur < 0 || cur > 1 || nNodes < 1 || nwords < 1 || nPm < 0 || rowptr[0] != 0) return (int)hipErrorInvalidValue;
    for (int v = 0; v < nNodes; ++v)
      if (rowptr[v] > rowptr[v + 1]) return (int)hipErrorInvalidValue;
    nEdges = rowptr[nNodes];
    for (int64_t e = 0; spamRow != nullptr && e < nEdges; ++e)
      if (spamRow[e] >= nRows) return (int)hipErrorInvalidValue;
    for (int k = 0; k < nwords; ++k)
      if (words[k] < 0 || words[k] >= S / 64) return (int)hipErrorInvalidValue;
    for (int v = 0; pmaskRow != nullptr && v < nNodes; ++v)
      if (pmaskRow[v] >= nPm) return (int)hipErrorInvalidValue;
  }
  Bufs B;
  const size_t nCnt = (size_t)nRows * (S / 8), nMask = (size_t)nPm * S;
  Dev d;
  std::memset(&d, 0, sizeof(d));
  d.S = S;
  d.W = S / 64;
  d.GR = GR;
  d.spamCnt = B.dev(spamCnt, nCnt);
  auto* drow = B.dev(row, nOps);
  auto* dslot = B.dev(slot, nOps);
  auto* dret = B.dev<int32_t>(nullptr, nOps);
  for (int r = 0; r < nRounds && perRound > 0 && B.ok(); ++r) {
    const size_t o = (size_t)r * perRound;
    hipLaunchKernelGGL(kp_spam_round, dim3(blocks_of(perRound)), dim3(64), 0, 0, d, perRound, drow + o, dslot + o, dret + o);
    B.sync();  // the barrier between rounds
  }
  if (doRetire) {
    d.n0 = 0;
    d.n1 = d.N = nNodes;
    d.rowptr = B.dev(rowptr, (size_t)nNodes + 1);
    if (spamRow != nullptr) d.spamRow = B.dev(spamRow, (size_t)nEdges);
    d.pubmask[cur] = B.dev(pubmask, (size_t)S / 64);
    if (pmaskRow != nullptr) {
      d.pmaskRow = B.dev(pmaskRow, nNodes);
      d.pmask = B.dev(pmask, nMask);
    }
    auto* dwords = B.dev(words, nwords);
    const int64_t nThreads = (int64_t)nNodes * nwords;
    if (B.ok()) hipLaunchKernelGGL(k_retire, dim3((unsigned)((nThreads + 255) / 256)), dim3(256), 0, 0, d, cur, dwords, nwords);
    B.sync();
    if (pmaskRow != nullptr) B.back(pmask, d.pmask, nMask);
  }
  B.back(spamCnt, d.spamCnt, nCnt);
  B.back(ret, dret, nOps);
  return (int)B.err;
}

// One launch of nBlocks blocks; lane 0 of block b calls pool_take(d, cur,
// n[b]) and out[b] is its result (n[b] == 0: no call, out[b] = 0).  poolCnt
// [2][poolSub * 16] and err [1] are in/out.
int gsp_pool_take(int poolSub, int poolS0Mask, int64_t poolSubCap, int64_t poolBase0, int cur, int nBlocks,
                  const uint64_t* n, uint64_t* out, uint64_t* poolCnt, int32_t* err) {
  if (poolSub < 1 || poolSub > 64 || (poolSub & (poolSub - 1)) != 0 || poolS0Mask < 0 || poolSubCap < 0 ||
      poolSubCap > ((int64_t)1 << 40) || poolBase0 < 0 || cur < 0 || cur > 1 || nBlocks < 1 || nBlocks > (1 << 20))
    return (int)hipErrorInvalidValue;
  for (int b = 0; b < nBlocks; ++b)
    if (n[b] > (1ull << 31)) return (int)hipErrorInvalidValue;
  Bufs B;
  const size_t nCnt = (size_t)2 * poolSub * 16;
  Dev d;
  std::memset(&d, 0, sizeof(d));
  d.poolSub = poolSub;
  d.poolS0Mask = poolS0Mask;
  d.poolSubCap = poolSubCap;
  d.poolBase0 = poolBase0;
  d.poolCap = poolSubCap * poolSub;
  d.poolCnt = (unsigned long long*)B.dev(poolCnt, nCnt);
  d.err = B.dev(err, 1);
  auto* dn = (const unsigned long long*)B.dev(n, nBlocks);
  auto* dout = B.dev<unsigned long long>(nullptr, nBlocks);
  if (B.ok()) hipLaunchKernelGGL(kp_pool_take, dim3(nBlocks), dim3(64), 0, 0, d, cur, dn, dout);
  B.sync();
  B.back(out, (const uint64_t*)dout, nBlocks);
  B.back(poolCnt, (const uint64_t*)d.poolCnt, nCnt);
  B.back(err, d.err, 1);
  return (int)B.err;
}

}  // extern "C"
