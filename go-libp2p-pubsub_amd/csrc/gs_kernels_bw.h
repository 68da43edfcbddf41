// gs_kernels_bw.h — bandwidth statistics (include/gs_bandwidth.h).
//
// The RPC accounting keeps, per directed edge and cumulative since the start,
// the bytes and the RPCs sent over it (Dev::rpcB, rpcN); with the statistics
// on, Dev::bwX[e] = {eager, pulled} splits the bytes: k_acct_payload adds what
// it adds to rpcB to `eager`, phase B adds the served messages of an IWANT
// reply to `pulled`.  A tick runs at the end of a hop:
//   k_bw_tick    per node the eight cumulative sums (egress over its out-edges,
//                ingress over their reverse edges; all, eager, pulled, RPCs),
//                the deltas against the previous tick's sums (`prev`, then
//                overwritten) into `delta`, and from the deltas the bins, the
//                totals and the maxima of the tick's row.
//   k_bw_argmax  the lowest node index whose delta equals the row's maximum.
//   k_bw_gather  the sampled nodes' deltas into the tick's ring slot.
// Integer sums, maxima and minima only: a row is the same bit for bit whatever
// the order of the adds.
#pragma once
#include "gs_kernels.h"
#include "../../include/gs_bandwidth.h"

#define GS_BW_BLOCK 256  // threads of a k_bw_tick workgroup: four nodes per pass
#ifndef GS_BW_WGS_PER_CU
#define GS_BW_WGS_PER_CU 8  // k_bw_tick's grid cap (every workgroup flushes its table once)
#endif
// the per-node tables (prev, delta): [N][GS_BW_DIRS][4] = all, eager, pulled, RPCs
#define GS_BW_NODE_WORDS 8
// a row in 8-byte words: total[4], total_rpcs, max[2][4], argmax[2][4], hist[2][4][nb + 1]
#define GS_BW_ROW_MAX 5
#define GS_BW_ROW_ARG 13
#define GS_BW_ROW_HIST 21
__host__ __device__ __forceinline__ int bw_row_len(int nb) { return GS_BW_ROW_HIST + 8 * (nb + 1); }

// Word j = dir * 4 + c of a node's values from its table row x[8]: the bytes
// of class c (overhead = all - eager - pulled).
__device__ __forceinline__ unsigned long long bw_class_value(const unsigned long long* __restrict__ x, int j) {
  const int b = j & 4;
  return (j & 3) == 3 ? x[b] - x[b + 1] - x[b + 2] : x[j];
}

// One wave per node, lane = out-edge (degree <= 64), nodes grid-strided over a
// capped grid.  Each lane loads the four cumulative values of its own edge
// (coalesced) and gathers the same four at rev[e]; eight 64-bit wave sums give
// the node's cumulative values, lanes 0..7 hold one (direction, value) each.
//   bin     the number of bounds <= x, by a branch-free binary search of the
//           bounds in LDS padded with INT64_MAX to 63 entries.
//   totals  from the egress side (the ingress side sums to the same).
// The workgroup's non-zero LDS entries go to the tick's row, one atomic each.
__global__ __launch_bounds__(GS_BW_BLOCK) void k_bw_tick(Dev d, const long long* __restrict__ bounds, int nb,
                                                          unsigned long long* __restrict__ prev,
                                                          unsigned long long* __restrict__ delta,
                                                          unsigned long long* __restrict__ row) {
  __shared__ long long sB[64];
  __shared__ uint32_t sHist[8 * 64];  // [8][nb + 1]
  __shared__ unsigned long long sTot[5], sMax[8];
  const int nh = nb + 1;
  for (int i = threadIdx.x; i < 8 * nh; i += GS_BW_BLOCK) sHist[i] = 0u;
  if (threadIdx.x < 64) sB[threadIdx.x] = (int)threadIdx.x < nb ? bounds[threadIdx.x] : INT64_MAX;
  if (threadIdx.x < 5) sTot[threadIdx.x] = 0ull;
  if (threadIdx.x < 8) sMax[threadIdx.x] = 0ull;
  __syncthreads();
  const ulonglong2* const split = reinterpret_cast<const ulonglong2*>(d.bwX);
  const int lane = lane_id();
  const int j = lane & 7;
  const int64_t stride = (int64_t)gridDim.x * (GS_BW_BLOCK / 64);
  for (int64_t v = d.n0 + (int64_t)blockIdx.x * (GS_BW_BLOCK / 64) + (threadIdx.x >> 6); v < d.n1; v += stride) {
    const int64_t base = d.rowptr[v];
    const int deg = (int)(d.rowptr[v + 1] - base);
    unsigned long long c[8] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    if (lane < deg) {
      const int64_t e = base + lane;
      const int64_t r = d.rev[e];
      const ulonglong2 xe = split[e], xr = split[r];
      c[0] = d.rpcB[e]; c[1] = xe.x; c[2] = xe.y; c[3] = d.rpcN[e];
      c[4] = d.rpcB[r]; c[5] = xr.x; c[6] = xr.y; c[7] = d.rpcN[r];
    }
    unsigned long long cum = 0ull;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const unsigned long long s = wave_sum_ll((long long)c[k]);
      cum = j == k ? s : cum;
    }
    // lanes 0..7: one word of the node's table row each
    unsigned long long dl = 0ull;
    if (lane < 8) {
      const int64_t i = v * GS_BW_NODE_WORDS + j;
      dl = cum - prev[i];
      prev[i] = cum;
      delta[i] = dl;
    }
    const int b4 = lane & 4;
    const unsigned long long d0 = __shfl(dl, b4), d1 = __shfl(dl, b4 + 1), d2 = __shfl(dl, b4 + 2);
    const unsigned long long val = (j & 3) == 3 ? d0 - d1 - d2 : dl;
    if (lane < 8) {
      int bin = 0;
#pragma unroll
      for (int step = 32; step >= 1; step >>= 1) bin += sB[bin + step - 1] <= (long long)val ? step : 0;
      bin = bin < nb ? bin : nb;  // (only INT64_MAX passes the padding)
      atomicAdd(&sHist[j * nh + bin], 1u);
      if (val) atomicMax(&sMax[j], val);
      if (lane < 4 && val) atomicAdd(&sTot[lane], val);
      if (lane == 3 && dl) atomicAdd(&sTot[4], dl);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 8 * nh; i += GS_BW_BLOCK) {
    const uint32_t n = sHist[i];
    if (n) atomicAdd(&row[GS_BW_ROW_HIST + i], (unsigned long long)n);
  }
  if (threadIdx.x < 5 && sTot[threadIdx.x]) atomicAdd(&row[threadIdx.x], sTot[threadIdx.x]);
  if (threadIdx.x < 8 && sMax[threadIdx.x]) atomicMax(&row[GS_BW_ROW_MAX + threadIdx.x], sMax[threadIdx.x]);
}

// The lowest node index that attains each of the row's eight maxima (the
// argmax words start at all ones: a maximum of 0 leaves -1).  Thread per
// (node, word).
__global__ void k_bw_argmax(Dev d, const unsigned long long* __restrict__ delta, unsigned long long* __restrict__ row) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)(d.n1 - d.n0) * GS_BW_NODE_WORDS) return;
  const int64_t v = d.n0 + (i >> 3);
  const int j = (int)(i & 7);
  const unsigned long long m = row[GS_BW_ROW_MAX + j];
  if (m != 0ull && bw_class_value(delta + v * GS_BW_NODE_WORDS, j) == m) atomicMin(&row[GS_BW_ROW_ARG + j], (unsigned long long)v);
}

// The sampled nodes' values at one tick: bytes[n][2][4] and rpcs[n][2].
// Thread per (sampled node, word).
__global__ void k_bw_gather(const int32_t* __restrict__ nodes, int64_t n, const unsigned long long* __restrict__ delta,
                            unsigned long long* __restrict__ bytes, unsigned long long* __restrict__ rpcs) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * GS_BW_NODE_WORDS) return;
  const int64_t s = i >> 3;
  const int j = (int)(i & 7);
  const unsigned long long* const x = delta + (int64_t)nodes[s] * GS_BW_NODE_WORDS;
  bytes[i] = bw_class_value(x, j);
  if ((j & 3) == 3) rpcs[2 * s + (j >> 2)] = x[j];
}
