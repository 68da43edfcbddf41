// gs_kernels_insp.h — WithPeerScoreInspect (include/gs_inspect.h).
//
// A tick runs at the end of a hop, after score_rows<0> left every owned
// edge's exact score in a scratch array (the pass gs_read_scores runs):
// k_inspect_reduce bins the scores and counts the mesh degrees per topic into
// the tick's row, k_inspect_gather copies the sampled edges' scores and
// snapshot fields into the tick's ring slot.  Integer sums only: a row is the
// same bit for bit whatever the order of the adds.
#pragma once
#include "gs_kernels.h"
#include "../../include/gs_inspect.h"

#define GS_INSP_BLOCK 256  // threads of a k_inspect_reduce workgroup: four nodes per pass
#ifndef GS_INSP_WGS_PER_CU
#define GS_INSP_WGS_PER_CU 8  // k_inspect_reduce's grid cap (every workgroup flushes its table once)
#endif
#define GS_INSP_CU_LDS (160u << 10)  // LDS of one gfx950 CU: bounds the resident workgroups
// a row: score_hist[nb + 1], then mesh_deg[T][GS_INSPECT_DEG_BINS]
__host__ __device__ __forceinline__ int insp_row_len(int nb, int T) { return nb + 1 + T * GS_INSPECT_DEG_BINS; }
// k_inspect_reduce's LDS: a row of uint32 (dynamic) and the 64 padded bounds
__host__ __device__ __forceinline__ size_t insp_row_lds(int nb, int T) { return (size_t)insp_row_len(nb, T) * 4; }
__host__ __device__ __forceinline__ size_t insp_lds_bytes(int nb, int T) { return insp_row_lds(nb, T) + 64 * 8; }

// One wave per owned node, lane = out-edge (degree <= 64), nodes grid-strided
// over a capped grid.  `score` holds the exact scores of the owned edges;
// bounds[nb] are strictly ascending.  A floodsub / randomsub host keeps no
// peerScore and no mesh: its edges' scores and its degrees count as 0.
//   score bin   the number of bounds <= s, by a branch-free binary search of
//               the bounds in LDS padded with +inf to 63 entries; the wave adds
//               once per distinct bin present (most scores share two or three).
//   mesh degree wave_transpose64 gives lane t the edge mask of topic t, its
//               popcount is the degree; lanes t < T add 1 to deg[t][d].
// The workgroup's non-zero LDS entries go to the tick's row, one atomic each.
__global__ __launch_bounds__(GS_INSP_BLOCK) void k_inspect_reduce(Dev d, const double* __restrict__ score,
                                                                  const double* __restrict__ bounds, int nb,
                                                                  unsigned long long* __restrict__ row) {
  extern __shared__ __attribute__((aligned(16))) uint32_t sRow[];  // [rowLen]
  __shared__ double sB[64];
  const int T = d.T;
  const int rowLen = insp_row_len(nb, T);
  for (int i = threadIdx.x; i < rowLen; i += GS_INSP_BLOCK) sRow[i] = 0u;
  if (threadIdx.x < 64) sB[threadIdx.x] = threadIdx.x < nb ? bounds[threadIdx.x] : __builtin_inf();
  __syncthreads();
  uint32_t* const sDeg = sRow + nb + 1;
  const int lane = lane_id();
  const int64_t stride = (int64_t)gridDim.x * (GS_INSP_BLOCK / 64);
  for (int64_t v = d.n0 + (int64_t)blockIdx.x * (GS_INSP_BLOCK / 64) + (threadIdx.x >> 6); v < d.n1; v += stride) {
    const int64_t base = d.rowptr[v];
    const int deg = (int)(d.rowptr[v + 1] - base);
    const bool gossip = gossip_host(d, (int)v);
    const bool in = lane < deg;
    double s = 0.0;
    uint64_t m = 0ull;
    if (in && gossip) {
      s = score[base + lane];
      m = d.mesh[base + lane];
    }
    int bin = 0;
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1) bin += sB[bin + step - 1] <= s ? step : 0;
    bin = bin < nb ? bin : nb;  // (only a score of +inf passes the padding)
    uint64_t left = __ballot(in);
    while (left) {
      const int leader = __ffsll((long long)left) - 1;
      const int b = __shfl(bin, leader);
      const uint64_t same = __ballot(in && bin == b);
      if (lane == leader) atomicAdd(&sRow[b], (uint32_t)__popcll(same));
      left &= ~same;
    }
    const int dg = __popcll(wave_transpose64(m));
    if (lane < T) atomicAdd(&sDeg[lane * GS_INSPECT_DEG_BINS + dg], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < rowLen; i += GS_INSP_BLOCK) {
    const uint32_t c = sRow[i];
    if (c) atomicAdd(&row[i], (unsigned long long)c);
  }
}

// The sampled edges' scores and, with ext != nullptr, their snapshot fields at
// one tick.  Thread per (sampled edge, topic): topic 0's thread writes the
// per-edge fields.  ext holds, one after the other, app[n], ipc[n], bp[n],
// timeInMesh[n][T] (int64), fmd[n][T], mmd[n][T], imd[n][T]; pending
// deliveries are applied as k_gather_pairs does.  An edge without a record,
// and an edge of a host that is not gossipsub, reads 0 in every field.
__global__ void k_inspect_gather(Dev d, const int64_t* __restrict__ edges, int64_t n,
                                 const double* __restrict__ score, double* __restrict__ outScore,
                                 double* __restrict__ ext) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nk = n * d.T;
  if (k >= nk) return;
  const int64_t j = k / d.T;
  const int t = (int)(k - j * d.T);
  const int64_t e = edges[j];
  const bool gossip = gossip_host(d, d.esrc[e]);
  const bool rec = gossip && d.scoring && has_record(d, e);
  if (t == 0) {
    outScore[j] = gossip ? score[e] : 0.0;
    if (ext != nullptr) {
      ext[j] = rec ? d.app[d.col[e]] : 0.0;
      ext[n + j] = rec ? d.p6[e] : 0.0;
      ext[2 * n + j] = rec ? d.bp[e] : 0.0;
    }
  }
  if (ext == nullptr) return;
  int64_t* const tim = reinterpret_cast<int64_t*>(ext + 3 * n);
  double* const fmd = ext + 3 * n + nk;
  double* const mmd = fmd + nk;
  double* const imd = mmd + nk;
  if (!rec) {
    tim[k] = 0;
    fmd[k] = 0.0;
    mmd[k] = 0.0;
    imd[k] = 0.0;
    return;
  }
  const int64_t i = tix(d, t, e);
  const TopicP& tp = d.tp[t];
  const uint32_t q = dlt_get(d, i);
  tim[k] = (d.flags[i] & 1) ? mesh_time_of(d.lastRefresh, d.graftTime[i]) : 0;
  fmd[k] = eff_fmd(tp, d.fmd[i], q);
  mmd[k] = eff_mmd(tp, d.mmd[i], q);
  imd[k] = d.imd[i];
}
