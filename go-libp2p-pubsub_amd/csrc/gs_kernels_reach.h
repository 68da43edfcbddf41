// gs_kernels_reach.h — mesh reach (include/gs_mesh_reach.h).
//
// A tick runs at the end of a hop and writes no engine state.  A pass searches
// breadth first from up to 64 sources at once over two uint64 [N][T] tables, R0
// and R1: bit j of R[v][t] says "v holds topic t's message of the pass's source
// j".  64 publishers cost one walk of the edges per level, not 64.
//   k_reach_members  lanes/(node, topic)  the members of every topic, once per tick
//   k_reach_init     thread/(source, topic)  the source's bit in its own row of
//                                         the cleared R0, its depth bytes 0
//   k_reach_level    lanes/(node, topic)  one level: next = prev | the OR of prev
//                                         over the in-neighbours by eager edges
//   k_reach_finish   thread/(source, topic)  UNREACHED = targets - REACHED
//
// A level reads one table and writes the other, every word of it, and never
// updates in place: a word written at this level is not seen before the next
// launch, so a bit arrives exactly one level after the bit it came from and
// the level of its arrival is the exact depth, whatever the order of
// execution.  No atomics on the tables.  newly = next & ~prev is this level's
// arrivals; the level number is uniform per launch.
//
// The gather runs at the receiver: v walks its own edges e = (v -> u) and tests
// bit t of (mesh | fanout)[rev[e]], the eager edge u -> v.  A node that is no
// member of t keeps its word (its own source bit, if it is a source) and
// gathers nothing, so it relays its own message and nothing else.  A node
// whose word already holds every bit of the pass skips its gather: nothing new
// can arrive.
//
// Lane layout as in gs_kernels_mesh.h (mesh_tp, mesh_groups, mesh_lane): a
// node's T words are contiguous, lane = topic; at mesh_tp(T) == 64 the node is
// wave-uniform (WIDE): lane j loads edge j's words once, coalesced, and the
// wave walks them with readlane, four neighbour rows in flight.
//
// Counting: an arrival adds 1 to the workgroup's LDS count of its (source,
// topic); at the end the non-zero counts go to the tick's row with one 64-bit
// atomic each (REACHED, the level's depth bin) and an atomicMax of the level
// (ECC).  All integer adds and one max.
#pragma once
#include "gs_kernels_mesh.h"
#include "../../include/gs_mesh_reach.h"

#define GS_REACH_BATCH 4  // levels per host flag read
// a tick's row: [K][T][GS_REACH_ROW_FIELDS], then depth_hist [K][T][GS_REACH_DEPTH_BINS]
#define GS_REACH_ROW_T (GS_REACH_ROW_FIELDS + GS_REACH_DEPTH_BINS)
__host__ __device__ __forceinline__ int64_t reach_row_len(int K, int T) { return (int64_t)K * T * GS_REACH_ROW_T; }
// the counters of a tick besides the row (the byte count)
enum { GS_REACH_W_GATHER = 0, GS_REACH_W_EDGES, GS_REACH_W_DEPTHS, GS_REACH_W_NUM };

__global__ __launch_bounds__(GS_MESH_BLOCK) void k_reach_members(Dev d, const uint8_t* __restrict__ include,
                                                                  uint32_t* __restrict__ members) {
  __shared__ uint32_t sM[64];
  if (threadIdx.x < 64) sM[threadIdx.x] = 0u;
  __syncthreads();
  const int T = d.T, tp = mesh_tp(T);
  const int64_t groups = mesh_groups(d.N, T);
  const int64_t stride = (int64_t)gridDim.x * (GS_MESH_BLOCK / 64);
  uint32_t n = 0;
  for (int64_t g = (int64_t)blockIdx.x * (GS_MESH_BLOCK / 64) + (threadIdx.x >> 6); g < groups; g += stride) {
    const MeshLane x = mesh_lane(d, g, tp);
    n += x.in && mesh_member(d, include, x.u, x.t) ? 1u : 0u;
  }
  if (n) atomicAdd(&sM[lane_id() & (tp - 1)], n);
  __syncthreads();
  if (threadIdx.x < T && sM[threadIdx.x]) atomicAdd(&members[threadIdx.x], sM[threadIdx.x]);
}

// R0 has been cleared, the depth table filled with 255.  src: the pass's ns
// sources; depths: the pass's part [ns][N][T] of the depth table, or nullptr.
__global__ void k_reach_init(Dev d, const int32_t* __restrict__ src, int ns, uint64_t* __restrict__ R0,
                             uint8_t* __restrict__ depths) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ns * d.T) return;
  const int j = i / d.T, t = i - j * d.T;
  const int64_t li = (int64_t)src[j] * d.T + t;
  R0[li] = 1ull << j;  // the sources are distinct: one writer per word
  if (depths != nullptr) depths[(int64_t)j * d.N * d.T + li] = 0;
}

// Level `level` (1, 2, ...) of a pass.  flag[0] == 0: the level before set
// nothing and this launch returns at once, leaving both tables as they are;
// flag[1] is set when this one sets a bit.  full: the pass's bits.  row, hist:
// the pass's part of the tick's row.  words[GS_REACH_W_NUM]: the byte count.
template <bool WIDE>
__global__ __launch_bounds__(GS_MESH_BLOCK) void k_reach_level(
    Dev d, const uint8_t* __restrict__ include, const uint64_t* __restrict__ prev, uint64_t* __restrict__ next,
    uint64_t full, int level, uint32_t* __restrict__ flag, unsigned long long* __restrict__ row,
    unsigned long long* __restrict__ hist, uint8_t* __restrict__ depths, unsigned long long* __restrict__ words) {
  if (flag[0] == 0u) return;
  __shared__ uint32_t sCnt[64 * 64];  // [source][mesh_tp(T)]
  __shared__ uint32_t sWords[GS_REACH_W_NUM];
  const int T = d.T, tp = mesh_tp(T), lane = lane_id();
  for (int i = threadIdx.x; i < 64 * tp; i += GS_MESH_BLOCK) sCnt[i] = 0u;
  if (threadIdx.x < GS_REACH_W_NUM) sWords[threadIdx.x] = 0u;
  __syncthreads();
  const int64_t groups = mesh_groups(d.N, T);
  const int64_t stride = (int64_t)gridDim.x * (GS_MESH_BLOCK / 64);
  const int64_t nt = (int64_t)d.N * T;
  const uint8_t lv = (uint8_t)(level < 254 ? level : 254);
  bool changed = false;
  uint32_t nGather = 0, nEdges = 0, nDepths = 0;
  for (int64_t g = (int64_t)blockIdx.x * (GS_MESH_BLOCK / 64) + (threadIdx.x >> 6); g < groups; g += stride) {
    const MeshLane x = mesh_lane(d, g, tp);
    const int64_t li = (int64_t)x.u * T + x.t;
    const uint64_t old = x.in ? prev[li] : 0ull;
    const bool act = x.in && old != full && mesh_member(d, include, x.u, x.t);
    uint64_t acc = old;
    if constexpr (WIDE) {  // node g is the wave's (the idle lanes t >= T walk its edges too)
      if (__ballot(act) != 0ull) {
        const int64_t base = d.rowptr[g];
        const int deg = (int)(d.rowptr[g + 1] - base);
        uint64_t mm = 0ull;
        int c = 0;
        if (lane < deg) {
          const int64_t r = d.rev[base + lane];
          mm = d.mesh[r] | d.fanout[r];
          c = d.col[base + lane];
        }
        if (lane == 0) nEdges += (uint32_t)deg;
        uint64_t left = __ballot(mm != 0ull);
        while (left) {  // four edges' rows in flight
          uint64_t y[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            y[k] = 0ull;
            if (!left) continue;
            const int j = __ffsll((long long)left) - 1;
            left &= left - 1;
            const uint64_t mj = lane_get64(mm, j);
            const int cj = lane_get(c, j);
            if (act && ((mj >> x.t) & 1)) {
              y[k] = prev[(int64_t)cj * T + x.t];
              ++nGather;
            }
          }
#pragma unroll
          for (int k = 0; k < 4; ++k) acc |= y[k];
        }
      }
    } else {
      if (act) {
        const int64_t e0 = d.rowptr[x.u], e1 = d.rowptr[x.u + 1];
        for (int64_t e = e0; e < e1; ++e) {
          const int64_t r = d.rev[e];
          if (!(((d.mesh[r] | d.fanout[r]) >> x.t) & 1)) continue;
          acc |= prev[(int64_t)d.col[e] * T + x.t];
          ++nGather;
        }
        // the lanes of a node read the same edge words: counted by the first of them
        const uint64_t mates = (__ballot(1) >> (lane & ~(tp - 1))) & ((1ull << tp) - 1ull);
        if ((lane & (tp - 1)) == __ffsll((long long)mates) - 1) nEdges += (uint32_t)(e1 - e0);
      }
    }
    if (x.in) next[li] = acc;
    uint64_t newly = acc & ~old;
    changed |= newly != 0ull;
    while (newly) {
      const int j = __ffsll((long long)newly) - 1;
      newly &= newly - 1;
      atomicAdd(&sCnt[j * tp + x.t], 1u);
      if (depths != nullptr) {
        depths[(int64_t)j * nt + li] = lv;
        ++nDepths;
      }
    }
  }
  if (nGather) atomicAdd(&sWords[GS_REACH_W_GATHER], nGather);
  if (nEdges) atomicAdd(&sWords[GS_REACH_W_EDGES], nEdges);
  if (nDepths) atomicAdd(&sWords[GS_REACH_W_DEPTHS], nDepths);
  const int any = __syncthreads_or(changed ? 1 : 0);
  const int bin = level < GS_REACH_DEPTH_BINS - 1 ? level : GS_REACH_DEPTH_BINS - 1;
  for (int i = threadIdx.x; i < 64 * tp; i += GS_MESH_BLOCK) {
    const uint32_t c = sCnt[i];
    if (!c) continue;
    const int64_t kt = (int64_t)(i / tp) * T + (i & (tp - 1));  // (source, topic); only t < T is ever counted
    atomicAdd(&row[kt * GS_REACH_ROW_FIELDS + GS_REACH_REACHED], (unsigned long long)c);
    atomicMax(&row[kt * GS_REACH_ROW_FIELDS + GS_REACH_ECC], (unsigned long long)level);
    atomicAdd(&hist[kt * GS_REACH_DEPTH_BINS + bin], (unsigned long long)c);
  }
  if (threadIdx.x == 0 && any) flag[1] = 1u;
  if (threadIdx.x < GS_REACH_W_NUM && sWords[threadIdx.x])
    atomicAdd(&words[threadIdx.x], (unsigned long long)sWords[threadIdx.x]);
}

// After a pass's last level: UNREACHED = the topic's members, less the source
// itself where it is one, less REACHED.
__global__ void k_reach_finish(Dev d, const uint8_t* __restrict__ include, const int32_t* __restrict__ src, int ns,
                               const uint32_t* __restrict__ members, unsigned long long* __restrict__ row) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ns * d.T) return;
  const int j = i / d.T, t = i - j * d.T;
  const unsigned long long targets = members[t] - (mesh_member(d, include, src[j], t) ? 1u : 0u);
  unsigned long long* const r = row + (int64_t)i * GS_REACH_ROW_FIELDS;
  r[GS_REACH_UNREACHED] = targets - r[GS_REACH_REACHED];
}
