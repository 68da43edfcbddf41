// gs_kernels_mesh.h — mesh health (include/gs_mesh_health.h).
//
// A tick runs at the end of a hop and writes no engine state.  Two uint32
// [N][T] tables: L, the labels (GS_MESH_NONE for a non-member), and Z, the
// component sizes at the roots.
//   k_mesh_init    thread/(node, topic)  L = own id for a member, Z = 0
//   k_mesh_label   lanes/(node, topic)   one iteration: m = min over the mutual
//                                        neighbours' L, then m = L[m] twice;
//                                        L and L[L] take m (hooking)
//   k_mesh_sizes   lanes/(node, topic)   Z[L] += 1, runs of equal labels summed first
//   k_mesh_row     lanes/(node, topic)   the tick's row: per root, per node's edges
// The mutual mask mesh[e] & mesh[rev[e]] is taken on the fly:
// a neighbour that is not a member reads GS_MESH_NONE and never wins a min, so
// an iteration needs no member test of the neighbour.
//
// Lane layout of the last three: a node's T labels are contiguous, lane = topic.
// mesh_tp(T) lanes per node (the next power of two), 64 / mesh_tp(T) nodes per
// wave, so a wave carries no idle lanes at small T.  At mesh_tp(T) == 64 the
// node is wave-uniform (WIDE): lane j loads edge j's words once and the wave
// walks them with readlane; otherwise every lane walks its own node's edges
// (the lanes of a node read the same words: one request).
//
// Order independence: a label is only ever lowered (atomicMin), to the label of
// a node of the same component, so L[x] <= x throughout.  A load that sees
// another workgroup's older value sees a larger valid label: it costs
// progress, never correctness.  Every write of a launch is visible to the
// next launch, and an iteration that finds nothing to lower writes nothing, so
// it has read a fixed point: no mutual neighbour holds a smaller label, hence
// one label c per component, c a member and c <= every member: the smallest
// id.  An iteration lowers a label at least as far as plain propagation of the
// minimum does, which settles in fewer than N iterations.  All counts are
// integer adds.
#pragma once
#include "gs_kernels.h"
#include "../../include/gs_mesh_health.h"

#define GS_MESH_BLOCK 256      // four waves
#define GS_MESH_WGS_PER_CU 8   // grid cap of the three node passes: full occupancy, no tail
#define GS_MESH_BATCH 4        // label iterations per host flag read
#define GS_MESH_NONE 0xFFFFFFFFu
// a tick's row: [T][GS_MESH_ROW_FIELDS], then comp_hist [T][GS_MESH_SIZE_BINS]
#define GS_MESH_ROW_T (GS_MESH_ROW_FIELDS + GS_MESH_SIZE_BINS)
__host__ __device__ __forceinline__ int mesh_row_len(int T) { return T * GS_MESH_ROW_T; }
// lanes per node: the smallest power of two >= T
__host__ __device__ __forceinline__ int mesh_tp(int T) {
  int p = 1;
  while (p < T) p <<= 1;
  return p;
}
// groups of 64 / mesh_tp(T) consecutive nodes: a wave's unit of work
__host__ __device__ __forceinline__ int64_t mesh_groups(int N, int T) {
  const int npw = 64 / mesh_tp(T);
  return ((int64_t)N + npw - 1) / npw;
}

__device__ __forceinline__ bool mesh_member(const Dev& d, const uint8_t* __restrict__ include, int v, int t) {
  return (include == nullptr || include[v] != 0) && gossip_host(d, v) && ((d.sub[v] >> t) & 1);
}

__global__ void k_mesh_init(Dev d, const uint8_t* __restrict__ include, uint32_t* __restrict__ L,
                            uint32_t* __restrict__ Z) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)d.N * d.T) return;
  int64_t v;
  int t;
  pair_split(d, i, v, t);
  L[i] = mesh_member(d, include, (int)v, t) ? (uint32_t)v : GS_MESH_NONE;
  Z[i] = 0u;
}

// The lane's (node, topic) of group g; t >= T or u >= N: an idle lane.
struct MeshLane {
  int u, t;
  bool in;
};
__device__ __forceinline__ MeshLane mesh_lane(const Dev& d, int64_t g, int tp) {
  const int lane = lane_id();
  MeshLane x;
  x.t = lane & (tp - 1);
  const int64_t u = g * (64 / tp) + lane / tp;
  x.in = u < d.N && x.t < d.T;
  x.u = x.in ? (int)u : 0;
  return x;
}

// One label iteration.  flag[0] == 0: the previous iteration lowered nothing
// and this launch returns at once; flag[1] is set when this one lowers a label.
// words: the labels loaded and stored besides the lanes' own (the byte count).
template <bool WIDE>
__global__ __launch_bounds__(GS_MESH_BLOCK) void k_mesh_label(Dev d, uint32_t* L, uint32_t* __restrict__ flag,
                                                               unsigned long long* __restrict__ words) {
  if (flag[0] == 0u) return;
  __shared__ uint32_t sWords;
  if (threadIdx.x == 0) sWords = 0u;
  const int T = d.T, tp = mesh_tp(T), lane = lane_id();
  const int64_t groups = mesh_groups(d.N, T);
  const int64_t stride = (int64_t)gridDim.x * (GS_MESH_BLOCK / 64);
  bool changed = false;
  uint32_t nw = 0;
  for (int64_t g = (int64_t)blockIdx.x * (GS_MESH_BLOCK / 64) + (threadIdx.x >> 6); g < groups; g += stride) {
    const MeshLane x = mesh_lane(d, g, tp);
    const int64_t li = (int64_t)x.u * T + x.t;
    const uint32_t old = x.in ? L[li] : GS_MESH_NONE;
    const bool act = old != GS_MESH_NONE;
    uint32_t m = old;
    if constexpr (WIDE) {  // node g is the wave's (the idle lanes t >= T walk its edges too)
      const int64_t base = d.rowptr[g];
      const int deg = (int)(d.rowptr[g + 1] - base);
      uint64_t mm = 0ull;
      int c = 0;
      if (lane < deg) {
        mm = d.mesh[base + lane] & d.mesh[d.rev[base + lane]];
        c = d.col[base + lane];
      }
      uint64_t left = __ballot(mm != 0ull);
      while (left) {  // four edges' label rows in flight
        uint32_t y[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          y[k] = GS_MESH_NONE;
          if (!left) continue;
          const int j = __ffsll((long long)left) - 1;
          left &= left - 1;
          const uint64_t mj = lane_get64(mm, j);
          const int cj = lane_get(c, j);
          if (act && ((mj >> x.t) & 1)) {
            y[k] = L[(int64_t)cj * T + x.t];
            ++nw;
          }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) m = y[k] < m ? y[k] : m;
      }
    } else if (act) {
      const int64_t e1 = d.rowptr[x.u + 1];
      for (int64_t e = d.rowptr[x.u]; e < e1; ++e) {
        if (!((d.mesh[e] >> x.t) & 1) || !((d.mesh[d.rev[e]] >> x.t) & 1)) continue;
        const uint32_t y = L[(int64_t)d.col[e] * T + x.t];
        m = y < m ? y : m;
        ++nw;
      }
    }
    if (act) {
      // shorten: m names a member of this component, whose label is <= m
      uint32_t y = L[(int64_t)m * T + x.t];
      m = y < m ? y : m;
      y = L[(int64_t)m * T + x.t];
      m = y < m ? y : m;
      nw += 2;
      if (m < old) {
        // hook: the node this one pointed to takes m too, and everything that
        // points to it follows by shortening (without it the smallest id walks
        // one edge per iteration into a part that has already agreed on a
        // larger one).  Most such lanes find it done: a load from L2 first.
        uint32_t* const up = &L[(int64_t)old * T + x.t];
        if (old != (uint32_t)x.u && m < __hip_atomic_load(up, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
          atomicMin(up, m);
          ++nw;
        }
        atomicMin(&L[li], m);
        changed = true;
        nw += 2;
      }
    }
  }
  __syncthreads();
  if (nw) atomicAdd(&sWords, nw);
  const int any = __syncthreads_or(changed ? 1 : 0);
  if (threadIdx.x == 0) {
    if (any) flag[1] = 1u;
    if (sWords) atomicAdd(words, (unsigned long long)sWords);
  }
}

// Z[label][t] += 1 for every member.  A wave takes consecutive groups, so a
// lane walks nodes in ascending order and adds a run of equal labels once: in
// one large component that is one add per wave and topic, not one per node.
__global__ __launch_bounds__(GS_MESH_BLOCK) void k_mesh_sizes(Dev d, const uint32_t* __restrict__ L,
                                                               uint32_t* __restrict__ Z,
                                                               unsigned long long* __restrict__ words) {
  __shared__ uint32_t sWords;
  if (threadIdx.x == 0) sWords = 0u;
  const int T = d.T, tp = mesh_tp(T);
  const int64_t groups = mesh_groups(d.N, T);
  const int64_t waves = (int64_t)gridDim.x * (GS_MESH_BLOCK / 64);
  const int64_t per = (groups + waves - 1) / waves;
  const int64_t w = (int64_t)blockIdx.x * (GS_MESH_BLOCK / 64) + (threadIdx.x >> 6);
  const int64_t g1 = (w + 1) * per < groups ? (w + 1) * per : groups;
  uint32_t cur = GS_MESH_NONE, run = 0, nw = 0;
  const int t = lane_id() & (tp - 1);
  for (int64_t g = w * per; g < g1; ++g) {
    const MeshLane x = mesh_lane(d, g, tp);
    const uint32_t lab = x.in ? L[(int64_t)x.u * T + x.t] : GS_MESH_NONE;
    if (lab == cur) {
      run += lab != GS_MESH_NONE ? 1u : 0u;
      continue;
    }
    if (run) {
      atomicAdd(&Z[(int64_t)cur * T + t], run);
      ++nw;
    }
    cur = lab;
    run = lab != GS_MESH_NONE ? 1u : 0u;
  }
  // the last runs: the lanes of one topic (tp apart) that end on the same label
  // fold into the lowest of them, so at T = 1 a wave inside one component adds
  // once, not 64 times to one address; then one add instruction for the wave
  // (at T = 64 its 64 lanes on one 256-byte row)
  for (int off = tp; off < 64; off <<= 1) {
    const uint32_t oc = (uint32_t)__shfl_xor((int)cur, off), orun = (uint32_t)__shfl_xor((int)run, off);
    if (run != 0u && orun != 0u && oc == cur) run = (lane_id() & off) ? 0u : run + orun;
  }
  if (run) {
    atomicAdd(&Z[(int64_t)cur * T + t], run);
    ++nw;
  }
  __syncthreads();
  if (nw) atomicAdd(&sWords, nw);
  __syncthreads();
  if (threadIdx.x == 0 && sWords) atomicAdd(words, (unsigned long long)sWords);
}

// The tick's row.  A lane keeps its topic's counts in registers over the
// nodes it visits; the workgroup sums them in LDS and adds its non-zero
// entries to the row, one atomic each (largest: a max).
//   per root (L == own id)  components, members (the sizes add up to them),
//                           largest, isolated (size 1), comp_hist
//   per member's edges      one_sided, outside, eclipsed
template <bool WIDE>
__global__ __launch_bounds__(GS_MESH_BLOCK) void k_mesh_row(Dev d, const uint8_t* __restrict__ include,
                                                             const uint32_t* __restrict__ L,
                                                             const uint32_t* __restrict__ Z,
                                                             unsigned long long* __restrict__ row) {
  __shared__ uint32_t sRow[64 * GS_MESH_ROW_T];
  const int T = d.T, tp = mesh_tp(T), lane = lane_id();
  const int rowLen = mesh_row_len(T);
  for (int i = threadIdx.x; i < rowLen; i += GS_MESH_BLOCK) sRow[i] = 0u;
  __syncthreads();
  uint32_t* const sHist = sRow + T * GS_MESH_ROW_FIELDS;
  const int64_t groups = mesh_groups(d.N, T);
  const int64_t stride = (int64_t)gridDim.x * (GS_MESH_BLOCK / 64);
  uint32_t acc[GS_MESH_ROW_FIELDS] = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
  int t = lane & (tp - 1);
  for (int64_t g = (int64_t)blockIdx.x * (GS_MESH_BLOCK / 64) + (threadIdx.x >> 6); g < groups; g += stride) {
    const MeshLane x = mesh_lane(d, g, tp);
    const int64_t li = (int64_t)x.u * T + x.t;
    const uint32_t lab = x.in ? L[li] : GS_MESH_NONE;
    const bool act = lab != GS_MESH_NONE;
    if (act && lab == (uint32_t)x.u) {
      const uint32_t s = Z[li];  // >= 1: the root itself
      acc[GS_MESH_COMPONENTS] += 1u;
      acc[GS_MESH_MEMBERS] += s;
      acc[GS_MESH_LARGEST] = s > acc[GS_MESH_LARGEST] ? s : acc[GS_MESH_LARGEST];
      acc[GS_MESH_ISOLATED] += s == 1u ? 1u : 0u;
      atomicAdd(&sHist[x.t * GS_MESH_SIZE_BINS + (31 - __clz((int)(s | 1u)))], 1u);
    }
    bool any = false, inside = false;
    if constexpr (WIDE) {
      const int64_t base = d.rowptr[g];
      const int deg = (int)(d.rowptr[g + 1] - base);
      uint64_t me = 0ull, mr = 0ull;
      bool inc = false;
      if (lane < deg) {
        me = d.mesh[base + lane];
        mr = d.mesh[d.rev[base + lane]];
        inc = include == nullptr || include[d.col[base + lane]] != 0;
      }
      const uint64_t incM = __ballot(inc);
      uint64_t left = __ballot(me != 0ull);
      while (left) {
        const int j = __ffsll((long long)left) - 1;
        left &= left - 1;
        const uint64_t ej = lane_get64(me, j), rj = lane_get64(mr, j);
        if (!act || !((ej >> x.t) & 1)) continue;
        any = true;
        if (!((incM >> j) & 1)) {
          acc[GS_MESH_OUTSIDE] += 1u;
        } else {
          inside = true;
          acc[GS_MESH_ONE_SIDED] += ((rj >> x.t) & 1) ? 0u : 1u;
        }
      }
    } else if (act) {
      const int64_t e1 = d.rowptr[x.u + 1];
      for (int64_t e = d.rowptr[x.u]; e < e1; ++e) {
        if (!((d.mesh[e] >> x.t) & 1)) continue;
        any = true;
        if (include != nullptr && include[d.col[e]] == 0) {
          acc[GS_MESH_OUTSIDE] += 1u;
        } else {
          inside = true;
          acc[GS_MESH_ONE_SIDED] += ((d.mesh[d.rev[e]] >> x.t) & 1) ? 0u : 1u;
        }
      }
    }
    acc[GS_MESH_ECLIPSED] += any && !inside ? 1u : 0u;
  }
  if (t < T) {
#pragma unroll
    for (int f = 0; f < GS_MESH_ROW_FIELDS; ++f) {
      if (!acc[f]) continue;
      if (f == GS_MESH_LARGEST) atomicMax(&sRow[t * GS_MESH_ROW_FIELDS + f], acc[f]);
      else atomicAdd(&sRow[t * GS_MESH_ROW_FIELDS + f], acc[f]);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < rowLen; i += GS_MESH_BLOCK) {
    const uint32_t c = sRow[i];
    if (!c) continue;
    if (i < T * GS_MESH_ROW_FIELDS && i % GS_MESH_ROW_FIELDS == GS_MESH_LARGEST)
      atomicMax(&row[i], (unsigned long long)c);
    else
      atomicAdd(&row[i], (unsigned long long)c);
  }
}
