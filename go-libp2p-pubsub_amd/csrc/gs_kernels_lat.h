// gs_kernels_lat.h — propagation-latency statistics (include/gs_latency.h).
//
// Within one hop every first delivery of slot s has the same age,
// h - slotPubHop[s], so a hop's whole contribution to the histograms is one
// count per slot.  Phase A leaves each owned node's first deliveries of the
// hop in its frontier list fl[cur][v] (k_phase_a) or its frontier bitmap
// fb[cur][v] (k_flood_a); k_lat_count sums them per slot into latCnt[S] after
// phase A and before the hop's own publishes are added (k_publish /
// k_publist), k_lat_fold turns the counts into histogram entries.  A
// GS_BEHAVE_NO_FORWARD host keeps no list: k_phase_a counts its deliveries
// into latCnt itself (pass 2b).  Integer sums only: the tables are the same
// bit for bit whatever the order of the adds.
#pragma once
#include "gs_kernels.h"

#define GS_LAT_BLOCK 256  // threads of a k_lat_count workgroup
#define GS_LAT_GROUP 16   // lanes that read one node's list: 16 x 16 bytes = 64 entries per pass
#ifndef GS_LAT_WGS_PER_CU
#define GS_LAT_WGS_PER_CU 4  // k_lat_count's grid cap (every workgroup flushes its table once)
#endif
#define GS_LAT_CU_LDS (160u << 10)  // LDS of one gfx950 CU: bounds the resident workgroups

// First deliveries of the hop per slot, over the owned nodes [n0, n1).  A
// capped grid; each workgroup walks its nodes grid-strided and counts into an
// LDS table of one uint32 per slot (S <= 16384: at most 64 KB; only the words
// of amR, which hold every message a sender's frontier can carry, are zeroed
// and flushed), then adds its non-zero entries to latCnt, one atomic each.
// BITMAP: the nodes' fb rows (rows with fbN == 0 are all zero and not read),
// one wave per node; otherwise their lists, GS_LAT_GROUP lanes per node
// reading whole 16-byte blocks (FC is a multiple of 4, so a row starts on
// one).  fln is clamped to FC (that hop fails with E_FCAP).
template <bool BITMAP>
__global__ __launch_bounds__(GS_LAT_BLOCK) void k_lat_count(Dev d, int cur, WMask amR) {
  extern __shared__ __attribute__((aligned(16))) uint32_t sLat[];  // [S]
  const int S = d.S, W = d.W;
  for (int s = threadIdx.x; s < S; s += GS_LAT_BLOCK)
    if (wm_has(amR, s >> 6)) sLat[s] = 0u;
  __syncthreads();
  if constexpr (BITMAP) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * (GS_LAT_BLOCK / 64);
    for (int64_t v = d.n0 + (int64_t)blockIdx.x * (GS_LAT_BLOCK / 64) + (threadIdx.x >> 6); v < d.n1; v += stride) {
      if (d.fbN[cur][v] == 0) continue;
      const uint64_t* row = d.fb[cur] + v * W;
      for (int w = lane; w < W; w += 64) {
        if (!wm_has(amR, w)) continue;
        for (uint64_t y = row[w]; y; y &= y - 1) atomicAdd(&sLat[w * 64 + __ffsll((long long)y) - 1], 1u);
      }
    }
  } else {
    const int gl = threadIdx.x & (GS_LAT_GROUP - 1);
    const int FC = d.FC;
    const int64_t stride = (int64_t)gridDim.x * (GS_LAT_BLOCK / GS_LAT_GROUP);
    // An entry outside amR's words (a first delivery later than the window: that hop fails with
    // E_LATE) adds into an entry that was not zeroed; it is never flushed, so it is dropped.
    auto count = [&](uint32_t ent) {  // slot | tag << 16; tag 255 = an own publish (none yet at this point)
      const int slot = (int)(ent & 0xFFFFu);
      if ((ent >> 16) != 255u && slot < S) atomicAdd(&sLat[slot], 1u);
    };
    for (int64_t v = d.n0 + (int64_t)blockIdx.x * (GS_LAT_BLOCK / GS_LAT_GROUP) + (threadIdx.x / GS_LAT_GROUP);
         v < d.n1; v += stride) {
      int len = d.fln[cur][v];
      len = len < FC ? len : FC;
      const uint4* L = reinterpret_cast<const uint4*>(d.fl[cur] + v * FC);
      for (int k = gl * 4; k < len; k += GS_LAT_GROUP * 4) {
        const uint4 x = L[k >> 2];
        count(x.x);
        if (k + 1 < len) count(x.y);
        if (k + 2 < len) count(x.z);
        if (k + 3 < len) count(x.w);
      }
    }
  }
  __syncthreads();
  for (int s = threadIdx.x; s < S; s += GS_LAT_BLOCK) {
    if (!wm_has(amR, s >> 6)) continue;
    const uint32_t c = sLat[s];
    if (c) atomicAdd(&d.latCnt[s], c);
  }
}

// Thread per slot: the hop's count of slot s becomes entry (s, a) of the
// per-message table and is added to entry (topic, a) of the per-topic one, a =
// h - slotPubHop[s]; latCnt is left zero for the next hop.  A (slot, age) pair
// is touched in one hop only, so the per-message store needs no atomic.  An
// age outside [0, the topic's own limit] is dropped: that hop fails with E_LATE.
__global__ void k_lat_fold(Dev d, int64_t h, int bins, uint32_t* __restrict__ mhist,
                           unsigned long long* __restrict__ hist) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= d.S) return;
  const uint32_t c = d.latCnt[s];
  if (c == 0) return;
  d.latCnt[s] = 0u;
  const int64_t a = h - d.slotPubHop[s];
  const int t = slot_topic(d, s);
  if (a < 0 || a >= bins || a > topic_age(d, t)) return;
  mhist[(int64_t)s * bins + a] = c;
  atomicAdd(&hist[(int64_t)t * bins + a], (unsigned long long)c);
}

// The per-message rows of the slots this hop's publishes take over start from
// zero (before k_publish).  One workgroup per publish.
__global__ void k_lat_clear(Dev d, int b, int bins, uint32_t* __restrict__ mhist) {
  uint32_t* row = mhist + (int64_t)d.mSlot[b + blockIdx.x] * bins;
  for (int a = threadIdx.x; a < bins; a += blockDim.x) row[a] = 0u;
}
