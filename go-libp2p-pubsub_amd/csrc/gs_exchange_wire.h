// gs_exchange_wire.h — the layouts of the per-hop exchange of a partitioned
// engine (gs_exchange.h), stated once for both ends.  Plain
// host C++17, no HIP: the engine includes it, and so does the stand-alone
// check tests/exchange_wire_check.cpp.
//
// Per hop a rank
//   1. counts on the device (XCnt, XpCnt) and reads the counts back (Readback);
//   2. packs its broadcast chunk (Bcast), its edge records and its push blocks
//      (planSend: one block per destination rank each);
//   3. all-gathers one SizeRow per rank, from which every rank derives what it
//      receives (planRecv) and how rank r's chunk is laid out (Bcast again);
//   4. all-gathers the chunks, all-gathers the dials (packDials), all-to-all-v's
//      the edge records, all-to-all-v's the push blocks.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace gsx {

constexpr int64_t kXRecBytes = 96, kPRecBytes = 16;  // sizeof(XRec), sizeof(PRec): asserted in gs_exchange.h

inline size_t align8(size_t x) { return (x + 7) & ~(size_t)7; }

// off[i] = v[0] + ... + v[i-1]; returns the total.
inline int64_t exclusivePrefix(const std::vector<int64_t>& v, std::vector<int64_t>& off) {
  int64_t tot = 0;
  off.resize(v.size());
  for (size_t i = 0; i < v.size(); ++i) {
    off[i] = tot;
    tot += v[i];
  }
  return tot;
}

// ---- device counter blocks (views: the pointers are device addresses) ----
// Edge records: counts per destination (k_x_count), pack cursors per
// destination (k_x_pack), the list entries' bump offset (k_x_lists).
struct XCnt {
  unsigned long long* p;
  int world;
  static size_t words(int world) { return 2 * (size_t)world + 1; }
  unsigned long long* counts() const { return p; }           // [world]
  unsigned long long* cursors() const { return p + world; }  // [world]
  unsigned long long* bump() const { return p + 2 * world; }
};
// Push blocks: records and slots per destination (k_xp_count), then the same
// pair as pack cursors (k_xp_pack).
struct XpCnt {
  unsigned long long* p;
  int world;
  static size_t countWords(int world) { return 2 * (size_t)world; }
  static size_t words(int world) { return 2 * countWords(world); }
  unsigned long long* counts() const { return p; }                       // [world] records, [world] slots
  unsigned long long* cursors() const { return p + countWords(world); }  // [world] records, [world] slots
};
// k_xp_pack's block byte offsets and record counts per destination (a view
// over the device array and over the host vector uploaded to it).
struct XpOff {
  int64_t* p;
  int world;
  static size_t words(int world) { return 2 * (size_t)world; }
  int64_t* blockOff() const { return p; }         // [world]
  int64_t* records() const { return p + world; }  // [world]
};

// ---- the pinned count readback (xHost) ----
struct Readback {
  unsigned long long* p;
  int world;
  static size_t words(int world) { return 3 * (size_t)world + 4; }
  unsigned long long* records() const { return p; }             // [world] edge records per destination (XCnt::counts)
  unsigned long long& entries() const { return p[world]; }      // list entries (XCnt::bump)
  unsigned long long& arenaIds() const { return p[world + 1]; } // arena ids used by this rank
  unsigned long long& error() const { return p[world + 2]; }    // device error word (low 32 bits)
  unsigned long long* push() const { return p + world + 3; }    // XpCnt::counts, countWords(world) words
  unsigned long long& pushRecords(int r) const { return push()[r]; }
  unsigned long long& pushSlots(int r) const { return push()[world + r]; }
  unsigned long long& pushOverflow() const { return p[3 * world + 3]; }  // Dev::pushOvf (low 32 bits)
};

// ---- one rank's row of the per-hop size vector (allgather_i64) ----
// The same view fills this rank's row and reads rank r's row of the gathered
// vector (SizeRow::of).
struct SizeRow {
  static constexpr int64_t kHeartbeat = 1, kLists = 2;  // flags(): gw rows travel / frontier lists travel
  int64_t* p;
  int world;
  static int count(int world) { return 6 + 3 * world; }
  static SizeRow of(std::vector<int64_t>& all, int world, int r) { return {all.data() + (size_t)r * count(world), world}; }
  int64_t& bcastBytes() const { return p[0]; }
  int64_t& entries() const { return p[1]; }
  int64_t& arenaIds() const { return p[2]; }
  int64_t& flags() const { return p[3]; }
  int64_t& records(int r) const { return p[4 + r]; }  // edge records to rank r
  int64_t& error() const { return p[4 + world]; }     // device error word: every rank stops on any rank's
  int64_t& dials() const { return p[5 + world]; }
  int64_t& pushRecords(int r) const { return p[6 + world + r]; }
  int64_t& pushSlots(int r) const { return p[6 + 2 * world + r]; }
  bool heartbeat() const { return (flags() & kHeartbeat) != 0; }
  bool lists() const { return (flags() & kLists) != 0; }
};

// ---- the broadcast chunk (all-gather, equal chunks) ----
// [node header][list entries][randomsub masks][arena ids][gw rows], every
// section 8-aligned.  k_x_lists always writes its entries behind a header of
// listHeaderBytes(nodes), whether or not the lists then travel.  When they do
// not (deferred lists, no push overflow: nothing was packed, `entries` is 0)
// no header travels either and the arena ids start the chunk; when they do,
// `ent` is where k_x_lists wrote.
inline size_t listHeaderBytes(int64_t nodes) { return align8((size_t)nodes * 8); }

struct Bcast {
  size_t ent, sel, arena, gw, total;  // section offsets (the header is at 0)
  bool masks() const { return arena != sel; }
  size_t gwBytes() const { return total - gw; }
};
inline Bcast bcastLayout(int64_t nodes, int64_t entries, int64_t ids, int W, bool lists, bool masksPresent, bool hb) {
  Bcast b;
  b.ent = lists ? listHeaderBytes(nodes) : 0;
  b.sel = b.ent + align8((size_t)entries * 4);
  b.arena = b.sel + ((lists && masksPresent) ? (size_t)entries * 8 : 0);
  b.gw = b.arena + align8((size_t)ids * 4);
  b.total = b.gw + (hb ? (size_t)nodes * W * 8 : 0);
  return b;
}
// Rank r's chunk as its size row describes it (`nodes` = part[r + 1] - part[r]).
inline Bcast bcastLayout(const SizeRow& a, int64_t nodes, int W, bool masksPresent) {
  return bcastLayout(nodes, a.entries(), a.arenaIds(), W, a.lists(), masksPresent, a.heartbeat());
}

// ---- block sizes (all-to-all-v, one block per destination rank) ----
inline int64_t recordBlockBytes(int64_t records) { return kXRecBytes * records; }
// [PRec x records][slots, 2 bytes each]
inline int64_t pushBlockBytes(int64_t records, int64_t slots) { return kPRecBytes * records + 2 * slots; }
// Slot index, in the receiver's ibx[cur], of the slot region of a push block
// landed `blockOff` bytes behind the `ownSlots` slots of its owned senders.
inline int64_t pushSlotBase(int64_t ownSlots, int64_t blockOff, int64_t records) {
  return ownSlots + (blockOff + kPRecBytes * records) / 2;
}

// ---- what this rank sends ----
struct SendPlan {
  std::vector<int64_t> rec, recOff, recBytes;  // per destination: edge records, first record (k_x_pack), block bytes
  std::vector<int64_t> pushRec, pushOff, pushBytes;  // per destination: push records, block byte offset, block bytes
  int64_t totRec = 0, pushTotal = 0;
  std::vector<int64_t> row;  // this rank's SizeRow
};
// `ids` is the readback's arena count clamped to the rank's segment; push
// counts are taken only when k_push ran (`xpush`).
inline SendPlan planSend(const Readback& c, bool xpush, const Bcast& b, int64_t ids, bool hb, bool lists, int64_t dials) {
  const int world = c.world;
  SendPlan s;
  s.rec.resize(world);
  s.recBytes.resize(world);
  s.pushRec.assign(world, 0);
  s.pushBytes.assign(world, 0);
  s.row.assign(SizeRow::count(world), 0);
  SizeRow m{s.row.data(), world};
  for (int r = 0; r < world; ++r) {
    m.records(r) = s.rec[r] = (int64_t)c.records()[r];
    s.recBytes[r] = recordBlockBytes(s.rec[r]);
    if (!xpush) continue;
    m.pushRecords(r) = s.pushRec[r] = (int64_t)c.pushRecords(r);
    m.pushSlots(r) = (int64_t)c.pushSlots(r);
    s.pushBytes[r] = pushBlockBytes(s.pushRec[r], m.pushSlots(r));
  }
  s.totRec = exclusivePrefix(s.rec, s.recOff);
  s.pushTotal = exclusivePrefix(s.pushBytes, s.pushOff);
  m.bcastBytes() = (int64_t)b.total;
  m.entries() = (int64_t)c.entries();
  m.arenaIds() = ids;
  m.flags() = (hb ? SizeRow::kHeartbeat : 0) | (lists ? SizeRow::kLists : 0);
  m.error() = (int32_t)c.error();
  m.dials() = dials;
  return s;
}

// ---- what this rank receives, from every rank's size row ----
struct RecvPlan {
  std::vector<int64_t> recBytes;                     // per source: edge record block bytes
  std::vector<int64_t> pushRec, pushOff, pushBytes;  // per source: push records, block byte offset, block bytes
  int64_t recTotal = 0, pushTotal = 0;
  int64_t chunk = 8;     // all-gather chunk: the largest broadcast part, 8-aligned, at least 8
  int64_t maxDials = 0;  // the dial all-gather's row length (0: none this hop)
};
inline RecvPlan planRecv(std::vector<int64_t>& all, int world, int rank, bool xpush) {
  RecvPlan p;
  p.recBytes.resize(world);
  p.pushRec.assign(world, 0);
  p.pushBytes.assign(world, 0);
  for (int r = 0; r < world; ++r) {
    const SizeRow a = SizeRow::of(all, world, r);
    p.recBytes[r] = recordBlockBytes(a.records(rank));
    p.recTotal += p.recBytes[r];
    p.chunk = std::max(p.chunk, a.bcastBytes());
    p.maxDials = std::max(p.maxDials, a.dials());
    if (!xpush) continue;
    p.pushRec[r] = a.pushRecords(rank);
    p.pushBytes[r] = pushBlockBytes(p.pushRec[r], a.pushSlots(rank));
  }
  p.chunk = (int64_t)align8((size_t)p.chunk);
  p.pushTotal = exclusivePrefix(p.pushBytes, p.pushOff);
  return p;
}

// ---- dials (allgather_i64 of maxDials words per rank) ----
// A dial is a node pair packed into one word; rows are padded with -1.
constexpr int64_t kNoDial = -1;
inline int64_t packDial(int a, int b) { return ((int64_t)a << 32) | (int64_t)(uint32_t)b; }
inline std::pair<int, int> unpackDial(int64_t x) { return {(int)(x >> 32), (int)(uint32_t)x}; }
inline std::vector<int64_t> packDials(const std::vector<std::pair<int, int>>& dials, int64_t maxDials) {
  std::vector<int64_t> row((size_t)maxDials, kNoDial);
  for (size_t i = 0; i < dials.size(); ++i) row[i] = packDial(dials[i].first, dials[i].second);
  return row;
}
inline std::vector<std::pair<int, int>> unpackDials(const std::vector<int64_t>& gathered) {
  std::vector<std::pair<int, int>> out;
  for (int64_t x : gathered)
    if (x >= 0) out.push_back(unpackDial(x));
  return out;
}

}  // namespace gsx
