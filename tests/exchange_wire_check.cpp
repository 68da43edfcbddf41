// Stand-alone check of csrc/gs_exchange_wire.h (tests/test_exchange_wire.py
// builds it with -fsanitize=address,undefined and runs it).  Every expected
// value is literal arithmetic: the index positions and size formulas the
// exchange used when both ends wrote them out by hand.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>

#include "gs_exchange_wire.h"

using namespace gsx;
using u64 = unsigned long long;

static long long checks = 0;
#define CHECK(c)                                             \
  do {                                                       \
    ++checks;                                                \
    if (!(c)) {                                              \
      std::printf("FAIL line %d: %s\n", __LINE__, #c);       \
      std::exit(1);                                          \
    }                                                        \
  } while (0)

static size_t up8(size_t x) { return (x + 7) / 8 * 8; }

static void positions(int w) {
  // size row
  std::vector<int64_t> row((size_t)SizeRow::count(w));
  CHECK(SizeRow::count(w) == 6 + 3 * w);
  const SizeRow m{row.data(), w};
  std::set<long> seen;
  auto at = [&](int64_t& f, long want) {
    CHECK(&f - row.data() == want);
    seen.insert(want);
  };
  at(m.bcastBytes(), 0);
  at(m.entries(), 1);
  at(m.arenaIds(), 2);
  at(m.flags(), 3);
  at(m.error(), 4 + w);
  at(m.dials(), 5 + w);
  for (int r = 0; r < w; ++r) {
    at(m.records(r), 4 + r);
    at(m.pushRecords(r), 6 + w + r);
    at(m.pushSlots(r), 6 + 2 * w + r);
  }
  CHECK((long)seen.size() == 6 + 3 * w && *seen.begin() == 0 && *seen.rbegin() == 6 + 3 * w - 1);
  CHECK(SizeRow::kHeartbeat == 1 && SizeRow::kLists == 2);
  for (int f = 0; f < 4; ++f) {
    m.flags() = f;
    CHECK(m.heartbeat() == ((f & 1) != 0) && m.lists() == ((f & 2) != 0));
  }
  std::vector<int64_t> all((size_t)(6 + 3 * w) * w);
  for (int r = 0; r < w; ++r) CHECK(SizeRow::of(all, w, r).p == all.data() + (size_t)r * (6 + 3 * w));
  // count readback
  CHECK(Readback::words(w) == (size_t)(3 * w + 4));
  std::vector<u64> host(Readback::words(w));
  const Readback c{host.data(), w};
  std::set<long> hs;
  auto hat = [&](u64& f, long want) {
    CHECK(&f - host.data() == want);
    hs.insert(want);
  };
  hat(c.entries(), w);
  hat(c.arenaIds(), w + 1);
  hat(c.error(), w + 2);
  hat(c.pushOverflow(), w + 3 + 2 * w);
  CHECK(c.push() == host.data() + w + 3);
  for (int r = 0; r < w; ++r) {
    hat(c.records()[r], r);
    hat(c.pushRecords(r), w + 3 + r);
    hat(c.pushSlots(r), w + 3 + w + r);
  }
  CHECK((long)hs.size() == 3 * w + 4);
  // device blocks
  std::vector<u64> dev(4 * (size_t)w + 1);
  const XCnt xc{dev.data(), w};
  CHECK(XCnt::words(w) == (size_t)(2 * w + 1));
  CHECK(xc.counts() == dev.data() && xc.cursors() == dev.data() + w && xc.bump() == dev.data() + 2 * w);
  const XpCnt xp{dev.data(), w};
  CHECK(XpCnt::words(w) == (size_t)(4 * w) && XpCnt::countWords(w) == (size_t)(2 * w));
  CHECK(xp.counts() == dev.data() && xp.cursors() == dev.data() + 2 * w);
  const XpOff xo{row.data(), w};
  CHECK(XpOff::words(w) == (size_t)(2 * w) && xo.blockOff() == row.data() && xo.records() == row.data() + w);
}

static void layout(int64_t nodes, int64_t ent, int64_t ids, int W, bool lists, bool masks, bool hb) {
  const Bcast b = bcastLayout(nodes, ent, ids, W, lists, masks, hb);
  const size_t hB = lists ? up8((size_t)nodes * 8) : 0, eB = up8((size_t)ent * 4);
  const size_t sB = (lists && masks) ? (size_t)ent * 8 : 0, pB = up8((size_t)ids * 4);
  const size_t gB = hb ? (size_t)nodes * W * 8 : 0;
  CHECK(b.ent == hB);
  CHECK(b.sel == hB + eB);
  CHECK(b.arena == hB + eB + sB);
  CHECK(b.gw == hB + eB + sB + pB);
  CHECK(b.total == hB + eB + sB + pB + gB);
  CHECK(b.masks() == (sB != 0) && b.gwBytes() == gB);
  CHECK(listHeaderBytes(nodes) == up8((size_t)nodes * 8));
  CHECK(b.ent % 8 == 0 && b.sel % 8 == 0 && b.arena % 8 == 0 && b.gw % 8 == 0 && b.total % 8 == 0);
  // each section holds its content before the next begins
  CHECK(b.ent >= (lists ? (size_t)nodes * 8 : 0));
  CHECK(b.sel - b.ent >= (size_t)ent * 4);
  CHECK(b.arena - b.sel >= sB);
  CHECK(b.gw - b.arena >= (size_t)ids * 4);
  CHECK(b.total - b.gw >= gB);
}

static void layouts() {
  std::mt19937_64 g(5);
  for (int it = 0; it < 400; ++it)
    layout((int64_t)(g() % 5000), (int64_t)(g() % 100000), (int64_t)(g() % 70000), 1 + (int)(g() % 256), g() & 1, g() & 1,
           g() & 1);
  for (int W : {1, 256})
    for (int f = 0; f < 8; ++f) {
      const bool lists = f & 1, masks = f & 2, hb = f & 4;
      layout(0, 0, 0, W, lists, masks, hb);     // a rank owning no nodes
      layout(0, 0, 7, W, lists, masks, hb);
      layout(13, 0, 5, W, lists, masks, hb);    // zero entries
      layout(13, 1, 1, W, lists, masks, hb);    // odd entry and id counts
      layout(14, 33, 0, W, lists, masks, hb);
      layout(1, 65535, 4097, W, lists, masks, hb);
    }
}

struct Rank {
  std::vector<u64> host;
  int64_t nodes, ids, dials;
  bool lists;
  Bcast b;
  SendPlan sp;
};

static void agreement(int w, uint64_t seed, bool xpush, bool masks, bool hb) {
  std::mt19937_64 g(seed);
  const int W = 1 + (int)(g() % 40);
  const int64_t own = (int64_t)(g() % 100000);
  std::vector<Rank> rk((size_t)w);
  std::vector<int64_t> all;
  for (int s = 0; s < w; ++s) {
    Rank& k = rk[s];
    k.host.assign(Readback::words(w), 0);
    const Readback c{k.host.data(), w};
    for (int r = 0; r < w; ++r) {
      c.records()[r] = r == s ? 0 : g() % 3000;
      c.pushRecords(r) = r == s ? 0 : g() % 2000;  // stale words when push is off: must not travel
      c.pushSlots(r) = 8 * (g() % 5000);
    }
    k.nodes = (int64_t)(g() % 300);
    k.lists = g() % 3 != 0;
    c.entries() = k.lists ? g() % 9000 : 0;
    k.ids = (int64_t)(g() % 4000);
    c.arenaIds() = (u64)k.ids + g() % 2;  // the engine clamps it to the segment: `ids` travels
    c.error() = s == 1 ? 0x80000003ull : (s == 2 ? 6 : 0);
    k.dials = (int64_t)(g() % 4);
    k.b = bcastLayout(k.nodes, (int64_t)c.entries(), k.ids, W, k.lists, masks, hb);
    k.sp = planSend(c, xpush, k.b, k.ids, hb, k.lists, k.dials);
    // the send plan and the row against the hand-written arithmetic
    const SendPlan& p = k.sp;
    const std::vector<int64_t>& m = p.row;
    CHECK((int)m.size() == 6 + 3 * w);
    CHECK(m[0] == (int64_t)k.b.total && m[1] == (int64_t)k.host[w] && m[2] == k.ids);
    CHECK(m[3] == ((hb ? 1 : 0) | (k.lists ? 2 : 0)));
    CHECK(m[4 + w] == (int32_t)k.host[w + 2] && m[5 + w] == k.dials);
    int64_t tot = 0, ptot = 0;
    for (int r = 0; r < w; ++r) {
      const int64_t pr = xpush ? (int64_t)k.host[w + 3 + r] : 0, ps = xpush ? (int64_t)k.host[w + 3 + w + r] : 0;
      CHECK(m[4 + r] == (int64_t)k.host[r] && m[6 + w + r] == pr && m[6 + 2 * w + r] == ps);
      CHECK(p.rec[r] == (int64_t)k.host[r] && p.recOff[r] == tot && p.recBytes[r] == 96 * p.rec[r]);
      CHECK(p.pushRec[r] == pr && p.pushOff[r] == ptot && p.pushBytes[r] == 16 * pr + 2 * ps);
      tot += p.rec[r];
      ptot += p.pushBytes[r];
    }
    CHECK(p.totRec == tot && p.pushTotal == ptot);
    all.insert(all.end(), m.begin(), m.end());
  }
  for (int r = 0; r < w; ++r) {
    const RecvPlan rp = planRecv(all, w, r, xpush);
    int64_t in = 0, pin = 0, big = 8, dmax = 0;
    for (int s = 0; s < w; ++s) {
      CHECK(rp.recBytes[s] == rk[s].sp.recBytes[r]);    // what r expects from s is what s sends to r
      CHECK(rp.pushBytes[s] == rk[s].sp.pushBytes[r]);
      CHECK(rp.pushRec[s] == rk[s].sp.pushRec[r] && rp.pushOff[s] == pin);
      CHECK(pushSlotBase(own, rp.pushOff[s], rp.pushRec[s]) == own + (pin + 16 * rp.pushRec[s]) / 2);
      in += rp.recBytes[s];
      pin += rp.pushBytes[s];
      big = std::max<int64_t>(big, (int64_t)rk[s].b.total);
      dmax = std::max(dmax, rk[s].dials);
      const Bcast b = bcastLayout(SizeRow::of(all, w, s), rk[s].nodes, W, masks);  // r's view of s's chunk
      const Bcast& o = rk[s].b;
      CHECK(b.ent == o.ent && b.sel == o.sel && b.arena == o.arena && b.gw == o.gw && b.total == o.total);
    }
    CHECK(rp.recTotal == in && rp.pushTotal == pin && rp.maxDials == dmax);
    CHECK(rp.chunk == (int64_t)up8((size_t)big) && rp.chunk >= 8);
  }
}

static void dials() {
  const int big = 2147483647;
  const int v[] = {0, 1, 7, 65536, big - 1, big};
  for (int a : v)
    for (int b : v) {
      const int64_t x = packDial(a, b);
      CHECK(x == (((int64_t)a << 32) | (int64_t)(uint32_t)b) && x >= 0);
      CHECK(unpackDial(x).first == a && unpackDial(x).second == b);
    }
  CHECK(kNoDial == -1);
  const std::vector<std::pair<int, int>> mine{{3, big}, {big - 1, 0}};
  std::vector<int64_t> row = packDials(mine, 4);
  CHECK(row.size() == 4 && row[0] == packDial(3, big) && row[1] == packDial(big - 1, 0) && row[2] == -1 && row[3] == -1);
  CHECK(packDials({}, 3) == std::vector<int64_t>(3, -1));
  std::vector<int64_t> gathered = packDials({}, 4);  // a rank without dials, then ours
  gathered.insert(gathered.end(), row.begin(), row.end());
  CHECK(unpackDials(gathered) == mine);
  CHECK(unpackDials(std::vector<int64_t>(5, -1)).empty());
}

int main() {
  CHECK(kXRecBytes == 96 && kPRecBytes == 16);
  CHECK(recordBlockBytes(7) == 96 * 7 && pushBlockBytes(5, 24) == 16 * 5 + 2 * 24);
  std::vector<int64_t> off;
  CHECK(exclusivePrefix({3, 0, 5}, off) == 8 && off == std::vector<int64_t>({0, 3, 3}));
  CHECK(exclusivePrefix({}, off) == 0 && off.empty());
  layouts();
  dials();
  uint64_t seed = 100;
  for (int w : {1, 2, 3, 8}) {
    positions(w);
    for (int f = 0; f < 8; ++f)
      for (int rep = 0; rep < 5; ++rep) agreement(w, ++seed, f & 1, f & 2, f & 4);
  }
  // nothing travels: the chunk is still 8 bytes
  std::vector<int64_t> none((size_t)SizeRow::count(2) * 2, 0);
  CHECK(planRecv(none, 2, 0, true).chunk == 8 && planRecv(none, 2, 1, false).pushTotal == 0);
  std::printf("ok %lld\n", checks);
  return 0;
}
