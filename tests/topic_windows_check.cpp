// Stand-alone check of csrc/gs_window_layout.h (the message window per topic,
// include/gs_window.h): the prefix tables, slot -> topic -> slot for every slot
// of several layouts, the ring wrap per topic, the publish guard at each
// topic's own retire horizon and the argument checks, against the arithmetic
// written out here.  Host C++ only; tests/test_topic_windows.py builds it with
// AddressSanitizer and UBSan and runs it.  Prints "ok <checks>".
#include <cstdio>
#include <cstdlib>
#include <numeric>

#include "gs_window_layout.h"

static long checks = 0;
#define CHECK(c)                                                      \
  do {                                                                \
    ++checks;                                                         \
    if (!(c)) {                                                       \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);      \
      std::exit(1);                                                   \
    }                                                                 \
  } while (0)

static void checkLayout(const std::vector<int32_t>& slots) {
  const int T = (int)slots.size();
  CHECK(gsw::checkSlots(slots.data(), T).empty());
  const gsw::Layout L = gsw::makeLayout(slots.data(), T);
  const int S = std::accumulate(slots.begin(), slots.end(), 0);
  CHECK(L.T == T && L.S == S && L.W == S / 64 && L.W <= gsw::kMaxWords);
  CHECK((int)L.w0.size() == T + 1 && (int)L.wTopic.size() == gsw::kMaxWords);
  // the prefix tables
  int first = 0, largest = 0;
  bool same = true;
  for (int t = 0; t < T; ++t) {
    CHECK(L.w0[t] == first / 64 && L.wordsOf(t) == slots[t] / 64);
    first += slots[t];
    largest = std::max(largest, (int)slots[t]);
    same = same && slots[t] == slots[0];
  }
  CHECK(L.w0[T] == L.W && L.maxSlots == largest && L.maxWords() == largest / 64 && L.uniform == same);
  for (int w = L.W; w < gsw::kMaxWords; ++w) CHECK(L.wTopic[w] == T - 1);  // past the window: a valid topic
  // every slot: its topic owns it, and the topic's k-th message lands on it
  int s = 0;
  for (int t = 0; t < T; ++t)
    for (int k = 0; k < slots[t]; ++k, ++s) {
      CHECK(L.topicOfSlot(s) == t);
      CHECK(L.slotOf(t, k) == s);
      if (L.uniform) CHECK(s / slots[0] == t);  // the uniform layout's divide
    }
  CHECK(s == S);
  // ring wrap per topic: message k + n * slots[t] takes message k's slot and
  // never leaves the topic's words
  for (int t = 0; t < T; ++t)
    for (int64_t k : {(int64_t)0, (int64_t)1, (int64_t)slots[t] - 1, (int64_t)slots[t], (int64_t)slots[t] + 1,
                      (int64_t)3 * slots[t] - 1, (int64_t)1 << 40}) {
      const int slot = L.slotOf(t, k);
      CHECK(slot == 64 * L.w0[t] + (int)(k % slots[t]));
      CHECK(L.topicOfSlot(slot) == t && slot >= 64 * L.w0[t] && slot < 64 * L.w0[t + 1]);
      CHECK(L.slotOf(t, k + slots[t]) == slot);
    }
}

// A ring of slots[t] filled at one message per hop from hop 0: the message
// that wraps onto slot 0 is refused one hop short of the topic's own retire
// horizon and taken at it, whatever the other topics' horizons are.
static void checkGuard(const std::vector<int32_t>& slots, const std::vector<int32_t>& ages, bool gossipsub, int HL,
                       int H) {
  const int T = (int)slots.size();
  const gsw::Layout L = gsw::makeLayout(slots.data(), T);
  for (int t = 0; t < T; ++t) {
    const int64_t retire = gsw::retireHops(ages[t], gossipsub, HL, H);
    CHECK(retire == (gossipsub ? ages[t] + (int64_t)(HL + 2) * H : ages[t] + 2));
    std::vector<int64_t> owner((size_t)L.S, INT64_MIN);
    CHECK(gsw::slotFree(owner[L.slotOf(t, 0)], 7, retire));  // never used
    owner[L.slotOf(t, 0)] = 7;
    CHECK(!gsw::slotFree(owner[L.slotOf(t, slots[t])], 7, retire));
    CHECK(!gsw::slotFree(owner[L.slotOf(t, slots[t])], 7 + retire - 1, retire));
    CHECK(gsw::slotFree(owner[L.slotOf(t, slots[t])], 7 + retire, retire));
    CHECK(gsw::slotFree(owner[L.slotOf(t, slots[t])], 7 + retire + 1, retire));
    const std::string own = gsw::guardText(t, slots[t], retire, true), old = gsw::guardText(t, slots[t], retire, false);
    const std::string within = "within " + std::to_string(retire) + " hops";
    CHECK(own.find("message window too small") == 0 && own.find(within) != std::string::npos);
    CHECK(own.find("of topic " + std::to_string(t)) != std::string::npos);
    CHECK(old == "message window too small: more than slots_per_topic messages of one topic " + within);
  }
}

int main() {
  // uniform, one hot topic, alternating 64 and 192, 64 topics of 256, and a few more
  checkLayout(std::vector<int32_t>(1, 64));
  checkLayout(std::vector<int32_t>(1, 16384));
  checkLayout(std::vector<int32_t>(4, 128));
  checkLayout(std::vector<int32_t>(3, 320));
  checkLayout(std::vector<int32_t>(64, 256));
  checkLayout(std::vector<int32_t>(64, 64));
  {
    std::vector<int32_t> hot(64, 64);
    hot[0] = 2048;
    checkLayout(hot);
    hot[0] = 64;
    hot[63] = 12352;  // the last topic takes all that is left
    checkLayout(hot);
    std::vector<int32_t> alt(16);
    for (int t = 0; t < 16; ++t) alt[t] = t % 2 ? 192 : 64;
    checkLayout(alt);
    for (int t = 0; t < 16; ++t) alt[t] = t % 2 ? 64 : 192;
    checkLayout(alt);
    checkLayout({128, 128});
    checkLayout({64, 10048, 128});
  }
  CHECK(gsw::uniformLayout(64, 256).uniform && gsw::uniformLayout(64, 256).W == 256);
  CHECK(gsw::uniformLayout(3, 128).slotOf(2, 129) == 2 * 128 + 1);

  // the guard, per topic: gossipsub (HistoryLength 5, 10 hops per heartbeat:
  // ages 30 and 47 retire at 100 and 117), floodsub (age + 2)
  checkGuard({128, 128}, {30, 47}, true, 5, 10);
  checkGuard({64, 192, 64}, {1, 30000, 21}, true, 3, 7);
  checkGuard({64, 64}, {48, 3}, false, 5, 16);
  CHECK(gsw::retireHops(30, true, 5, 10) == 100 && gsw::retireHops(47, true, 5, 10) == 117);
  CHECK(gsw::retireHops(48, false, 5, 16) == 50);

  // the argument checks
  const std::string mult = "slots_per_topic must be a positive multiple of 64";
  const std::string sum = "num_topics * slots_per_topic must be <= 16384 in this build";
  for (int32_t bad : {0, -64, 1, 63, 65, 100, 16385}) {
    const int32_t s[2] = {64, bad};
    CHECK(gsw::checkSlots(s, 2) == mult);
  }
  {
    std::vector<int32_t> s(64, 256);
    CHECK(gsw::checkSlots(s.data(), 64).empty());
    s[17] = 320;
    CHECK(gsw::checkSlots(s.data(), 64) == sum);
    const int32_t one[1] = {16384 + 64};
    CHECK(gsw::checkSlots(one, 1) == sum);
    const int32_t big[2] = {INT32_MAX - 63, INT32_MAX - 63};  // (no overflow in the sum)
    CHECK(gsw::checkSlots(big, 2) == sum);
  }
  {
    const int32_t ok[4] = {0, 1, 47, 30000};
    CHECK(gsw::checkAges(ok, 4).empty());
    for (int32_t bad : {-1, 30001, INT32_MAX}) {
      const int32_t a[2] = {0, bad};
      CHECK(!gsw::checkAges(a, 2).empty());
    }
  }
  std::printf("ok %ld\n", checks);
  return 0;
}
