// gs_window_layout.h — the message window's layout and its two horizons,
// stated once (include/gs_window.h, DESIGN.md §3 "Seen cache").  Plain host
// C++17, no HIP: the engine includes it, and so does the stand-alone check
// tests/topic_windows_check.cpp.
//
// The window is S slots = W 64-bit words.  Topic t owns the ring of slots[t]
// slots (a positive multiple of 64) that starts at word w0[t]; w0 is the
// exclusive prefix of slots[] / 64 with w0[T] = W.  The k-th message of topic
// t takes slot 64 * w0[t] + k % slots[t].  A first delivery of a message of
// topic t is accepted up to maxAge[t] hops after its publish, and the slot is
// taken again only retire[t] hops after it.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace gsw {

constexpr int kMaxWords = 256;    // W <= 64 lanes * 4 words (GS_MAX_WPL)
constexpr int kMaxSlots = 64 * kMaxWords;
constexpr int kMaxAgeHops = 30000;  // ages are 16-bit on the device (Dev::age)

// retire_hops of a topic whose first deliveries are accepted up to `age`:
// gossipsub keeps a message in mcache for HistoryLength heartbeats of H hops
// (+ 2: the shift that drops it, and the IWANT round trip); the other routers
// forward a message the hop after its delivery and never again.
inline int64_t retireHops(int64_t age, bool gossipsub, int historyLength, int H) {
  return gossipsub ? age + (int64_t)(historyLength + 2) * H : age + 2;
}

struct Layout {
  int T = 0, W = 0, S = 0;
  int maxSlots = 0;               // the largest topic's ring
  bool uniform = true;            // every ring the same size: topic of slot s = s / slots[0]
  std::vector<int32_t> slots;     // [T]
  std::vector<uint16_t> w0;       // [T + 1] first word of topic t
  std::vector<uint8_t> wTopic;    // [kMaxWords] topic of word w (past W: T - 1)

  int wordsOf(int t) const { return w0[(size_t)t + 1] - w0[(size_t)t]; }
  int maxWords() const { return maxSlots / 64; }
  int topicOfSlot(int s) const { return wTopic[(size_t)(s >> 6)]; }
  // slot of topic t's k-th message (k counts from 0)
  int slotOf(int t, int64_t k) const { return 64 * (int)w0[(size_t)t] + (int)(k % slots[(size_t)t]); }
};

// Why a set of rings cannot be laid out, or "" (T in 1..64 is the caller's).
// The last text is the engine's creation error, word for word.
inline std::string checkSlots(const int32_t* slots, int T) {
  int64_t sum = 0;
  for (int t = 0; t < T; ++t) {
    if (slots[t] <= 0 || slots[t] % 64 != 0) return "slots_per_topic must be a positive multiple of 64";
    sum += slots[t];
  }
  if (sum > kMaxSlots) return "num_topics * slots_per_topic must be <= 16384 in this build";
  return "";
}

// The layout of rings that passed checkSlots.
inline Layout makeLayout(const int32_t* slots, int T) {
  Layout L;
  L.T = T;
  L.slots.assign(slots, slots + T);
  L.w0.assign((size_t)T + 1, 0);
  L.wTopic.assign(kMaxWords, (uint8_t)(T - 1));
  for (int t = 0; t < T; ++t) {
    L.w0[(size_t)t + 1] = (uint16_t)(L.w0[(size_t)t] + slots[t] / 64);
    for (int w = L.w0[(size_t)t]; w < L.w0[(size_t)t + 1]; ++w) L.wTopic[(size_t)w] = (uint8_t)t;
    L.maxSlots = std::max(L.maxSlots, (int)slots[t]);
    if (slots[t] != slots[0]) L.uniform = false;
  }
  L.W = L.w0[(size_t)T];
  L.S = 64 * L.W;
  return L;
}
inline Layout uniformLayout(int T, int slotsPerTopic) {
  const std::vector<int32_t> s((size_t)T, slotsPerTopic);
  return makeLayout(s.data(), T);
}

// Why a set of age limits is refused, or "" (0 = the policy's value).
inline std::string checkAges(const int32_t* ages, int T) {
  for (int t = 0; t < T; ++t)
    if (ages[t] < 0 || ages[t] > kMaxAgeHops) return "max_age_hops must be 0 (the policy's) or 1..30000";
  return "";
}

// The publish guard: may a message of a topic published in hop `hop` take a
// slot whose previous message was published in hop `owner` (INT64_MIN: none)?
inline bool slotFree(int64_t owner, int64_t hop, int64_t retire) { return owner == INT64_MIN || hop - owner >= retire; }
// ... and the refusal's text.
inline std::string guardText(int t, int slots, int64_t retire, bool perTopic) {
  if (!perTopic)
    return "message window too small: more than slots_per_topic messages of one topic within " + std::to_string(retire) +
           " hops";
  return "message window too small: more than " + std::to_string(slots) + " messages of topic " + std::to_string(t) +
         " within " + std::to_string(retire) + " hops";
}

}  // namespace gsw
