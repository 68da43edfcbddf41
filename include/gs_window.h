/* gs_window.h — the message window sized per topic.
 *
 * The engine's seen set is a fixed window of message slots, a ring per topic.
 * By default every ring has gs_config.slots_per_topic slots and every topic
 * the policy's first-delivery age limit (3 heartbeats; HistoryLength +
 * HistoryGossip + 3 heartbeats with the adversarial model or churn).  Real
 * topic rates differ by orders of magnitude, and a sparsely subscribed topic
 * delivers much later than a dense one, so both can be set per topic:
 *   slots[t]         the ring of topic t: it must hold every message of t
 *                    published within retire_hops[t] hops (gs_publish refuses
 *                    with GS_ECAPACITY otherwise);
 *   max_age_hops[t]  a first delivery of a message of t later than this fails
 *                    the step (GS_ECAPACITY, "later than").
 * The limits that remain: the rings sum to at most 16384 slots, and every node
 * holds the whole window (a window per node over its own topics is DESIGN.md
 * §7).  With no call made nothing changes.  Product library only (the CPU
 * oracle has no window).
 */
#ifndef GS_WINDOW_H
#define GS_WINDOW_H

#include <stdint.h>

#include "gossip_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Before the first gs_publish and the first gs_step (GS_ESTATE after).
 * slots[t]: topic t's ring, a positive multiple of 64; NULL: cfg.slots_per_topic each.
 *   Sum over topics <= 16384 (GS_EUNSUPPORTED, in the words of the creation error).
 * max_age_hops[t] > 0: first deliveries of topic t are accepted up to that age, replacing
 *   the policy value for that topic (shorter or longer; 1..30000); 0 or NULL: the policy's. */
int gs_set_topic_windows(gs_engine* g, const int32_t* slots /*[T]*/, const int32_t* max_age_hops /*[T]*/);
/* What is in force, any time after creation (the policy's values where nothing was set);
 * each array may be NULL:
 * retire_hops[t] = max_age[t] + (HistoryLength + 2) * H for gossipsub, max_age[t] + 2 otherwise
 * (H = hops per heartbeat). */
int gs_read_topic_windows(const gs_engine* g, int32_t* slots, int32_t* max_age_hops, int32_t* retire_hops);

#ifdef __cplusplus
}
#endif
#endif
