/* gs_latency.h — propagation-latency histograms counted on the device.
 *
 * How many hops until a message reaches its subscribers: with the statistics
 * on, the engine counts every first delivery (what gs_counters.deliveries
 * counts: a host other than the author taking a valid message for the first
 * time; GS_BEHAVE_NO_FORWARD hosts included, rejected / ignored / throttled /
 * gated copies not) by its age
 *     a = delivery hop - publish hop,  1 <= a <= maxAge,
 * into two tables of bins = maxAge + 1 entries per row (index = age, bin 0
 * stays 0; a first delivery later than maxAge fails the step, so there is no
 * overflow bin; with per-topic age limits, gs_window.h, maxAge is the largest
 * topic's and a topic's bins past its own limit stay 0):
 *   per topic    hist[t][a], int64, since the start or the last reset;
 *   per message  mhist[a], uint32, of the message that owns its slot; readable
 *                while the slot is not recycled (the rule of
 *                gs_read_deliveries), zeroed when the slot gets a new owner.
 * Nothing of GS_FLAG_RECORD_DELIVERIES is needed.  A partitioned rank counts
 * its own nodes' deliveries; the ranks' tables add up to the whole graph's.
 * With the statistics off nothing is allocated or launched.  Product library
 * only (the CPU oracle reports per-message deliveries instead).
 */
#ifndef GS_LATENCY_H
#define GS_LATENCY_H

#include <stdint.h>

#include "gossip_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Before the first gs_step; GS_ESTATE after. */
int gs_set_latency_stats(gs_engine* g, int32_t on);
/* maxAge + 1 once the engine has started; GS_ESTATE before, or if off. */
int gs_latency_bins(const gs_engine* g);
/* hist[num_topics][bins]; bins must be gs_latency_bins() (GS_EINVAL). */
int gs_read_latency_hist(gs_engine* g, int64_t* hist, int32_t bins);
/* Zeroes the per-topic table only. */
int gs_reset_latency_stats(gs_engine* g);
/* hist[n][bins] of the messages ids[0..n): GS_EINVAL for an unknown id,
 * GS_ESTATE for a message whose slot was recycled, zeros for a message not
 * yet published. */
int gs_read_message_latency(gs_engine* g, int64_t n, const int64_t* ids, uint32_t* hist, int32_t bins);
/* A profiling aid, not part of the statistics: with gs_set_profiling(1),
 * total_ms[2] and launches[2] of the counting and the folding kernel since
 * then.  They are not among the GS_K_* of gs_read_kernel_stats, whose arrays
 * (GS_NUM_KERNELS entries, shared with the oracle) stay as they are;
 * scripts/latency_cdf.py reports the statistics' cost per hop from it. */
int gs_read_latency_kernel_stats(gs_engine* g, double* total_ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif
