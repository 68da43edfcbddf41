/* gs_mesh_reach.h — mesh reach: eager-push depth from chosen publishers, on the device.
 *
 * If host s published on topic t now, whom would eager push reach, and in how
 * many hops?  Mesh health (gs_mesh_health.h) does not say: eager push runs over
 * directed mesh edges, a one-sided edge carries messages, and a component says
 * nothing about depth.  The latency histograms (gs_latency.h) see only what was
 * published and mix push with IHAVE / IWANT repair.  With mesh reach on, a tick
 * is taken inside gs_step: tick k (k = 0, 1, ...) when gs_current_hop() becomes
 * (k + 1) * period_hops, at the end of that hop, after its other kernels and
 * after the other inspectors' ticks; it writes no engine state.  A tick reads
 * what gs_read_mesh and gs_read_fanout would return had gs_step returned there.
 *
 *   source      sources[k], k = 0 .. num_sources - 1: distinct host ids.  A
 *               source is a source whether or not it is included, joined to t,
 *               or a gossipsub host.
 *   eager edge  for topic t, a directed edge e = (u -> v) with bit t set in
 *               mesh[e] | fanout[e].  Fanout bits exist only where u is not
 *               joined to t, so the one rule covers an unjoined publisher's
 *               first hop and changes nothing else.
 *   target      for topic t, a member exactly as gs_mesh_health.h defines it
 *               (include[v] != 0, NULL: every node; a gossipsub host; joined to
 *               t by its subscription word after the GS_EV_JOIN / GS_EV_LEAVE
 *               events of the hops run so far), other than the source.
 *   relay       only hosts that hold the message relay it: the source and the
 *               reached targets.  A host with include == 0 is never reached, so
 *               it is a dead end (a Sybil that does not forward).
 *   depth       depth_k[v][t]: the breadth-first level of v from sources[k] over
 *               the eager edges of t through targets.  The search is
 *               level-synchronous, so this is the exact shortest depth.
 *
 * Not modelled: WithFloodPublish's first hop (the publisher's send to every
 * topic peer), direct peers, floodsub and randomsub peers on a mixed network
 * (they are no targets and, holding no mesh, relay to nobody), score gates
 * (graylist, publish threshold), and any change of the mesh while a message is
 * in flight.  Where none of these applies the depth is the first-delivery age
 * of a message published at the tick's hop.
 *
 * The row of a tick holds, per source k and topic t, GS_REACH_ROW_FIELDS int64
 *   [GS_REACH_REACHED]    targets reached
 *   [GS_REACH_UNREACHED]  targets not reached
 *   [GS_REACH_ECC]        the largest depth, exact (0 if nothing was reached)
 * and depth_hist[k][t][b], b = 0 .. GS_REACH_DEPTH_BINS - 1: the targets
 * reached at depth b.  Bin 0 stays 0, bins 1 .. 62 are exact, bin 63 holds every
 * depth >= 63.  All are integer sums and one max: a row is the same bit for bit
 * from run to run.
 *
 * The rows are kept in a ring of `ticks` slots: tick k is readable while
 * ticks_taken - ticks <= k < ticks_taken; an overwritten tick is GS_ESTATE, a
 * tick not yet taken GS_EINVAL.  With `depths` set the newest tick's per-host
 * table is readable too: uint8 [num_sources][N][T], 0 in the source's own row
 * (every t), min(depth, 254) for a reached target, 255 otherwise.
 *
 * A tick runs ceil(num_sources / 64) passes, each a breadth-first search from
 * up to 64 sources at once over two bit tables (uint64 [N][T], bit j: reached
 * from the pass's source j).  The host launches the levels in batches and reads
 * one flag per batch (one stream synchronise per batch); after num_nodes levels
 * the step fails with GS_EDEVICE ("mesh reach: levels did not end") rather than
 * going on.
 *
 * A partitioned engine (gs_set_partition with world > 1) is refused: the bit
 * tables would have to cross ranks every level.  With mesh reach off nothing is
 * allocated or launched and every read returns GS_ESTATE.  Product library
 * only.
 */
#ifndef GS_MESH_REACH_H
#define GS_MESH_REACH_H

#include <stdint.h>

#include "gossip_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GS_REACH_DEPTH_BINS 64
#define GS_REACH_MAX_SOURCES 256
enum { GS_REACH_REACHED = 0, GS_REACH_UNREACHED, GS_REACH_ECC, GS_REACH_ROW_FIELDS };
/* gs_read_mesh_reach_kernel_stats: the four kernels of a tick, then three
 * counts that have no time (their total_ms entry is 0) */
enum {
  GS_REACH_K_MEMBERS = 0, /* the members of every topic, once per tick */
  GS_REACH_K_INIT,        /* a pass's tables cleared, its sources' bits set */
  GS_REACH_K_LEVEL,       /* the levels (a launch that finds the level before it empty returns at once) */
  GS_REACH_K_FINISH,      /* a pass's UNREACHED */
  GS_REACH_ST_PASSES,     /* launches[]: passes run, summed over the ticks */
  GS_REACH_ST_LEVELS,     /* launches[]: levels that ran, summed over the passes */
  GS_REACH_ST_BYTES,      /* launches[]: bytes the kernels read and wrote, by the engine's own count */
  GS_REACH_NUM_STATS
};

typedef struct gs_mesh_reach_config {
  int64_t period_hops;    /* > 0 */
  int32_t ticks;          /* ring capacity in ticks, >= 1 */
  int32_t num_sources;    /* 1 .. GS_REACH_MAX_SOURCES */
  const int32_t* sources; /* [num_sources] distinct host ids */
  const uint8_t* include; /* [N] the hosts that can be targets, or NULL for all */
  int32_t depths;         /* keep the newest tick's depth table readable */
} gs_mesh_reach_config;

/* Before the first gs_step.  GS_ESTATE once the engine has started or on a
 * second call ("duplicate mesh reach inspector"); GS_EUNSUPPORTED when the
 * router is not gossipsub ("pubsub router is not gossipsub"; scoring is not
 * needed) or the engine is partitioned ("mesh reach: not on a partitioned
 * engine": from this call, or from a gs_set_partition with world > 1 that comes
 * after it); GS_EINVAL for period_hops <= 0, ticks < 1, num_sources outside
 * 1 .. GS_REACH_MAX_SOURCES, no sources, a source outside 0 .. N - 1 or one
 * given twice.  The tables (two uint64 [N][T], the ring, and with `depths` the
 * uint8 [num_sources][N][T]) are allocated at their exact sizes when the engine
 * starts (GS_ENOMEM from that call if they do not fit). */
int gs_set_mesh_reach(gs_engine* g, const gs_mesh_reach_config* cfg);
/* Ticks taken so far (GS_ESTATE, as a negative value, with mesh reach off). */
int64_t gs_mesh_reach_ticks(const gs_engine* g);
/* Tick `tick`: the hop at which it was taken ((tick + 1) * period_hops),
 * row[num_sources][num_topics][GS_REACH_ROW_FIELDS] and
 * depth_hist[num_sources][num_topics][GS_REACH_DEPTH_BINS].  Any of the three
 * may be NULL. */
int gs_read_mesh_reach_row(gs_engine* g, int64_t tick, int64_t* hop, int64_t* row, int64_t* depth_hist);
/* The newest tick and its depths[num_sources][num_nodes][num_topics];
 * GS_ESTATE unless `depths` was set, GS_EINVAL before the first tick. */
int gs_read_mesh_reach_depths(gs_engine* g, int64_t* tick, uint8_t* depths);
/* total_ms[GS_REACH_NUM_STATS] and launches[GS_REACH_NUM_STATS]: the kernels'
 * times since gs_set_profiling(1) and their launches, the passes, the levels
 * and the bytes moved (counted with profiling on or off, and zeroed by
 * gs_set_profiling).  Not among the GS_K_* of gs_read_kernel_stats. */
int gs_read_mesh_reach_kernel_stats(gs_engine* g, double* total_ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif
