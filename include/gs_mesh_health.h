/* gs_mesh_health.h — mesh health: per-topic mesh components counted on the device.
 *
 * Is each topic's mesh still one piece, and who has been cut off?  A
 * mesh-degree histogram (gs_inspect.h) can look healthy while the mesh is
 * partitioned, and delivery counts hide a partition because IHAVE / IWANT
 * gossip repairs what the mesh fails to push.  With mesh health on, a tick is
 * taken inside gs_step: tick k (k = 0, 1, ...) when gs_current_hop() becomes
 * (k + 1) * period_hops, i.e. at the end of that hop, after its refresh, its
 * heartbeat and every other kernel of it (gs_inspect.h's convention; with both
 * inspectors on the order of the two ticks does not matter, neither writes
 * engine state).  A tick reads what gs_read_mesh would return had gs_step
 * returned there.  For topic t at a tick:
 *
 *   member       a node u with include[u] != 0 (NULL: every node), whose host
 *                speaks gossipsub (v1.0 or v1.1 on a mixed network,
 *                gs_set_routers), and that is joined to t at that moment: its
 *                own subscription word after the GS_EV_JOIN / GS_EV_LEAVE
 *                events of the hops run so far (a tick when the hop counter
 *                becomes k has processed the events scheduled for hops
 *                <= k - 1).
 *   mutual edge  a directed edge e = (u -> v) with u and v both members, bit t
 *                set in mesh[e] and bit t set in mesh[rev[e]].  Components are
 *                those of the undirected graph of the mutual edges over the
 *                members.
 *   label        the smallest node id in a node's component, so the result
 *                does not depend on the order of execution.
 *
 * The row of a tick holds, per topic, GS_MESH_ROW_FIELDS int64 counts
 *   [GS_MESH_MEMBERS]     members of t
 *   [GS_MESH_COMPONENTS]  components, singletons included
 *   [GS_MESH_LARGEST]     size of the largest component (0 without members)
 *   [GS_MESH_ISOLATED]    members without a mutual edge
 *   [GS_MESH_ONE_SIDED]   directed edges e = (u -> v) with u a member,
 *                         include[v], bit t in mesh[e] and not in mesh[rev[e]]
 *   [GS_MESH_OUTSIDE]     directed edges with u a member, bit t in mesh[e] and
 *                         include[v] == 0 (mesh slots held by excluded peers,
 *                         e.g. Sybils)
 *   [GS_MESH_ECLIPSED]    members whose mesh for t is not empty and holds only
 *                         peers with include == 0
 * and comp_hist[t][b], b = 0 .. GS_MESH_SIZE_BINS - 1: the components whose
 * size s has floor(log2 s) == b.  All are integer sums: a row is the same bit
 * for bit from run to run.
 *
 * The rows are kept in a ring of `ticks` slots: tick k is readable while
 * ticks_taken - ticks <= k < ticks_taken; an overwritten tick is GS_ESTATE, a
 * tick not yet taken GS_EINVAL.  With `labels` set the label table of the
 * newest tick only is readable too (int32 [N][T], -1 for a non-member).
 *
 * A tick iterates "label := the smallest label among the node and its mutual
 * neighbours, then the label's own label" until an iteration changes nothing.
 * The host launches the iterations in batches and reads one flag per batch
 * (one stream synchronise per batch); after num_nodes iterations without
 * convergence the step fails with GS_EDEVICE ("mesh health: labels did not
 * converge") rather than going on.
 *
 * A partitioned engine (gs_set_partition with world > 1) is refused: labels
 * would have to cross ranks every iteration.  With mesh health off nothing is
 * allocated or launched and every read returns GS_ESTATE.  Product library
 * only.
 */
#ifndef GS_MESH_HEALTH_H
#define GS_MESH_HEALTH_H

#include <stdint.h>

#include "gossip_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GS_MESH_SIZE_BINS 32
enum {
  GS_MESH_MEMBERS = 0, GS_MESH_COMPONENTS, GS_MESH_LARGEST, GS_MESH_ISOLATED, GS_MESH_ONE_SIDED,
  GS_MESH_OUTSIDE, GS_MESH_ECLIPSED, GS_MESH_ROW_FIELDS
};
/* gs_read_mesh_health_kernel_stats: the four passes of a tick, then two
 * counts that have no time (their total_ms entry is 0) */
enum {
  GS_MESH_K_INIT = 0,  /* members and their first labels */
  GS_MESH_K_LABEL,     /* the label iterations (a launch that finds the labels settled returns at once) */
  GS_MESH_K_SIZES,     /* component sizes */
  GS_MESH_K_ROW,       /* the row: components per root, edge counts per node */
  GS_MESH_ST_ITERS,    /* launches[]: label iterations that ran, summed over the ticks */
  GS_MESH_ST_BYTES,    /* launches[]: bytes the four passes read and wrote, by the engine's own count */
  GS_MESH_NUM_STATS
};

typedef struct gs_mesh_health_config {
  int64_t period_hops;    /* > 0 */
  int32_t ticks;          /* ring capacity in ticks, >= 1 */
  const uint8_t* include; /* [N] the hosts counted, or NULL for all */
  int32_t labels;         /* keep the newest tick's label table readable */
} gs_mesh_health_config;

/* Before the first gs_step.  GS_ESTATE once the engine has started or on a
 * second call ("duplicate mesh health inspector"); GS_EUNSUPPORTED when the
 * router is not gossipsub ("pubsub router is not gossipsub"; scoring is not
 * needed) or the engine is partitioned ("mesh health: not on a partitioned
 * engine": from this call, or from a gs_set_partition with world > 1 that
 * comes after it); GS_EINVAL for period_hops <= 0 or ticks < 1.  The tables
 * (two uint32 [N][T] and the ring) are allocated at their exact sizes when the
 * engine starts (GS_ENOMEM from that call if they do not fit). */
int gs_set_mesh_health(gs_engine* g, const gs_mesh_health_config* cfg);
/* Ticks taken so far (GS_ESTATE, as a negative value, with mesh health off). */
int64_t gs_mesh_health_ticks(const gs_engine* g);
/* Tick `tick`: the hop at which it was taken ((tick + 1) * period_hops),
 * row[num_topics][GS_MESH_ROW_FIELDS] and comp_hist[num_topics][GS_MESH_SIZE_BINS].
 * Any of the three may be NULL. */
int gs_read_mesh_health_row(gs_engine* g, int64_t tick, int64_t* hop, int64_t* row, int64_t* comp_hist);
/* The newest tick and its labels[num_nodes][num_topics]; GS_ESTATE unless
 * `labels` was set, GS_EINVAL before the first tick. */
int gs_read_mesh_labels(gs_engine* g, int64_t* tick, int32_t* labels);
/* total_ms[GS_MESH_NUM_STATS] and launches[GS_MESH_NUM_STATS]: the passes'
 * times since gs_set_profiling(1) and their launches, the label iterations and
 * the bytes moved (both counted with profiling on or off, and zeroed by
 * gs_set_profiling).  Not among the GS_K_* of gs_read_kernel_stats. */
int gs_read_mesh_health_kernel_stats(gs_engine* g, double* total_ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif
