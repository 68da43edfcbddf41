/* gs_inspect.h — WithPeerScoreInspect: score and mesh snapshots taken on the device.
 *
 * The reference hands the application every host's peer -> score map (or
 * peer -> PeerScoreSnapshot) once per period (score.go:120-175, 438-491).
 * Here a tick is taken inside gs_step, on the engine's stream, without a
 * stream synchronise: tick k (k = 0, 1, ...) when gs_current_hop() becomes
 * (k + 1) * period_hops, i.e. at the end of that hop, after its refresh, its
 * heartbeat and every other kernel of it.  A tick holds, by definition, what
 * gs_read_scores, gs_read_mesh, gs_read_topic_stats_edges and
 * gs_read_behaviour_penalty would return had gs_step returned there:
 *
 *   score_hist[j]   this rank's owned edges whose score s satisfies
 *                   bounds[j-1] <= s < bounds[j] (numpy's searchsorted(bounds,
 *                   s, side="right"): a score equal to a bound goes to the
 *                   upper bin).  An edge without a score record (a connection
 *                   that is down and not retained, or dormant) and an edge of
 *                   a floodsub / randomsub host of a mixed network count as
 *                   0.  The row sums to the owned edges.
 *   mesh_deg[t][d]  this rank's owned nodes whose mesh for topic t holds d
 *                   peers (unsubscribed and non-gossipsub hosts: d = 0).
 *                   Each topic's row sums to the owned nodes; the ranks' rows
 *                   add up to the whole graph's.
 *   sampled edges   the out-edges of this rank's owned nodes in node_mask, in
 *                   ascending edge id: their exact scores, and with `extended`
 *                   the PeerScoreSnapshot fields — AppSpecificScore,
 *                   IPColocationFactor (the value score() multiplies by the
 *                   weight), BehaviourPenalty, and per topic TimeInMesh (0
 *                   unless the pair is in the mesh, score.go:477-479),
 *                   FirstMessageDeliveries, MeshMessageDeliveries and
 *                   InvalidMessageDeliveries.  An edge without a record reads
 *                   0 in every field (the reference's map has no entry).
 *
 * The rows are kept in a ring of `ticks` slots: tick k is readable while
 * ticks_taken - ticks <= k < ticks_taken; an overwritten tick is GS_ESTATE, a
 * tick not yet taken GS_EINVAL.  All counts are integer sums, so a row is the
 * same bit for bit whatever the order of the adds.  With inspection off
 * nothing is allocated or launched and every read returns GS_ESTATE.
 * Product library only.
 */
#ifndef GS_INSPECT_H
#define GS_INSPECT_H

#include <stdint.h>

#include "gossip_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GS_INSPECT_MAX_BOUNDS 63
#define GS_INSPECT_DEG_BINS 65 /* mesh degree 0..64 */

typedef struct gs_inspect_config {
  int64_t period_hops;      /* > 0 */
  int32_t ticks;            /* ring capacity in ticks, >= 1 */
  int32_t num_bounds;       /* 0..GS_INSPECT_MAX_BOUNDS */
  const double* bounds;     /* finite, strictly ascending */
  const uint8_t* node_mask; /* [N] observers whose peers are snapshotted, or NULL */
  int32_t extended;         /* 0: Score only; 1: the PeerScoreSnapshot fields too */
} gs_inspect_config;

/* Before the first gs_step.  GS_ESTATE once the engine has started or on a
 * second call ("duplicate peer score inspector"); GS_EUNSUPPORTED when the
 * router is not gossipsub ("pubsub router is not gossipsub") or scoring is
 * off ("peer scoring is not enabled"); GS_EINVAL for period_hops <= 0,
 * ticks < 1, num_bounds out of range, or bounds that are not finite or not
 * strictly ascending.  The ring is allocated when the engine starts
 * (GS_ENOMEM from that call if it cannot be). */
int gs_set_score_inspect(gs_engine* g, const gs_inspect_config* cfg);
/* Ticks taken so far (GS_ESTATE, as a negative value, with inspection off). */
int64_t gs_inspect_ticks(const gs_engine* g);
/* The sampled edges of this rank: their number, and their ids (cap >= n). */
int gs_inspect_num_edges(const gs_engine* g, int64_t* n);
int gs_inspect_edges(gs_engine* g, int64_t* edges, int64_t cap);
/* Tick `tick`: the hop at which it was taken ((tick + 1) * period_hops),
 * score_hist[num_bounds + 1] and mesh_deg[num_topics][GS_INSPECT_DEG_BINS].
 * Any of the three may be NULL. */
int gs_read_inspect_row(gs_engine* g, int64_t tick, int64_t* hop, int64_t* score_hist, int64_t* mesh_deg);
/* score[nS] of the sampled edges at tick `tick`. */
int gs_read_inspect_scores(gs_engine* g, int64_t tick, double* score);
/* The extended fields at tick `tick` ([nS] and [nS][num_topics]); GS_ESTATE
 * unless `extended` was set. */
int gs_read_inspect_snapshot(gs_engine* g, int64_t tick, double* app, double* ip_colocation,
                             double* behaviour_penalty, int64_t* time_in_mesh, double* fmd, double* mmd,
                             double* imd);
/* A profiling aid: with gs_set_profiling(1), total_ms[3] and launches[3] of
 * the score pass, the reduction and the gather since then (not among the
 * GS_K_* of gs_read_kernel_stats). */
int gs_read_inspect_kernel_stats(gs_engine* g, double* total_ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif
