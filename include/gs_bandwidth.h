/* gs_bandwidth.h — bandwidth statistics counted on the device: who pays, and for what.
 *
 * gs_set_rpc_accounting keeps the cumulative RPC.Size() total and RPC count of
 * every directed edge; gs_read_rpc_bytes synchronises the stream, copies two
 * E-sized arrays and gives one undivided number per edge.  With the bandwidth
 * statistics on, the reduction is taken inside gs_step, on the engine's stream
 * and without a stream synchronise: tick k (k = 0, 1, ...) when
 * gs_current_hop() becomes (k + 1) * period_hops, i.e. at the end of that hop,
 * after its payload accounting and every other kernel of it (gs_inspect.h's
 * convention).  A tick holds, by definition, what gs_read_rpc_bytes would
 * return had gs_step returned there minus the same thing at the previous tick
 * (zero before tick 0: tick 0 contains the hello packets), reduced per node.
 *
 * Every node v has two directions in a period:
 *   egress   what v sent: the sum over its out-edges e.
 *   ingress  what its peers sent to v: the sum over the reverse edges rev[e].
 *            Counted when sent, as the accounting counts: an RPC in flight on
 *            a connection that closes is still ingress of its addressee.
 * and four byte classes:
 *   all       every RPC's Size() (the bytes of gs_read_rpc_bytes).
 *   eager     the RPCs of rpcWithMessages (gossipsub.go:1004, floodsub.go:
 *             81-99, randomsub.go:154): forwarded and locally published
 *             messages, one RPC each.
 *   pulled    the publish entries (gs_pb_field(msg_size[t]) each) of HandleRPC
 *             replies: messages served to an IWANT (gossipsub.go:674-711).  The
 *             reply's ControlMessage is not counted here.
 *   overhead  all - eager - pulled: every ControlMessage (IHAVE, IWANT, GRAFT,
 *             PRUNE with PX, the empty control of a reply, IWANT spam), every
 *             SubOpts announcement and every hello packet.
 * The number of RPCs is kept for `all` only.
 *
 * A tick's row holds, all integers (so it is the same bit for bit whatever the
 * order of the adds):
 *   total[c], total_rpcs  bytes per class and RPCs of the period, over all
 *                         nodes (the egress and the ingress totals are equal
 *                         by construction: one set is kept).
 *   hist[dir][c][j]       the nodes whose bytes x of class c in direction dir
 *                         satisfy bounds[j-1] <= x < bounds[j] (numpy's
 *                         searchsorted(bounds, x, side="right"): a value equal
 *                         to a bound goes to the upper bin; with bounds[0] = 1
 *                         bin 0 holds the silent nodes).  Each of the 8 rows
 *                         sums to the nodes.
 *   max[dir][c]           the largest per-node value, and argmax[dir][c] the
 *                         lowest node index that attains it (-1 when it is 0).
 *   sampled nodes         the nodes of node_mask in ascending index:
 *                         bytes[nS][dir][c] and rpcs[nS][dir].
 *
 * The rows are kept in a ring of `ticks` slots: tick k is readable while
 * ticks_taken - ticks <= k < ticks_taken; an overwritten tick is GS_ESTATE, a
 * tick not yet taken GS_EINVAL.  With the statistics off nothing is allocated
 * or launched and every read returns GS_ESTATE.  A partitioned engine
 * (gs_set_partition with world > 1) is refused: a rank does not hold the bytes
 * another rank's nodes sent over rev[e].  Product library only.
 */
#ifndef GS_BANDWIDTH_H
#define GS_BANDWIDTH_H

#include <stdint.h>

#include "gossip_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GS_BW_MAX_BOUNDS 63
enum { GS_BW_EGRESS = 0, GS_BW_INGRESS, GS_BW_DIRS };
enum { GS_BW_ALL = 0, GS_BW_EAGER, GS_BW_PULLED, GS_BW_OVERHEAD, GS_BW_CLASSES };
/* gs_read_bandwidth_kernel_stats: the three kernels of a tick */
enum {
  GS_BW_K_TICK = 0, /* the per-node sums, deltas, bins, totals and maxima */
  GS_BW_K_ARGMAX,   /* the lowest node index at each maximum */
  GS_BW_K_GATHER,   /* the sampled nodes' values into the ring slot */
  GS_BW_NUM_STATS
};

typedef struct gs_bandwidth_config {
  int64_t period_hops;      /* > 0 */
  int32_t ticks;            /* ring capacity in ticks, >= 1 */
  int32_t num_bounds;       /* 0..GS_BW_MAX_BOUNDS */
  const int64_t* bounds;    /* byte counts, positive and strictly ascending */
  const uint8_t* node_mask; /* [N] the sampled nodes, or NULL */
} gs_bandwidth_config;

/* Before the first gs_step and after gs_set_rpc_accounting.  GS_ESTATE once
 * the engine has started, on a second call ("duplicate bandwidth statistics")
 * or without the accounting ("bandwidth statistics: RPC accounting is off");
 * GS_EUNSUPPORTED on a partitioned engine ("bandwidth statistics: not on a
 * partitioned engine": from this call, or from a gs_set_partition with
 * world > 1 that comes after it); GS_EINVAL for period_hops <= 0, ticks < 1,
 * num_bounds out of range, or bounds that are not positive or not strictly
 * ascending.  The two per-edge counters, the per-node tables and the ring are
 * allocated when the engine starts (GS_ENOMEM from that call if they do not
 * fit). */
int gs_set_bandwidth_stats(gs_engine* g, const gs_bandwidth_config* cfg);
/* Ticks taken so far (GS_ESTATE, as a negative value, with the statistics off). */
int64_t gs_bandwidth_ticks(const gs_engine* g);
/* The sampled nodes: their number, and their indices ascending (cap >= n). */
int gs_bandwidth_num_nodes(const gs_engine* g, int64_t* n);
int gs_bandwidth_nodes(gs_engine* g, int32_t* nodes, int64_t cap);
/* Tick `tick`: the hop at which it was taken ((tick + 1) * period_hops),
 * total[GS_BW_CLASSES], total_rpcs[1], hist[GS_BW_DIRS][GS_BW_CLASSES][num_bounds + 1],
 * max[GS_BW_DIRS][GS_BW_CLASSES] and argmax[GS_BW_DIRS][GS_BW_CLASSES].  Any
 * of them may be NULL. */
int gs_read_bandwidth_row(gs_engine* g, int64_t tick, int64_t* hop, int64_t* total, int64_t* total_rpcs,
                          int64_t* hist, int64_t* max, int64_t* argmax);
/* bytes[nS][GS_BW_DIRS][GS_BW_CLASSES] and rpcs[nS][GS_BW_DIRS] of the sampled
 * nodes at tick `tick`.  Either may be NULL. */
int gs_read_bandwidth_nodes(gs_engine* g, int64_t tick, int64_t* bytes, int64_t* rpcs);
/* A profiling aid: with gs_set_profiling(1), total_ms[GS_BW_NUM_STATS] and
 * launches[GS_BW_NUM_STATS] of a tick's kernels since then (not among the
 * GS_K_* of gs_read_kernel_stats). */
int gs_read_bandwidth_kernel_stats(gs_engine* g, double* total_ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif
