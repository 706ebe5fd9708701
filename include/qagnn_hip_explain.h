/*
 * qagnn_hip_explain.h -- extension of qagnn_hip.h: the attention of an evaluated k-hop stack, handed out and traced from the context
 * node.  qagnn_hip.h, its structs and its ABI number are unchanged by it; libqagnn_hip.so exports these symbols beside the others
 * (qagnn_amd/_lib.py: EXPORTS_EXPLAIN).
 *
 * `a` below is what the hops leave in qagnn_hop_args.a: the per-source softmax of the edge scores BEFORE the out-degree scaling,
 * [Ep][4] floats in SOURCE order (position p of the graph's rowptr_s / eid_s arrays; the reference's `_alpha`, modeling_qagnn.py:472-473),
 * one such matrix per layer: layer l lies at a + l * layer_stride floats.  layer_stride >= 4 * g->Ep and layer_stride % 4 == 0; a is
 * 16-byte aligned (each row is read with one 16-byte load).  Only the first rowptr_s[N] rows of a layer are read: the count is taken
 * on the device, as the capacity forms of the graph require.
 *
 * Both entry points take the stream last, allocate nothing and synchronise nothing (safe inside a stream capture), and refuse a bad
 * argument with QAGNN_EINVAL and a message for the last-error call before anything is enqueued.
 */
#ifndef QAGNN_HIP_EXPLAIN_H
#define QAGNN_HIP_EXPLAIN_H

#include "qagnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QAGNN_TRACE_MAX_N 1024 /* node slots per subgraph: the pooling head's limit */

/* 1: this header's own version (the ABI number of qagnn_hip.h does not move with it) */
int qagnn_explain_version(void);

/* The attention in the caller's edge order, all k layers in ONE launch:
 *     out[l][g->eid_s[p]][h] = a[l][p][h]      for p < rowptr_s[N], h < 4, l < k
 * Edge ids are those of GATConvE.forward(return_attention_weights=True): the caller's edges first, then one self loop per node row.
 * eid_s is a permutation of [0, rowptr_s[N]): each such row of a layer of out is written exactly once, no row behind it is touched
 * (an id outside that range -- a corrupt graph -- is dropped, never stored through).
 * out: layer l at out + l * out_layer_stride floats, out_layer_stride >= 4 * g->Ep and % 4 == 0, 16-byte aligned.  k >= 0 (0: nothing
 * is launched). */
int qagnn_attn_export_f32(const qagnn_graph* g, const float* a, int64_t layer_stride, int32_t k, float* out, int64_t out_layer_stride,
                          qagnn_stream_t stream);

/* The attention followed out of the context node (node slot `root`) of every subgraph, over all k layers in ONE launch.  The graph is
 * B subgraphs of n consecutive node rows.  With abar_l[p] the attention of layer l at source-order position p -- the mean of the four
 * heads (head == -1: ((a0 + a1) + (a2 + a3)) / 4) or head `head` alone (0..3) -- and, for node t, its target-order segment
 * i in [rowptr_t[t], rowptr_t[t + 1]) with p = pos_t[i], s = src_t[i]:
 *     flow_0[v] = best_0[v] = 1 if v % n == root else 0
 *     flow_{l+1}[t] = sum_i abar_l[p] * flow_l[s]        the share of the context node's attention mass on t after l + 1 hops (the
 *                                                        softmax runs over the out-edges of a source, so each flow_l sums to 1 over
 *                                                        a subgraph)
 *     best_{l+1}[t] = max_i abar_l[p] * best_l[s]        the weight of the single heaviest (l + 1)-edge path from the context node to t
 *     pred_l[t]     = eid_s[p] of the FIRST i in segment order whose candidate is that maximum (the segment is ordered by edge id: the
 *                     lowest edge id among equals), -1 where best_{l+1}[t] == 0 (t not reachable in l + 1 hops)
 * The running maximum starts at 0 and a candidate c replaces it only if c > running (IEEE): equal candidates keep the earlier edge and
 * a NaN candidate never wins, so best holds no NaN.  In flow a NaN propagates as IEEE arithmetic gives it (0 * NaN = NaN), and only
 * inside its own subgraph.
 * flow, best: [k + 1][N] floats; pred: [k][N] int32.  k == 0 writes layer 0 of flow and best only (a and pred may then be NULL).
 *
 * One workgroup per subgraph, flow_l and best_l of the running layer in LDS; pull form over the target order: no floating-point
 * atomics, a summation order that depends on the graph alone (a segment of up to 64 edges is walked by 16 lanes, a longer one by a
 * wave, each lane in segment order, then a fixed butterfly) -- two calls give the same bits.
 * QAGNN_EINVAL unless g->block_n == n, g->N == B * n, 1 <= n <= QAGNN_TRACE_MAX_N, 0 <= root < n, -1 <= head <= 3, k >= 0.
 * A source outside its subgraph's block of rows (the graph's device flag err[1] is then set) is clamped into the block before it forms
 * an address; that subgraph's values are then unspecified -- the caller looks at the flag.
 *
 * Error against exact arithmetic on the same a, with m the largest in-degree (self loop included) and u = 2^-24; every term is
 * non-negative, so the bounds hold for any summation order:
 *     flow: relative error <= k * (m + 6) * u     (per layer: <= 2 roundings in the head mean, 1 in the product, m - 1 in the sum)
 *     best: relative error <= 6 * k * u           (per layer: the head mean and the product)
 * (a value that underflows to a subnormal is outside the relative bound: compare values below 1e-30 absolutely). */
int qagnn_attn_trace_f32(const qagnn_graph* g, const float* a, int64_t layer_stride, int32_t k, int32_t B, int32_t n, int32_t root,
                         int32_t head, float* flow, float* best, int32_t* pred, qagnn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
