/*
 * qagnn_hip_defer.h -- extension of qagnn_hip.h: the backward of a k-hop stack with the reductions nothing inside the stack reads
 * finished ONCE, after its last hop.  qagnn_hip.h, its structs and its ABI number are unchanged by it; libqagnn_hip.so exports these
 * symbols beside the others (qagnn_amd/_lib.py: EXPORTS_DEFER).
 *
 * Two gradients of every hop are read only after the whole stack has returned: dEkEm (the class table's gradient feeds the shared edge
 * encoder's backward) and db1 (a parameter gradient).  qagnn_hop_bwd_f32 and qagnn_stack_bwd_f32 finish both inside each hop, on the
 * chain of launches the next hop waits for.  The deferred form leaves each hop's partial sums in a region of their own and reduces all
 * k layers with one launch pair for dEkEm and one launch for db1, behind the last hop.  Every sum keeps the order of additions of the
 * per-hop form: the results are bit-identical to qagnn_stack_bwd_f32, run to run and against k calls of qagnn_hop_bwd_f32.
 *
 * No allocation, no synchronisation, no memset and no stream fork of its own: safe inside a stream capture.  The new launches go on
 * `stream`, before it joins the hops' side stream.
 */
#ifndef QAGNN_HIP_DEFER_H
#define QAGNN_HIP_DEFER_H

#include "qagnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: this header's own version (the ABI number of qagnn_hip.h does not move with it) */
int qagnn_defer_version(void);

/* Floats of the deferral workspace of a k-hop stack: per layer the class partials of the edge backward (cls_part_rows x 2 DP, as
 * qagnn_edge_attn_bwd_f32's cls_part; cls_part_rows = g->max_chunks + QAGNN_CLS_SLICES * g->C) and the column partials of db1. */
int64_t qagnn_stack_bwd_defer_elems(int32_t N, int32_t DP, int32_t cls_part_rows, int32_t k);

#define QAGNN_DEFER_MAX_HOPS 16 /* layers one deferred launch covers (the pointer table of its kernel arguments) */

/* qagnn_stack_bwd_f32 with the deferral.  defer_ws: 16-byte aligned, at least qagnn_stack_bwd_defer_elems(...) floats, written and read
 * by this call only (nothing in it survives the call, nothing in it needs to be initialised).  The hops' own workspace is used as before.
 * The k hops must share one graph, N, DP and HP, and k <= QAGNN_DEFER_MAX_HOPS: a stack that does not is refused (QAGNN_EUNSUPPORTED),
 * a workspace that is too small or misaligned likewise (QAGNN_EINVAL), both before anything is enqueued -- such a stack goes through
 * qagnn_stack_bwd_f32.  With defer_ws == NULL the call IS qagnn_stack_bwd_f32.
 *
 * The live classes the class reduction takes its blocks from lie in the graph's storage behind the live k-tiles of qagnn_hip_tn.h
 * (behind err: 16 words | n_live [4] | live_tiles, live_list [2 x roundup4(ceil(N / 32))] | n_live_cls [4] | live_cls [roundup4(C)]):
 * the classes with at least one edge in the batch, ascending, written by the graph preparation. */
int qagnn_stack_bwd_deferred_f32(const qagnn_hop_args* hops, int32_t k, float* defer_ws, int64_t defer_elems, qagnn_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* QAGNN_HIP_DEFER_H */
