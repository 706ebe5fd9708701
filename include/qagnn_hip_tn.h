/*
 * qagnn_hip_tn.h -- extension of qagnn_hip.h: the two-operand weight gradient [X | S]^T dK|dM|dQ balanced by the LIVE k-tiles of a
 * prepared graph.  qagnn_hip.h, its structs and its ABI number are unchanged by it; libqagnn_hip.so exports these symbols beside the others
 * (qagnn_amd/_lib.py: EXPORTS_TN).
 *
 * k-tile t = node rows [32 t, 32 t + 32) of a graph is LIVE if one of its rows has an out- or in-edge besides its self loop (rows past N
 * have none).  In a dead tile dK = dQ = 0 exactly (qagnn_edge_attn_bwd_f32), so the K and Q columns of that product skip it
 * (csrc/gemm_split.hip).  Graph preparation leaves, as pure functions of the two rowptr arrays, in the graph's storage directly behind
 * the 16 words of qagnn_graph.err, with T = ceil(N / 32):
 *   n_live      [4]             [0] = the number of live tiles
 *   live_tiles  [roundup4(T)]   1 = live, 0 = dead
 *   live_list   [roundup4(T)]   the live tiles in ascending order, then the dead ones in ascending order
 * (qagnn_graph_storage_elems counts them; the struct does not name them).
 */
#ifndef QAGNN_HIP_TN_H
#define QAGNN_HIP_TN_H

#include "qagnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* [A1 | A2]^T B as qagnn_gemm_tn_h2_f32 for a B = dK | dM | dQ whose R rows are the node rows of `g` (R == g->N, No = 3 x 208): where the dispatch runs the long
 * two-operand kernel (k_gemm_tn_ws), the K and Q column blocks walk only g's LIVE k-tiles and the chunk slots are divided so that every
 * block walks the same number of tiles (csrc/common.h: tn_work).  B's K and Q columns MUST be zero in every row of a dead tile -- the
 * backward of the edge attention guarantees it; what they hold there is not read.  g == NULL, a graph without dead tiles, or any product
 * the dispatch routes elsewhere: exactly qagnn_gemm_tn_h2_f32 / _h1_f32 / (pieces == 3, amax ignored) the six-MFMA form, bit for bit.
 * pieces: 3, 2 or 1. */
int qagnn_gemm_tn_graph_f32(const float* A1, int32_t lda1, int32_t Ka1, const float* A2, int32_t lda2, int32_t Ka2, const float* B, int32_t ldb,
                            float* C, int32_t ldc, int32_t R, int32_t No, const uint32_t* amax_a1, const uint32_t* amax_a2,
                            const uint32_t* amax_b, int32_t pieces, const qagnn_graph* g, float* workspace, qagnn_stream_t stream);
/* Host-only: the route the dispatch takes for the weight gradient [A1 | A2]^T B of these sizes (dense pitches, aligned operands, no
 * prologue).  out[0] = kernel family (0 k_gemm_tn, 1 k_gemm_tn_strip, 2 k_gemm_tn_split, 3 k_gemm_tn_ws, 4 two single products),
 * out[1] = rows per chunk, out[2] = chunks, out[3] = 1 if a graph's live tiles would be used (No, length and the switch below). */
int qagnn_gemm_tn_route_query(int32_t R, int32_t Ka1, int32_t Ka2, int32_t No, int32_t* h_out /* host [4] */);
/* TESTS: the work table of qagnn_gemm_tn_graph_f32 for S chunk slots per row block and chunks of chunk_tiles k-tiles (out[1] / 32 of the
 * query), written by the device function the kernels use: out = device int32 [4 + 5 S]: cK, cM, T, L, then per unit u (block order)
 * column block (0 K, 1 M, 2 Q) | 1 = list, 0 = range | first list position or first tile | tiles | partial tile in the workspace. */
int qagnn_tn_work_table(const qagnn_graph* g, int32_t S, int32_t chunk_tiles, int32_t* out, qagnn_stream_t stream);
/* TESTS AND A/B RUNS ONLY.  ONE PROCESS-WIDE SWITCH (as qagnn_packed_min_rows): 0 = the weight gradients ignore the graph's live tiles,
 * 1 (default) = use them; on < 0 only reads.  Returns the previous value. */
int qagnn_tn_live_tiles(int32_t on);

#ifdef __cplusplus
}
#endif
#endif
