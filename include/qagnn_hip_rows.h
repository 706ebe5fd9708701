/*
 * qagnn_hip_rows.h -- extension of qagnn_hip.h: the gradient of a TRAINABLE entity table on the fused input stage.  qagnn_hip.h, its
 * structs and its ABI number are unchanged by it; libqagnn_hip.so exports these symbols beside the others (qagnn_amd/_lib.py: EXPORTS_ROWS).
 *
 * The input stage gathers table rows by ridx [N] (qagnn_node_prep_f32: -1 on context-node rows and on ids outside the table) and projects
 * them with cpt_transform.  The table's gradient is the gather's transpose; concept ids repeat heavily (the choices of a question share
 * most concepts, every padded slot carries the same id), so it is reduced FIRST, in the DP <= 256 wide space, and projected SECOND:
 *
 *     dTable[r] = sum_{i : ridx[i] = r} (dpre[i] @ Wc) = ( sum_{i : ridx[i] = r} dpre[i] ) @ Wc
 *
 *   1. qagnn_row_groups           ridx -> the positions grouped by row id (order, seg), the distinct ids (uniq), their number U (count)
 *   2. qagnn_row_segment_sum_f32  G[u] = sum of dpre over group u                                    [U, DP]
 *   3. qagnn_gemm_nn_f32 ...      R = G @ Wc, the existing product                                   [U, in]
 *   4. qagnn_rows_scatter_f32     dTable[uniq[u]] = R[u] into a gradient zeroed by qagnn_zero_words  [table_rows, in]
 *
 * U is known on the device only: every array is sized by a CAPACITY the host knows, and the launches are shaped by it.  Nothing here
 * allocates or synchronises, so the chain is safe inside a stream capture; nothing uses floating-point atomics, so it gives the same
 * bits on every run.
 */
#ifndef QAGNN_HIP_ROWS_H
#define QAGNN_HIP_ROWS_H

#include "qagnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: this header's own version (the ABI number of qagnn_hip.h does not move with it) */
int qagnn_rows_version(void);

#define QAGNN_ROWS_MAX_N (1 << 20)      /* positions of one call */
#define QAGNN_ROWS_MAX_TABLE (1 << 26)  /* table rows: two 13-bit digits */
#define QAGNN_ROWS_CHUNK 64             /* positions of one chunk of a segment sum (one wave walks one chunk) */

/* int32 words of workspace qagnn_row_groups needs for N positions (0 where N is outside 1..QAGNN_ROWS_MAX_N) */
int64_t qagnn_row_groups_workspace_elems(int32_t N);

/* ridx int64 [N]: a position i is LIVE when 0 <= ridx[i] < table_rows.  Written, ALL of them in full (no output keeps a word of what it
 * held before):
 *   order  int32 [N]     the live positions sorted by (row id, position); -1 behind the first M = number of live positions
 *   seg    int32 [N + 1] seg[u] = where group u starts in `order`, u < U; seg[U] = M, and M behind it
 *   uniq   int64 [N]     the distinct live row ids, ascending; -1 behind the first U
 *   count  int32 [1]     U
 * A stable LSD radix sort in two 13-bit digits (per 1024-position block a histogram, block bases by a scan, a stable scatter by one
 * wave that ranks 64 positions at a time with ballots), then head flags and a scan.  The result is a pure function of ridx: the only
 * atomics are integer counters in LDS whose totals do not depend on their order.
 * workspace: ws_elems >= qagnn_row_groups_workspace_elems(N) int32 words, 16-byte aligned.
 * Admitted: 1 <= N <= QAGNN_ROWS_MAX_N, 1 <= table_rows <= QAGNN_ROWS_MAX_TABLE; anything else, a NULL pointer or a short workspace is
 * QAGNN_EINVAL before any launch, and no output is touched. */
int qagnn_row_groups(const int64_t* ridx, int32_t N, int64_t table_rows, int32_t* order, int32_t* seg, int64_t* uniq, int32_t* count,
                     int32_t* workspace, int64_t ws_elems, qagnn_stream_t stream);

/* floats of workspace qagnn_row_segment_sum_f32 needs (0 where N or cols is outside the admitted range) */
int64_t qagnn_row_segment_sum_workspace_elems(int32_t N, int32_t cols);

/* G[u] = sum_{j = seg[u]}^{seg[u + 1] - 1} X[order[j]] for u < min(U, g_rows), U = *count; rows U <= u < g_rows of G are written as zeros.
 *   X      N rows of cols floats, ldx floats apart;  order, seg, count: as qagnn_row_groups leaves them for N positions
 *   G      g_rows rows of cols floats, ldg floats apart (g_rows <= N: a caller that knows a smaller bound of U, such as the table's
 *          rows, need not carry N rows)
 * THE ORDER OF THE ADDITIONS IS FIXED.  A segment is cut into chunks of QAGNN_ROWS_CHUNK consecutive j, counted from ITS OWN start.
 * A chunk's partial is p = X[order[j0]], then p += X[order[j]] for j = j0 + 1, ... in ascending j: sequential fp32 additions.  A segment
 * of one chunk is that partial; a longer one is t = p_0, then t += p_k for k = 1, 2, ...  So a segment's bits depend on its own rows
 * and nothing else -- not on the launch, on the other segments or on the run -- and a row id that fills 30 000 positions is summed by
 * 470 waves, not by one.
 * ERROR BOUND against exact arithmetic on the fp32 inputs, per element of G[u], with u32 = 2^-24 and c = ceil(len / QAGNN_ROWS_CHUNK)
 * chunks in a segment of len positions:
 *       |G[u] - exact| <= (QAGNN_ROWS_CHUNK + c) * u32 * sum_j |X[order[j]]|
 *   (a value passes through at most QAGNN_ROWS_CHUNK - 1 additions inside its chunk and c - 1 additions of partials, each with a
 *   relative error of at most u32; the two extra units cover the second-order terms while (QAGNN_ROWS_CHUNK + c)^2 u32 <= 2, i.e. for
 *   segments of up to 360 000 positions; a longer one, up to QAGNN_ROWS_MAX_N, stays within 1.001 times the bound).
 * For the whole table gradient dTable[r] = G[u] @ Wc add the product's bound, 12 * 2^-23 * sum_k |G[u][k]| |Wc[k][.]|, and propagate the
 * bound above through |Wc|:
 *       |dTable[r][c] - exact| <= sum_k ((QAGNN_ROWS_CHUNK + c) u32 S[k] + 12 eps32 (1 + (QAGNN_ROWS_CHUNK + c) u32) S[k]) |Wc[k][c]|,
 *   S[k] = sum_j |X[order[j]][k]|, eps32 = 2^-23.
 * workspace: ws_elems >= qagnn_row_segment_sum_workspace_elems(N, cols) floats, 16-byte aligned (the partials of the long segments).
 * Admitted: 1 <= N <= QAGNN_ROWS_MAX_N, 1 <= g_rows <= N, cols % 4 == 0, 4 <= cols <= 256, ldx >= cols, ldg >= cols, both pitches
 * multiples of 4 floats, X and G 16-byte aligned; anything else or a NULL pointer is QAGNN_EINVAL before any launch. */
int qagnn_row_segment_sum_f32(const float* X, int64_t ldx, int32_t cols, const int32_t* order, const int32_t* seg, const int32_t* count,
                              int32_t N, float* G, int64_t ldg, int32_t g_rows, float* workspace, int64_t ws_elems, qagnn_stream_t stream);

/* out[uniq[u]] = R[u] (accumulate == 0) or out[uniq[u]] += R[u] (accumulate != 0) for u < min(*count, n_rows), with 16-byte stores.  The
 * ids of uniq are distinct, so no two rows of R meet: no atomics.  No other word of `out` is touched; an id outside [0, table_rows) is
 * skipped.
 *   R      n_rows rows of cols floats, ldr floats apart;  uniq int64 [>= n_rows];  out: table_rows rows of cols floats, ldo floats apart
 * Admitted: 1 <= n_rows <= QAGNN_ROWS_MAX_N, table_rows >= 1, cols % 4 == 0, cols >= 4, ldr >= cols, ldo >= cols, both pitches multiples
 * of 4 floats, R and out 16-byte aligned; anything else or a NULL pointer is QAGNN_EINVAL before any launch. */
int qagnn_rows_scatter_f32(const float* R, int64_t ldr, int32_t cols, const int64_t* uniq, const int32_t* count, int32_t n_rows, float* out,
                           int64_t ldo, int64_t table_rows, int32_t accumulate, qagnn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
