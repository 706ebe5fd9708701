/*
 * qagnn_hip_dual.h -- extension of qagnn_hip.h: two NN products that share their A operand as ONE launch.  qagnn_hip.h, its structs
 * and its ABI number are unchanged by it; libqagnn_hip.so exports these symbols beside the others (qagnn_amd/_lib.py: EXPORTS_DUAL).
 *
 * A hop's backward ends with dX = dK|dM|dQ Wx (624 -> 208) and dS = dK|dM|dQ Ws (624 -> 112) over the same [N, 624] operand.  As two
 * launches each of them loads that operand and splits it into its fp16 pieces; here one block carries the 13 + 7 column tiles of both
 * outputs and pays for A once.  Per output tile the k-tiles, the three MFMAs, the operand scales and the order "product + old value"
 * are those of the separate launches: the results are bit-identical to two calls of qagnn_gemm_nn_split_ws_f32.
 */
#ifndef QAGNN_HIP_DUAL_H
#define QAGNN_HIP_DUAL_H

#include "qagnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: this header's own version (the ABI number of qagnn_hip.h does not move with it) */
int qagnn_dual_version(void);

/* C1 (+)= A B1 and C2 (+)= A B2 in one launch.  p1 / p2: the argument blocks of the two products as qagnn_gemm_nn_split_ws_f32 takes
 * them (each with its own C, ldc, No, accumulate); B1n / B2n: the weights as [No][K] (k contiguous) with pitches ldn1 / ldn2.
 * pack_ws / pack_bytes: 16-byte aligned scratch for the B images that are not registered (qagnn_gemm_nn_prepack_f32), may be NULL / 0.
 *
 * Returns QAGNN_EUNSUPPORTED -- and enqueues nothing, the caller then issues the two products on their own -- unless ALL of these hold:
 *   - both blocks have the same A1, lda1, K1, M and a_amax1, and a_amax1 is not NULL (the scaled three-MFMA form: pieces != 1);
 *   - K2 == 0 in both; no bias, no row table, no a_scale / a_shift, no colstat_part, no a_rowidx in either;
 *   - ceil(p1->No / 16) == 13 and ceil(p2->No / 16) == 7 (193..208 and 97..112 output columns);
 *   - each block alone is one the second-generation kernel takes (K1 a multiple of 8, operands below 2 GB);
 *   - M is at or above the row threshold of the packed forms (qagnn_packed_min_rows);
 *   - M is large enough that the separate products would keep their full 13 / 7 column tiles: ceil(M / 128) row tiles are at least 1.5
 *     per CU (49 152 rows on 256 CUs).  Below that the dispatcher narrows the separate products' column tiles to fill the chip, and the
 *     one launch -- a block is 128 rows x all 20 column tiles -- would be a few long serial blocks.  Mode 2 of qagnn_nn_dual_enable lifts this
 *     condition (tests at small row counts);
 *   - both two-piece images are at hand: registered, or packable into pack_ws without exceeding pack_bytes (the second image goes
 *     behind the first; a misaligned scratch counts as none).
 * Arguments that qagnn_gemm_nn_split_f32 would reject (null pointers, misaligned operands, pitches below widths) are QAGNN_EINVAL.
 * Timed as ONE entry of kind 0 (gemm_nn) by qagnn_timing_enable. */
int qagnn_gemm_nn_dual_f32(const qagnn_gemm_nn_args* p1, const float* B1n, int32_t ldn1, const qagnn_gemm_nn_args* p2, const float* B2n,
                           int32_t ldn2, void* pack_ws, int64_t pack_bytes, qagnn_stream_t stream);

/* Host only: would the call above take the one launch?  1 / 0; pointers are looked at for presence, equality and alignment only, so a
 * machine without a device can ask -- it counts 256 CUs then (B images count as registered when pack_ws is NULL and pack_bytes < 0). */
int qagnn_gemm_nn_dual_query(const qagnn_gemm_nn_args* p1, const float* B1n, int32_t ldn1, const qagnn_gemm_nn_args* p2, const float* B2n,
                             int32_t ldn2, const void* pack_ws, int64_t pack_bytes);

/* Launches of the two-output kernel since the library was loaded (by qagnn_gemm_nn_dual_f32 and by the hops' backward). */
int64_t qagnn_dual_launches(void);

/* Blocks of the two-output kernel the runtime places on one CU (its 80 KB of LDS per block: two fill a CU's 160 KB exactly, and the launch
 * is sized for two); 0 without a device.  tests/test_dual_product.py holds it to 2. */
int qagnn_dual_blocks_per_cu(void);

/* TESTS AND A/B RUNS ONLY: the process-wide mode of the two-output launch.  0: qagnn_hop_bwd_f32 / qagnn_stack_bwd*_f32 issue a hop's dX and
 * dS as two launches; 1 (the default): as the one launch where the conditions above hold; 2: likewise, and the row-tile condition is
 * lifted for the hops and for qagnn_gemm_nn_dual_f32 / _query alike.  The environment variable QAGNN_NN_DUAL (0 / 1 / 2, read once) sets
 * the starting value.  on < 0 reads; returns the previous value. */
int qagnn_nn_dual_enable(int32_t on);

#ifdef __cplusplus
}
#endif

#endif /* QAGNN_HIP_DUAL_H */
