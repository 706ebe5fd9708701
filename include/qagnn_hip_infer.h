/*
 * qagnn_hip_infer.h -- extension of qagnn_hip.h: the forward-only (evaluation) path.  qagnn_hip.h, its structs and its ABI number are
 * unchanged by it; libqagnn_hip.so exports these symbols beside the others (qagnn_amd/_lib.py: EXPORTS_INFER).
 *
 * An eval-mode forward normalises with BatchNorm's RUNNING statistics, draws no dropout mask and is followed by no backward.  The k-hop
 * stack of qagnn_hip.h keeps, per hop, everything a backward would read, and admits the three-MFMA GEMM form only with batch
 * statistics (the bound of relu(bn(h1)) it hands the second mlp product is derived from them).  Here nothing is kept -- the hops of a
 * stack may share one set of result buffers -- and the operand maximum of that product is taken from h1 itself, by one streaming pass.
 */
#ifndef QAGNN_HIP_INFER_H
#define QAGNN_HIP_INFER_H

#include "qagnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: this header's own version (the ABI number of qagnn_hip.h does not move with it) */
int qagnn_infer_version(void);

/* max over r < R, c < Cc of relu(scale[c] * H[r][c] + shift[c]), as the a_scale / a_shift prologue of qagnn_gemm_nn_args computes it (one
 * fused multiply-add, then the ReLU): the operand maximum a_amax1 of such a product, exactly.  The bit pattern is merged into *slot under
 * the contract of the plain maximum pass of qagnn_hip.h: the caller zeroes the word; integer max on the bit pattern (order-independent);
 * NaNs are skipped; +inf gives 0x7F800000; an input whose values are all <= 0 leaves the word as it was.
 * H: R rows of Cc floats, ldh floats apart; Cc % 4 == 0, ldh >= Cc, ldh % 4 == 0, H / scale / shift 16-byte aligned.  scale / shift [Cc]:
 * stats[3] / stats[4] as the BatchNorm bookkeeping kernels leave them (a column of ones is scale 0, shift 1 there: no special case).
 * scratch: device floats, the count the query below returns for (R, Cc); per-block partial maxima, folded by a second small launch. */
int64_t qagnn_bn_relu_absmax_scratch_elems(int32_t R, int32_t Cc);
int qagnn_bn_relu_absmax_f32(const float* H, int32_t ldh, int32_t R, int32_t Cc, const float* scale, const float* shift, uint32_t* slot,
                             float* scratch, qagnn_stream_t stream);

/* The k-hop forward with running statistics that keeps nothing: hops[l] as for the stack forward of qagnn_hip.h, with
 *   batch_stats == 0, run_mean_p / run_var_p set, run_mean == NULL (no buffer is updated) and p_drop == 0 in EVERY hop
 * -- anything else is QAGNN_EINVAL before the first enqueue.
 * The hops' result buffers may be shared: KMQ, a, alpha, aggr, h1, out and stats of all hops may be the same memory, and y may alternate
 * between two buffers.  Refused on the host: a hop one of whose result buffers (y included) overlaps its own X or S, anywhere in their
 * extents.  The amax blocks stay one per hop.  Workspace: that of the hop forward of qagnn_hip.h (the partial maxima of the extra pass use its last region).
 * The three-MFMA form is on in a hop when gemm_split >= 2, amax != NULL and N is at or above the packed-image row threshold -- the
 * training forward's condition without its batch-statistics term: the projection and the first mlp product then take it and words 0, 1, 2
 * and 4 of the block (AM_X, AM_S, AM_AGGR, AM_Y) are filled as in training.  At the widths where the training forward hands the second mlp
 * product a bound (192 < DP <= 208) that product takes the form too, and word 3 (AM_H1) is the TRUE maximum of relu(bn(h1)), left by one
 * bn_relu_absmax pass between the BatchNorm bookkeeping launch and the product.  With the form off the launches are exactly those of the
 * stack forward for the same arguments. */
int qagnn_stack_infer_f32(const qagnn_hop_args* hops, int32_t k, qagnn_stream_t stream);

/* Multiple-choice scoring on the device: logits [Q rows of nc floats, ldl floats apart], labels [Q] or NULL.
 *   pred[q]    = argmax_c logits[q][c]: the first index among equals, a NaN counts as the greatest (torch.argmax); pred may be NULL
 *   counts[0] += #{q : labels[q] == pred[q]}  (a label outside [0, nc) is never correct; labels == NULL: unchanged)
 *   counts[1] += Q
 * Integer atomics only: exact in any order.  1 <= nc <= 1024, ldl >= nc.  No synchronisation, no allocation: safe inside a stream
 * capture; the counters live on the device across batches and the host reads them once at the end. */
int qagnn_choice_eval_f32(const float* logits, int64_t ldl, const int64_t* labels, int32_t Q, int32_t nc, int64_t* pred,
                          int64_t* counts /* device [2] */, qagnn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
