/*
 * qagnn_hip_loss.h -- extension of qagnn_hip.h: the training losses of the multiple-choice head.  qagnn_hip.h, its structs and its ABI
 * number are unchanged by it; libqagnn_hip.so exports these symbols beside the others (qagnn_amd/_lib.py: EXPORTS_LOSS).
 *
 * The reference computes its loss with stock modules (qagnn.py:208-224): nn.CrossEntropyLoss on logits [Q, nc], or nn.MarginRankingLoss
 * on (correct, wrong) pairs it builds with boolean-mask indexing -- which synchronises the host and cannot be captured into a hipGraph.
 * Here the loss AND its gradient with respect to the logits leave ONE launch; the backward of the scalar is one more small launch.
 */
#ifndef QAGNN_HIP_LOSS_H
#define QAGNN_HIP_LOSS_H

#include "qagnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QAGNN_LOSS_CROSS_ENTROPY 0
#define QAGNN_LOSS_MARGIN_RANK 1

/* 1: this header's own version (the ABI number of qagnn_hip.h does not move with it) */
int qagnn_loss_version(void);

/* logits: Q rows of nc floats, ldl floats apart; labels int64 [Q]; w = *weight (a DEVICE word, so that a replayed graph reads each step's
 * weight from a static buffer), or 1 where weight == NULL.
 *
 *   QAGNN_LOSS_CROSS_ENTROPY   loss = w * mean_q (logsumexp_c x[q][c] - x[q][label_q]), the row maximum subtracted first
 *                              g[q][c] = w / Q * (softmax(x[q])[c] - [c == label_q])
 *   QAGNN_LOSS_MARGIN_RANK     loss = w / (Q (nc - 1)) * sum_q sum_{c != label_q} max(0, h),  h = -(x[q][label_q] - x[q][c]) + margin
 *                              (nn.MarginRankingLoss(margin, 'mean') on the pairs (correct, wrong) of every question; a mean does not
 *                              depend on the order of the pairs).  A pair is ACTIVE when h >= 0 -- torch's clamp_min subgradient: a pair
 *                              exactly on the kink has loss 0 and gradient -1 / +1.
 *                              g[q][c] = +w / (Q (nc - 1)) for an active wrong choice, g[q][label_q] = -(active pairs of q) * that
 *
 *   loss      device float[1], written
 *   g         Q rows of nc floats, ldg floats apart, written (d loss / d logits)
 *   stats     device double[2] or NULL:  stats[0] += (double)loss, stats[1] += 1, by one thread: launches on one stream accumulate in
 *             their order, bit for bit the sequential double sum of the fp32 losses
 *   flags     device int32[1] or NULL: set to 1 when a label lies outside [0, nc).  Such a row adds 0 to the loss and gets a zero
 *             gradient row, the denominators Q and Q (nc - 1) do not change, and no address is formed from the label.
 *
 * Non-finite logits behave as in torch: a NaN anywhere in a row, a +inf, or a row of -inf make the cross-entropy NaN; a -inf on a wrong
 * choice is a probability of 0; a NaN hinge argument makes the margin-rank loss NaN and is not active.
 * Deterministic: ONE workgroup of QAGNN_LOSS_THREADS threads, thread t takes questions t, t + T, ... in that order, the per-thread sums
 * are folded by a fixed tree; no atomics: the same bits on every run.  No allocation, no synchronisation: safe inside a stream capture.
 * Admitted: Q >= 1, ldl >= nc, ldg >= nc, 1 <= nc <= 1024 (cross-entropy), 2 <= nc <= 1024 (margin-rank); anything else, an unknown
 * kind or a NULL logits / labels / loss / g is QAGNN_EINVAL before a launch.
 *
 * ERROR BOUND against exact arithmetic on the fp32 inputs.  u = 2^-24 (unit roundoff of fp32), v = 2^-53, M = max(1, max |x|),
 * T = QAGNN_LOSS_THREADS, S = ceil(Q / T) + log2(T) + nc (the additions of the double-precision sums: a thread's questions, the tree,
 * a margin-rank row), L = ln(nc).
 *
 *   cross-entropy   |loss - exact| <= |w| M (u (nc + 8 + 5 L) + v S (2 + L))
 *       a row: the differences x - max (they enter exp: sum_c p_c |x_c - max| <= L), expf and logf to 1 ulp = 2 u each, the nc - 1 fp32
 *       additions of the exponentials, x[label] - max (<= 2 M), the last subtraction (<= 2 M + L): u (nc + 5 + 4 L) M; the rows are
 *       summed, weighted and divided in double and rounded once (2 + L); one more u for second-order terms
 *                   |g - exact|    <= |w| / Q * u (nc + 8 + L)
 *       p_c: exp of a rounded difference (p_c |x_c - max| <= 1 / e), expf, the sum as above, the division; the subtraction of the
 *       one-hot; w / Q rounded to fp32 and one multiplication
 *   margin-rank     |loss - exact| <= |w| M (3 u + v S) (2 + |margin| / M)
 *       h: two fp32 roundings of magnitudes <= 2 M + |margin|; pairs and rows are summed in double; one rounding of the result
 *                   |g - exact|    <= |w| / Q * 2 u      (the scale w / (Q (nc - 1)) rounded once, the label column's count times it)
 *       provided no pair's h changes sign under the two roundings above, i.e. |h| > 2 u (2 M + |margin|) or h == 0 exactly.
 * (qagnn_amd/_lib.py: choice_loss_bound evaluates these; tests/test_choice_loss.py holds the kernel to them against float64 torch.) */
#define QAGNN_LOSS_THREADS 256
int qagnn_choice_loss_f32(const float* logits, int64_t ldl, const int64_t* labels, int32_t Q, int32_t nc, int32_t kind, float margin,
                          const float* weight /* device [1] or NULL */, float* loss /* device [1] */, float* g, int64_t ldg,
                          double* stats /* device [2] or NULL */, int32_t* flags /* device [1] or NULL */, qagnn_stream_t stream);

/* dlogits[q][c] = g[q][c] * *grad_out: the upstream gradient of the scalar loss (a device float word) applied to what the forward kept.
 * dlogits: Q rows of nc floats, ldd floats apart; it may be g itself (then ldd == ldg).  Same admitted range of Q and nc (nc >= 1). */
int qagnn_choice_loss_bwd_f32(const float* g, int64_t ldg, const float* grad_out /* device [1] */, float* dlogits, int64_t ldd, int32_t Q,
                              int32_t nc, qagnn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
