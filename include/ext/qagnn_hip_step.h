/*
 * qagnn_hip_step.h -- extension of qagnn_hip.h: the tail of a CAPTURED training step -- the accumulation of a mini-batch's gradient into
 * its window and the RAdam update -- as launches a hipGraph may replay.  qagnn_hip.h, its structs and its ABI number are unchanged by it;
 * libqagnn_hip.so exports these symbols beside the others (qagnn_amd/_step.py binds them on a handle of its own).
 *
 * WHERE THIS FILE LIVES.  The inventory of the headers directly in include/ (8 files, 93 prototypes) is pinned by the binding's tests, so this header waits
 * in include/ext/, which the binding generator does not glob; it moves up into include/ when that inventory is next revised.  It is read
 * by the same parser (qagnn_amd/_abi.py: header(path)) and is written in the same subset of C99.
 *
 * Why records.  A replayed launch repeats the arguments it was captured with.  qagnn_radam_step_scaled_f32 takes lr, step_size and the
 * branch as arguments: captured, it would repeat the first step's.  Here every tensor of a call names a RECORD in device memory, and the
 * kernel reads decay, s and mode (and the group's constants) from it:
 *
 *   1. qagnn_step_records_write     in FRONT of the replay, on its stream: the records' new values travel in this launch's own arguments
 *                                   (no memset / memcpy node, no host buffer a pending copy could still be reading), so a replay that is
 *                                   still pending keeps the values written in front of IT
 *   2. qagnn_window_accumulate_f32  inside the graph: window = first ? gradient : window + gradient
 *   3. qagnn_grad_norm_f32          inside the graph (qagnn_hip.h; workspace and out2 are static buffers)
 *   4. qagnn_radam_step_records_f32 inside the graph: the update, the clip coefficient applied as the gradient is read
 *
 * Nothing here allocates or synchronises; every buffer is the caller's.
 */
#ifndef QAGNN_HIP_STEP_H
#define QAGNN_HIP_STEP_H

#include "../qagnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: this header's own version (the ABI number of qagnn_hip.h does not move with it) */
int qagnn_step_version(void);

#define QAGNN_STEP_VERSION 1
#define QAGNN_STEP_RECORD_WORDS 12 /* 4-byte words of one record */

/* What one tensor's update reads instead of launch arguments.  The host derives every value in DOUBLE and rounds it to fp32 once, exactly as
 * qagnn_radam_step_scaled_f32 does from its double arguments:
 *   decay = (float)(-weight_decay * lr)    s = (float)(-step_size * lr)    mode: 2 rectified, 1 SGD-like, 0 moments only
 *   beta1, beta2, ob1 = (float)(1.0 - beta1), ob2 = (float)(1.0 - beta2), eps: constant per parameter group; kept here so that ONE launch
 *   sequence serves tensors of every group and every step count. */
typedef struct qagnn_step_record {
  float decay;
  float s;
  int32_t mode;
  int32_t pad;
  float beta1;
  float beta2;
  float ob1;
  float ob2;
  float eps;
  int32_t pad2[3];
} qagnn_step_record;

/* records[first + i] = values[i], i < n: `values` is HOST memory, read before the call returns (its words travel in the launches' arguments,
 * 64 records to a launch); `records` is device memory.  A mode outside 0..2, a NULL pointer or a negative range is QAGNN_EINVAL before any
 * launch. */
int qagnn_step_records_write(qagnn_step_record* records, int32_t first, int32_t n, const qagnn_step_record* values, qagnn_stream_t stream);

/* The update of qagnn_radam_step_scaled_f32 -- the same expressions, the same roundings, the same bits given the same fp32 scalars -- on
 * tensor i with the scalars of records[rec_index[i]].  p, g, m, v, numel, rec_index: HOST tables of n_tensors entries (the pointers in
 * them device memory), read before the call returns; records: n_records records in DEVICE memory, read when the kernels run.
 * grad_scale: NULL, or a device word every gradient is multiplied by as it is read (one rounding; the gradients are not written).
 * Admitted: 0 <= numel[i] < 2^31, 0 <= rec_index[i] < n_records; anything else or a NULL table is QAGNN_EINVAL before any launch. */
int qagnn_radam_step_records_f32(int32_t n_tensors, float* const* p, const float* const* g, float* const* m, float* const* v,
                                 const int64_t* numel, const int32_t* rec_index, const qagnn_step_record* records, int32_t n_records,
                                 const float* grad_scale, qagnn_stream_t stream);

/* dst[i][j] = *first ? src[i][j] : dst[i][j] + src[i][j].  first: a device word, read when the kernels run; non-zero is a SELECT of src --
 * dst is not read, so the inf or NaN of a stale window does not reach the new one.  One rounding per element: the bits of a copy, then of
 * an addition.  dst, src, numel: HOST tables of n_tensors entries.  Admitted: 0 <= numel[i] < 2^31; anything else or a NULL table or word
 * is QAGNN_EINVAL before any launch. */
int qagnn_window_accumulate_f32(int32_t n_tensors, float* const* dst, const float* const* src, const int64_t* numel, const int32_t* first,
                                qagnn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
