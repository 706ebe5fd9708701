// The tail of the training step behind the backward pass: global-norm gradient clipping and the fused multi-tensor RAdam step, over the
// decoder's ~70 parameter tensors (2.85 M fp32).
//
// Reference: qagnn.py:267-278 -- clip_grad_norm_(model.parameters(), max_grad_norm) (torch: ~10 launches, one more read and write of every
// gradient), then utils/optimization_utils.py:31-97 -- a Python loop over every parameter, ~10 elementwise kernels each (~700 launches per
// optimiser step for the decoder).  Here all tensors of one call are walked by a handful of launches: the host packs up to MT_MAX_TENSORS
// tensor pointers and a block -> (tensor, chunk) map into the kernel ARGUMENT (no device-side table to keep in sync with the gradient
// tensors, which autograd re-allocates every step), apex-style.
//
// Clipping (qagnn_grad_norm_f32): k_sumsq_multi leaves ONE fp32 partial per 4096-element chunk in a caller-owned workspace slot -- 16
// sequential adds per thread, then an 8-level tree (wave_sum + two levels over the four waves); no atomics, so the same bits on every call --
// and k_norm_finish, one block, sums the partials in a fixed order in DOUBLE and writes  out[0] = total_norm,  out[1] = min(1, max_norm /
// (total_norm + 1e-6))  (torch.nn.utils.clip_grad_norm_'s formula; NaN / inf propagate as they do there).  The coefficient never visits the
// host: k_scale_multi applies it in place (g *= *scale), or the RAdam kernel multiplies g by it as it reads (grad_scale), in which case the
// clipped gradient is never written at all.
//
// RAdam, per element, exactly the reference's update:
//     v <- beta2 v + (1 - beta2) g g ;   m <- beta1 m + (1 - beta1) g                       (:57-58)
//     mode 2 (N_sma >= 5):  p <- p - wd lr p ;  p <- p - step_size lr  m / (sqrt(v) + eps)   (:83-87)
//     mode 1 (SGD-like)  :  p <- p - wd lr p ;  p <- p - step_size lr  m                     (:89-92)
//     mode 0             :  moments only (step_size < 0: degenerated_to_sgd = False and N_sma < 5)
// HBM-bound streaming: 4 reads + 3 writes of 4 bytes per element (the norm: 1 read; the in-place scale: 1 read + 1 write).
#include "common.h"
#include "../../include/ext/qagnn_hip_step.h"

namespace qagnn {

constexpr int MT_MAX_TENSORS = 24;
constexpr int MT_MAX_BLOCKS = 320;
constexpr int MT_CHUNK = 4096;  // elements per block
constexpr int MT_THREADS = 256;
constexpr int MT_PER_THREAD = MT_CHUNK / MT_THREADS;

struct block_map {  // block b of a pack's launch works on chunk block_chunk[b] of the pack's tensor block_tensor[b]
  int numel[MT_MAX_TENSORS];
  int block_chunk[MT_MAX_BLOCKS];
  unsigned char block_tensor[MT_MAX_BLOCKS];
};

struct radam_pack {
  float* p[MT_MAX_TENSORS];
  const float* g[MT_MAX_TENSORS];
  float* m[MT_MAX_TENSORS];
  float* v[MT_MAX_TENSORS];
  block_map map;
  float beta1, beta2, ob1, ob2, eps, decay, s;  // ob = 1 - beta, decay = -wd * lr, s = -step_size * lr: derived in DOUBLE on the host,
  int mode;                                     // like the reference's Python scalars (1 - 0.999 in fp32 is off by 1.3e-5 relative)
  const float* grad_scale;                      // SCALED only: the device word every gradient is multiplied by as it is read
};

// SCALED = false is the arithmetic of qagnn_radam_step_f32 since its first version: the gradient enters as it is stored
template <bool SCALED>
__global__ __launch_bounds__(MT_THREADS) void k_radam_multi(const radam_pack a) {
  const int t = a.map.block_tensor[blockIdx.x];
  const int base = a.map.block_chunk[blockIdx.x] * MT_CHUNK;
  const int n = min(a.map.numel[t] - base, MT_CHUNK);
  float* __restrict__ p = a.p[t] + base;
  const float* __restrict__ g = a.g[t] + base;
  float* __restrict__ m = a.m[t] + base;
  float* __restrict__ v = a.v[t] + base;
  const float ob1 = a.ob1, ob2 = a.ob2, decay = a.decay, s = a.s;
  float sc = 1.0f;
  if constexpr (SCALED) sc = a.grad_scale[0];
  for (int i = threadIdx.x; i < n; i += MT_THREADS) {
    float gi = g[i];
    if constexpr (SCALED) gi = __fmul_rn(gi, sc);  // one rounding, never contracted: the bits k_scale_multi would have stored
    // spelled out so that both instantiations round alike (left to the compiler, a b + c d contracts either way round): the products
    // v beta2, m beta1 and ob2 g are rounded, the second product of each sum is fused -- what this kernel has always computed
    const float vi = fmaf(__fmul_rn(ob2, gi), gi, __fmul_rn(v[i], a.beta2));
    const float mi = fmaf(ob1, gi, __fmul_rn(m[i], a.beta1));
    v[i] = vi;
    m[i] = mi;
    if (a.mode) {
      float pi = p[i];
      if (decay != 0.0f) pi += decay * pi;
      pi += a.mode == 2 ? s * (mi / (sqrtf(vi) + a.eps)) : s * mi;
      p[i] = pi;
    }
  }
}

struct sumsq_pack {
  const float* g[MT_MAX_TENSORS];
  block_map map;
  float* part;  // slot of the launch's block 0: the workspace advanced by the global chunk number of the pack's first chunk
};

// part[b] = sum of squares of the block's chunk.  Every thread adds its MT_PER_THREAD elements in order (a lane past the tail adds zeros:
// no lane leaves before wave_sum, which needs all 64), the wave totals are summed pairwise.
__global__ __launch_bounds__(MT_THREADS) void k_sumsq_multi(const sumsq_pack a) {
  __shared__ float red[MT_THREADS / 64];
  const int t = a.map.block_tensor[blockIdx.x];
  const int base = a.map.block_chunk[blockIdx.x] * MT_CHUNK;
  const int n = min(a.map.numel[t] - base, MT_CHUNK);
  const float* __restrict__ g = a.g[t] + base;
  float acc = 0.0f;
#pragma unroll
  for (int k = 0; k < MT_PER_THREAD; ++k) {
    const int i = threadIdx.x + k * MT_THREADS;
    const float x = i < n ? g[i] : 0.0f;
    acc += x * x;
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  static_assert(MT_THREADS == 256, "the pairwise sum below is written for four waves");
  if (threadIdx.x == 0) a.part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// one block: partials -> out[0] = sqrt(sum), out[1] = the clip coefficient.  Fixed order: thread t sums partials t, t + 256, ... in
// double, then a pairwise tree over the threads in LDS.
__global__ __launch_bounds__(MT_THREADS) void k_norm_finish(const float* __restrict__ part, int64_t n_part, double max_norm, float* __restrict__ out) {
  __shared__ double red[MT_THREADS];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n_part; i += MT_THREADS) acc += (double)part[i];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int w = MT_THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double total = sqrt(red[0]);
    const double coef = max_norm / (total + 1e-6);
    out[0] = (float)total;
    out[1] = (float)(coef > 1.0 ? 1.0 : coef);  // torch.clamp(coef, max = 1): a NaN stays a NaN
  }
}

struct scale_pack {
  float* g[MT_MAX_TENSORS];
  block_map map;
  const float* scale;
};

__global__ __launch_bounds__(MT_THREADS) void k_scale_multi(const scale_pack a) {
  const int t = a.map.block_tensor[blockIdx.x];
  const int base = a.map.block_chunk[blockIdx.x] * MT_CHUNK;
  const int n = min(a.map.numel[t] - base, MT_CHUNK);
  float* __restrict__ g = a.g[t] + base;
  const float sc = a.scale[0];
  for (int i = threadIdx.x; i < n; i += MT_THREADS) g[i] = __fmul_rn(g[i], sc);
}

// ---- the tail of a CAPTURED training step (include/ext/qagnn_hip_step.h; graphed.GraphedStep(optimizer=...)) ------------------------------
// A replayed launch repeats its arguments, so what changes from one optimiser step to the next -- lr, step_size, the branch -- cannot travel
// in them: every tensor of the call names a RECORD in device memory (rec[slot]), which a launch of k_step_records_write in front of the
// replay fills from ITS arguments.  The pointer tables stay in the argument: parameters, moments, window buffers and a capture's gradients
// have fixed addresses.
struct radam_rec_pack {
  float* p[MT_MAX_TENSORS];
  const float* g[MT_MAX_TENSORS];
  float* m[MT_MAX_TENSORS];
  float* v[MT_MAX_TENSORS];
  int rec[MT_MAX_TENSORS];  // the record of the slot's tensor
  block_map map;
  const qagnn_step_record* records;
  const float* grad_scale;  // SCALED only
};

// k_radam_multi with decay, s, mode (and the group's constants) read from the block's record: one uniform load per block, then the same
// expressions in the same spelling, so the same bits
template <bool SCALED>
__global__ __launch_bounds__(MT_THREADS) void k_radam_multi_rec(const radam_rec_pack a) {
  const int t = a.map.block_tensor[blockIdx.x];
  const int base = a.map.block_chunk[blockIdx.x] * MT_CHUNK;
  const int n = min(a.map.numel[t] - base, MT_CHUNK);
  float* __restrict__ p = a.p[t] + base;
  const float* __restrict__ g = a.g[t] + base;
  float* __restrict__ m = a.m[t] + base;
  float* __restrict__ v = a.v[t] + base;
  const qagnn_step_record r = a.records[a.rec[t]];
  const float ob1 = r.ob1, ob2 = r.ob2, decay = r.decay, s = r.s, beta1 = r.beta1, beta2 = r.beta2, eps = r.eps;
  const int mode = r.mode;
  float sc = 1.0f;
  if constexpr (SCALED) sc = a.grad_scale[0];
  for (int i = threadIdx.x; i < n; i += MT_THREADS) {
    float gi = g[i];
    if constexpr (SCALED) gi = __fmul_rn(gi, sc);
    const float vi = fmaf(__fmul_rn(ob2, gi), gi, __fmul_rn(v[i], beta2));
    const float mi = fmaf(ob1, gi, __fmul_rn(m[i], beta1));
    v[i] = vi;
    m[i] = mi;
    if (mode) {
      float pi = p[i];
      if (decay != 0.0f) pi += decay * pi;
      pi += mode == 2 ? s * (mi / (sqrtf(vi) + eps)) : s * mi;
      p[i] = pi;
    }
  }
}

struct accum_pack {
  float* dst[MT_MAX_TENSORS];
  const float* src[MT_MAX_TENSORS];
  block_map map;
  const int32_t* first;
};

// dst = *first ? src : dst + src.  A SELECT: what a stale window holds (inf, NaN) is not read into the first mini-batch of the next one
__global__ __launch_bounds__(MT_THREADS) void k_window_accumulate(const accum_pack a) {
  const int t = a.map.block_tensor[blockIdx.x];
  const int base = a.map.block_chunk[blockIdx.x] * MT_CHUNK;
  const int n = min(a.map.numel[t] - base, MT_CHUNK);
  float* __restrict__ dst = a.dst[t] + base;
  const float* __restrict__ src = a.src[t] + base;
  if (a.first[0]) {
    for (int i = threadIdx.x; i < n; i += MT_THREADS) dst[i] = src[i];
  } else {
    for (int i = threadIdx.x; i < n; i += MT_THREADS) dst[i] = dst[i] + src[i];
  }
}

constexpr int REC_PER_LAUNCH = 64;  // records of one k_step_records_write launch: 3 KiB of kernel argument

struct records_pack {
  qagnn_step_record r[REC_PER_LAUNCH];
  qagnn_step_record* out;
  int n;
};

__global__ __launch_bounds__(REC_PER_LAUNCH) void k_step_records_write(const records_pack a) {
  if ((int)threadIdx.x < a.n) a.out[threadIdx.x] = a.r[threadIdx.x];
}

static inline int64_t mt_chunks(int64_t numel) { return (numel + MT_CHUNK - 1) / MT_CHUNK; }

// Cuts tensors 0..n_tensors-1 into packs of at most MT_MAX_TENSORS tensor slots and MT_MAX_BLOCKS chunks (a tensor that does not fit is
// continued in the next pack).  open(slot, i): tensor i takes `slot` of the pack being filled;  launch(nb, first): the pack is full or the
// last one -- nb blocks, the first of which is chunk number `first` of the whole call (chunks counted over all tensors in order).
template <class Open, class Launch>
static int for_each_pack(int n_tensors, const int64_t* numel, block_map& map, Open open, Launch launch) {
  int nt = 0, nb = 0;
  int64_t first = 0;
  auto flush = [&]() -> int {
    const int rc = nb ? launch(nb, first) : QAGNN_OK;
    first += nb;
    nt = 0; nb = 0;
    return rc;
  };
  for (int i = 0; i < n_tensors; ++i) {
    const int chunks = (int)mt_chunks(numel[i]);
    int c = 0;
    while (c < chunks) {
      if (nt == MT_MAX_TENSORS || nb == MT_MAX_BLOCKS) {
        int rc = flush();
        if (rc != QAGNN_OK) return rc;
      }
      // (re-)open tensor i in the current pack
      const int slot = nt++;
      open(slot, i);
      map.numel[slot] = (int)numel[i];
      while (c < chunks && nb < MT_MAX_BLOCKS) {
        map.block_tensor[nb] = (unsigned char)slot;
        map.block_chunk[nb] = c++;
        ++nb;
      }
    }
  }
  return flush();
}

}  // namespace qagnn

using namespace qagnn;

extern "C" int qagnn_radam_step_scaled_f32(int32_t n_tensors, float* const* p, const float* const* g, float* const* m, float* const* v,
                                           const int64_t* numel, double beta1, double beta2, double eps, double lr, double weight_decay,
                                           double step_size, int32_t mode, const float* grad_scale, qagnn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  QAGNN_REQUIRE(n_tensors >= 0 && (n_tensors == 0 || (p && g && m && v && numel)), QAGNN_EINVAL, "radam_step: null table");
  QAGNN_REQUIRE(mode >= 0 && mode <= 2, QAGNN_EINVAL, "radam_step: mode %d", mode);
  for (int i = 0; i < n_tensors; ++i)
    QAGNN_REQUIRE(numel[i] >= 0 && numel[i] < (1ll << 31) && (numel[i] == 0 || (p[i] && g[i] && m[i] && v[i])), QAGNN_EINVAL,
                  "radam_step: tensor %d: null pointer or bad size", i);
  radam_pack a;
  a.beta1 = (float)beta1; a.beta2 = (float)beta2; a.ob1 = (float)(1.0 - beta1); a.ob2 = (float)(1.0 - beta2); a.eps = (float)eps;
  a.decay = (float)(-weight_decay * lr); a.s = (float)(-step_size * lr); a.mode = mode; a.grad_scale = grad_scale;
  return for_each_pack(
      n_tensors, numel, a.map, [&](int slot, int i) { a.p[slot] = p[i]; a.g[slot] = g[i]; a.m[slot] = m[i]; a.v[slot] = v[i]; },
      [&](int nb, int64_t) -> int {
        if (grad_scale) k_radam_multi<true><<<nb, MT_THREADS, 0, stream>>>(a);
        else k_radam_multi<false><<<nb, MT_THREADS, 0, stream>>>(a);
        QAGNN_LAUNCH_CHECK("k_radam_multi");
        return QAGNN_OK;
      });
}

extern "C" int qagnn_radam_step_f32(int32_t n_tensors, float* const* p, const float* const* g, float* const* m, float* const* v,
                                    const int64_t* numel, double beta1, double beta2, double eps, double lr, double weight_decay,
                                    double step_size, int32_t mode, qagnn_stream_t stream) {
  return qagnn_radam_step_scaled_f32(n_tensors, p, g, m, v, numel, beta1, beta2, eps, lr, weight_decay, step_size, mode, nullptr, stream);
}

// the table checks shared by the gradient-only entry points
static int check_grad_table(const char* what, int32_t n_tensors, const float* const* g, const int64_t* numel) {
  QAGNN_REQUIRE(n_tensors >= 0 && (n_tensors == 0 || (g && numel)), QAGNN_EINVAL, "%s: null table", what);
  for (int i = 0; i < n_tensors; ++i)
    QAGNN_REQUIRE(numel[i] >= 0 && numel[i] < (1ll << 31) && (numel[i] == 0 || g[i]), QAGNN_EINVAL, "%s: tensor %d: null pointer or bad size", what, i);
  return QAGNN_OK;
}

extern "C" int64_t qagnn_grad_norm_workspace_elems(int32_t n_tensors, const int64_t* numel) {
  int64_t total = 0;
  for (int i = 0; i < n_tensors; ++i) total += numel && numel[i] > 0 ? mt_chunks(numel[i]) : 0;
  return total > 0 ? total : 1;
}

extern "C" int qagnn_grad_norm_f32(int32_t n_tensors, const float* const* g, const int64_t* numel, double max_norm, float* workspace,
                                   float* out2, qagnn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  int rc = check_grad_table("grad_norm", n_tensors, g, numel);
  if (rc != QAGNN_OK) return rc;
  QAGNN_REQUIRE(workspace && out2, QAGNN_EINVAL, "grad_norm: null workspace or output");
  sumsq_pack a;
  int64_t n_part = 0;
  rc = for_each_pack(
      n_tensors, numel, a.map, [&](int slot, int i) { a.g[slot] = g[i]; },
      [&](int nb, int64_t first) -> int {
        a.part = workspace + first;
        k_sumsq_multi<<<nb, MT_THREADS, 0, stream>>>(a);
        QAGNN_LAUNCH_CHECK("k_sumsq_multi");
        n_part = first + nb;
        return QAGNN_OK;
      });
  if (rc != QAGNN_OK) return rc;
  k_norm_finish<<<1, MT_THREADS, 0, stream>>>(workspace, n_part, max_norm, out2);
  QAGNN_LAUNCH_CHECK("k_norm_finish");
  return QAGNN_OK;
}

extern "C" int qagnn_scale_multi_f32(int32_t n_tensors, float* const* g, const int64_t* numel, const float* scale, qagnn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  int rc = check_grad_table("scale_multi", n_tensors, g, numel);
  if (rc != QAGNN_OK) return rc;
  QAGNN_REQUIRE(scale, QAGNN_EINVAL, "scale_multi: null scale");
  scale_pack a;
  a.scale = scale;
  return for_each_pack(
      n_tensors, numel, a.map, [&](int slot, int i) { a.g[slot] = g[i]; },
      [&](int nb, int64_t) -> int {
        k_scale_multi<<<nb, MT_THREADS, 0, stream>>>(a);
        QAGNN_LAUNCH_CHECK("k_scale_multi");
        return QAGNN_OK;
      });
}

// ---- include/ext/qagnn_hip_step.h ---------------------------------------------------------------------------------------------------------
static_assert(sizeof(qagnn_step_record) == 48, "qagnn_step_record: twelve 4-byte words");

extern "C" int qagnn_step_version(void) { return 1; }

extern "C" int qagnn_step_records_write(qagnn_step_record* records, int32_t first, int32_t n, const qagnn_step_record* values,
                                        qagnn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  QAGNN_REQUIRE(first >= 0 && n >= 0 && (n == 0 || (records && values)), QAGNN_EINVAL, "step_records_write: null table or negative range");
  for (int i = 0; i < n; ++i)
    QAGNN_REQUIRE(values[i].mode >= 0 && values[i].mode <= 2, QAGNN_EINVAL, "step_records_write: record %d: mode %d", i, values[i].mode);
  records_pack a;
  for (int done = 0; done < n; done += REC_PER_LAUNCH) {
    a.n = n - done < REC_PER_LAUNCH ? n - done : REC_PER_LAUNCH;
    for (int i = 0; i < REC_PER_LAUNCH; ++i) a.r[i] = values[done + (i < a.n ? i : 0)];
    a.out = records + first + done;
    k_step_records_write<<<1, REC_PER_LAUNCH, 0, stream>>>(a);
    QAGNN_LAUNCH_CHECK("k_step_records_write");
  }
  return QAGNN_OK;
}

extern "C" int qagnn_radam_step_records_f32(int32_t n_tensors, float* const* p, const float* const* g, float* const* m, float* const* v,
                                            const int64_t* numel, const int32_t* rec_index, const qagnn_step_record* records,
                                            int32_t n_records, const float* grad_scale, qagnn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  QAGNN_REQUIRE(n_tensors >= 0 && (n_tensors == 0 || (p && g && m && v && numel && rec_index && records)), QAGNN_EINVAL,
                "radam_step_records: null table");
  for (int i = 0; i < n_tensors; ++i) {
    QAGNN_REQUIRE(numel[i] >= 0 && numel[i] < (1ll << 31) && (numel[i] == 0 || (p[i] && g[i] && m[i] && v[i])), QAGNN_EINVAL,
                  "radam_step_records: tensor %d: null pointer or bad size", i);
    QAGNN_REQUIRE(rec_index[i] >= 0 && rec_index[i] < n_records, QAGNN_EINVAL, "radam_step_records: tensor %d: record %d of %d", i, rec_index[i],
                  n_records);
  }
  radam_rec_pack a;
  a.records = records; a.grad_scale = grad_scale;
  return for_each_pack(
      n_tensors, numel, a.map,
      [&](int slot, int i) { a.p[slot] = p[i]; a.g[slot] = g[i]; a.m[slot] = m[i]; a.v[slot] = v[i]; a.rec[slot] = rec_index[i]; },
      [&](int nb, int64_t) -> int {
        if (grad_scale) k_radam_multi_rec<true><<<nb, MT_THREADS, 0, stream>>>(a);
        else k_radam_multi_rec<false><<<nb, MT_THREADS, 0, stream>>>(a);
        QAGNN_LAUNCH_CHECK("k_radam_multi_rec");
        return QAGNN_OK;
      });
}

extern "C" int qagnn_window_accumulate_f32(int32_t n_tensors, float* const* dst, const float* const* src, const int64_t* numel,
                                           const int32_t* first, qagnn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  QAGNN_REQUIRE(n_tensors >= 0 && (n_tensors == 0 || (dst && src && numel)), QAGNN_EINVAL, "window_accumulate: null table");
  QAGNN_REQUIRE(first, QAGNN_EINVAL, "window_accumulate: null first-of-window word");
  for (int i = 0; i < n_tensors; ++i)
    QAGNN_REQUIRE(numel[i] >= 0 && numel[i] < (1ll << 31) && (numel[i] == 0 || (dst[i] && src[i])), QAGNN_EINVAL,
                  "window_accumulate: tensor %d: null pointer or bad size", i);
  accum_pack a;
  a.first = first;
  return for_each_pack(
      n_tensors, numel, a.map, [&](int slot, int i) { a.dst[slot] = dst[i]; a.src[slot] = src[i]; },
      [&](int nb, int64_t) -> int {
        k_window_accumulate<<<nb, MT_THREADS, 0, stream>>>(a);
        QAGNN_LAUNCH_CHECK("k_window_accumulate");
        return QAGNN_OK;
      });
}
