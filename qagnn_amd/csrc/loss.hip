// The training losses of the multiple-choice head: include/qagnn_hip_loss.h.  Loss and d loss / d logits in one launch.
#include "common.h"
#include "../../include/qagnn_hip_loss.h"

namespace qagnn {

// Q questions of nc logits are a few hundred floats at the reference's operating point (2 x 5) and 64 x 5 at bench size: next to anything
// else in the step the work is nothing and the launch is everything.  ONE workgroup; a thread owns whole questions (t, t + T, ...), walks
// a row three times (maximum, sum of exponentials, gradient) and keeps its questions' losses in a double; the T doubles are folded by a
// fixed tree in LDS.  No atomics, one order of additions: the same bits on every run, and the bound of the header has no term in Q but
// the double-precision one.  There is no second form at large nc: a row of 1024 is 4 KB read three times by one lane, still microseconds.
constexpr int CL_THREADS = 256;
static_assert(CL_THREADS == QAGNN_LOSS_THREADS, "the header's bound names the kernel's thread count");

// (-(xl - xc) + margin).clamp_min(0) as torch's margin_ranking_loss rounds it; a NaN passes through the clamp as it does there
__device__ __forceinline__ float hinge_arg(float xl, float xc, float margin) { return -(xl - xc) + margin; }

template <int KIND>
__global__ __launch_bounds__(CL_THREADS) void k_choice_loss(const float* __restrict__ logits, int64_t ldl, const int64_t* __restrict__ labels, int Q, int nc,
                                                            float margin, const float* __restrict__ weight, float* __restrict__ loss,
                                                            float* __restrict__ g, int64_t ldg, double* __restrict__ stats, int* __restrict__ flags) {
  __shared__ double red[CL_THREADS];
  const float w = weight ? weight[0] : 1.f;
  const double denom = KIND == QAGNN_LOSS_MARGIN_RANK ? (double)Q * (double)(nc - 1) : (double)Q;
  const float gscale = (float)((double)w / denom);
  double acc = 0.0;
  for (int q = threadIdx.x; q < Q; q += CL_THREADS) {
    const float* __restrict__ row = logits + (int64_t)q * ldl;
    float* __restrict__ grow = g + (int64_t)q * ldg;
    const int64_t lab = labels[q];
    if (lab < 0 || lab >= (int64_t)nc) {  // (no address is formed from it)
      if (flags) flags[0] = 1;
      for (int c = 0; c < nc; ++c) grow[c] = 0.f;
      continue;
    }
    const int l = (int)lab;
    const float xl = row[l];
    if constexpr (KIND == QAGNN_LOSS_CROSS_ENTROPY) {
      float m = row[0];
      for (int c = 1; c < nc; ++c) {
        const float v = row[c];
        if (v > m || v != v) m = v;  // a NaN, once taken, stays (nothing compares greater): the whole row becomes NaN, as in torch
      }
      float s = 0.f;
      for (int c = 0; c < nc; ++c) s += expf(row[c] - m);
      acc += (double)(logf(s) - (xl - m));
      for (int c = 0; c < nc; ++c) {
        const float p = expf(row[c] - m) / s;
        grow[c] = (c == l ? p - 1.f : p) * gscale;
      }
    } else {
      double rs = 0.0;
      int active = 0;
      for (int c = 0; c < nc; ++c) {
        if (c == l) continue;
        const float h = hinge_arg(xl, row[c], margin);
        const bool on = h >= 0.f;
        rs += (double)((on || h != h) ? h : 0.f);
        active += on;
        grow[c] = on ? gscale : 0.f;
      }
      acc += rs;
      grow[l] = -((float)active * gscale);
    }
  }
  red[threadIdx.x] = acc;
  __syncthreads();
#pragma unroll
  for (int s = CL_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float out = (float)((double)w * red[0] / denom);
    loss[0] = out;
    if (stats) {
      stats[0] += (double)out;
      stats[1] += 1.0;
    }
  }
}

__global__ __launch_bounds__(CL_THREADS) void k_choice_loss_bwd(const float* g, int64_t ldg, const float* __restrict__ grad_out, float* dlogits, int64_t ldd,
                                                                int64_t total, int nc) {
  // (g and dlogits may be one buffer: an element is read and written by the same thread)
  const float go = grad_out[0];
  for (int64_t i = (int64_t)blockIdx.x * CL_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * CL_THREADS) {
    const int64_t q = i / nc;
    const int c = (int)(i - q * nc);
    dlogits[q * ldd + c] = g[q * ldg + c] * go;
  }
}

}  // namespace qagnn

using namespace qagnn;

extern "C" int qagnn_loss_version(void) { return 1; }

extern "C" int qagnn_choice_loss_f32(const float* logits, int64_t ldl, const int64_t* labels, int32_t Q, int32_t nc, int32_t kind, float margin,
                                     const float* weight, float* loss, float* g, int64_t ldg, double* stats, int32_t* flags, qagnn_stream_t stream) {
  QAGNN_REQUIRE(logits && labels && loss && g && Q > 0, QAGNN_EINVAL, "choice_loss: bad arguments");
  QAGNN_REQUIRE(kind == QAGNN_LOSS_CROSS_ENTROPY || kind == QAGNN_LOSS_MARGIN_RANK, QAGNN_EINVAL, "choice_loss: unknown kind %d", kind);
  QAGNN_REQUIRE(nc >= (kind == QAGNN_LOSS_MARGIN_RANK ? 2 : 1) && nc <= 1024 && ldl >= nc && ldg >= nc, QAGNN_EINVAL,
                "choice_loss: nc=%d must be in %d..1024 and the pitches ldl=%lld, ldg=%lld >= nc", nc, kind == QAGNN_LOSS_MARGIN_RANK ? 2 : 1,
                (long long)ldl, (long long)ldg);
  if (kind == QAGNN_LOSS_CROSS_ENTROPY)
    k_choice_loss<QAGNN_LOSS_CROSS_ENTROPY><<<1, CL_THREADS, 0, (hipStream_t)stream>>>(logits, ldl, labels, Q, nc, margin, weight, loss, g, ldg, stats, flags);
  else
    k_choice_loss<QAGNN_LOSS_MARGIN_RANK><<<1, CL_THREADS, 0, (hipStream_t)stream>>>(logits, ldl, labels, Q, nc, margin, weight, loss, g, ldg, stats, flags);
  QAGNN_LAUNCH_CHECK("k_choice_loss");
  return QAGNN_OK;
}

extern "C" int qagnn_choice_loss_bwd_f32(const float* g, int64_t ldg, const float* grad_out, float* dlogits, int64_t ldd, int32_t Q, int32_t nc,
                                         qagnn_stream_t stream) {
  QAGNN_REQUIRE(g && grad_out && dlogits && Q > 0, QAGNN_EINVAL, "choice_loss_bwd: bad arguments");
  QAGNN_REQUIRE(nc >= 1 && nc <= 1024 && ldg >= nc && ldd >= nc, QAGNN_EINVAL, "choice_loss_bwd: nc=%d must be in 1..1024 and the pitches ldg=%lld, ldd=%lld >= nc",
                nc, (long long)ldg, (long long)ldd);
  const int64_t total = (int64_t)Q * nc;
  const int grid = (int)(total / CL_THREADS + 1 < 1024 ? total / CL_THREADS + 1 : 1024);
  k_choice_loss_bwd<<<grid, CL_THREADS, 0, (hipStream_t)stream>>>(g, ldg, grad_out, dlogits, ldd, total, nc);
  QAGNN_LAUNCH_CHECK("k_choice_loss_bwd");
  return QAGNN_OK;
}
