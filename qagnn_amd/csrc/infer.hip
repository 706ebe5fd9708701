// The kernels of the forward-only (evaluation) path: include/qagnn_hip_infer.h.  The sequencing of the stack lives in hop.hip, next to
// the static helpers it shares with the training forward.
#include "common.h"

namespace qagnn {

// ---- max relu(scale * H + shift): the operand maximum of the BatchNorm + ReLU prologue, measured ----------------------------------
// With running statistics nothing bounds relu(bn(h1)) (the training forward's bound comes from the batch variance), so the second mlp
// product of an eval hop gets the true maximum from one streaming read of h1: 53 MB at 64 000 x 208, HBM-bound.  A thread owns ONE group
// of four columns -- scale / shift stay in registers -- and walks rows; a block is 256 / (Cc / 4) row lanes x Cc / 4 column groups (4 x 52
// at Cc = 208: 208 of 256 lanes load, each a 16-byte piece of a contiguous 832-byte row) over BRA_ROWS rows per lane, UNR rows in flight.
// Per-block maxima leave by a plain store and launch_amax_reduce folds them: no atomics on the tail of ~2 000 blocks (common.h, the
// note at wave_amax_lane63).  The value is the prologue's own: floor_nan(fmaf(x, scale, shift), 0); fmaxf drops the NaNs.
constexpr int BRA_THREADS = 256, BRA_ROWS = 8, BRA_MAX_BLOCKS = 2048;
struct BraShape { int W, G, rows_per_block, grid; };
static BraShape bra_shape(int R, int Cc) {
  BraShape s;
  const int c4 = Cc / 4;
  s.W = c4 < BRA_THREADS ? c4 : BRA_THREADS;  // column groups side by side (wider matrices: a thread walks groups W apart)
  s.G = BRA_THREADS / s.W;                    // row lanes
  int rows = s.G * BRA_ROWS;
  const int need = cdiv(R, BRA_MAX_BLOCKS);
  if (rows < need) rows = cdiv(need, s.G) * s.G;
  s.rows_per_block = rows;
  s.grid = cdiv(R, rows);
  return s;
}

__device__ __forceinline__ float relu_affine_max4(float4 v, float4 sc, float4 sh, float m) {
  m = fmaxf(m, floor_nan(fmaf(v.x, sc.x, sh.x), 0.f));
  m = fmaxf(m, floor_nan(fmaf(v.y, sc.y, sh.y), 0.f));
  m = fmaxf(m, floor_nan(fmaf(v.z, sc.z, sh.z), 0.f));
  m = fmaxf(m, floor_nan(fmaf(v.w, sc.w, sh.w), 0.f));
  return m;
}

__global__ __launch_bounds__(BRA_THREADS) void k_bn_relu_absmax(const float* __restrict__ H, int ldh, int R, int c4n, int W, int G, int rows_per_block,
                                                                const float* __restrict__ scale, const float* __restrict__ shift,
                                                                float* __restrict__ part) {
  __shared__ float red[BRA_THREADS / 64];
  constexpr int UNR = 4;
  const int cl = threadIdx.x % W, rl = threadIdx.x / W;
  const int r0 = blockIdx.x * rows_per_block;
  const int r1 = min(r0 + rows_per_block, R);
  float m = 0.f;
  if (rl < G) {
    for (int cg = cl; cg < c4n; cg += W) {
      const float4 sc = ld4(scale + cg * 4), sh = ld4(shift + cg * 4);
      const float* __restrict__ col = H + cg * 4;
      int r = r0 + rl;
      for (; r + (UNR - 1) * G < r1; r += UNR * G) {  // UNR independent 16-byte loads in flight per lane
        float4 v[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) v[u] = ld4(col + (int64_t)(r + u * G) * ldh);
#pragma unroll
        for (int u = 0; u < UNR; ++u) m = relu_affine_max4(v[u], sc, sh, m);
      }
      for (; r < r1; r += G) m = relu_affine_max4(ld4(col + (int64_t)r * ldh), sc, sh, m);
    }
  }
  m = wave_amax_lane63(m);  // (whole waves: idle lanes carry 0)
  if ((threadIdx.x & 63) == 63) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

int launch_bn_relu_absmax(const float* H, int ldh, int R, int Cc, const float* scale, const float* shift, uint32_t* slot, float* part,
                          hipStream_t stream) {
  const BraShape s = bra_shape(R, Cc);
  k_bn_relu_absmax<<<s.grid, BRA_THREADS, 0, stream>>>(H, ldh, R, Cc / 4, s.W, s.G, s.rows_per_block, scale, shift, part);
  QAGNN_LAUNCH_CHECK("k_bn_relu_absmax");
  return launch_amax_reduce(part, s.grid, slot, stream);
}

// ---- multiple-choice scoring: argmax per question, counters on the device ---------------------------------------------------------
// A question's nc logits are a handful of floats (5 on CommonsenseQA): one thread per question.  torch.argmax's order: a NaN is the
// greatest value, the first index wins among equals (and among NaNs).  One 64-bit integer atomic per block for the matches, one per
// launch for the questions seen.
constexpr int CE_THREADS = 256;
__global__ __launch_bounds__(CE_THREADS) void k_choice_eval(const float* __restrict__ logits, int64_t ldl, const int64_t* __restrict__ labels, int Q,
                                                            int nc, int64_t* __restrict__ pred, unsigned long long* __restrict__ counts) {
  __shared__ int hits[CE_THREADS / 64];
  const int q = blockIdx.x * CE_THREADS + threadIdx.x;
  int hit = 0;
  if (q < Q) {
    const float* __restrict__ row = logits + (int64_t)q * ldl;
    float best = row[0];
    int bi = 0;
    for (int c = 1; c < nc; ++c) {
      const float v = row[c];
      if (best == best && (v > best || v != v)) { best = v; bi = c; }
    }
    if (pred) pred[q] = bi;
    if (labels) hit = labels[q] == (int64_t)bi;  // (bi is in [0, nc): a label outside it never matches)
  }
  const unsigned long long ballot = __ballot(hit);
  if ((threadIdx.x & 63) == 0) hits[threadIdx.x >> 6] = __popcll(ballot);
  __syncthreads();
  if (threadIdx.x == 0) {
    const int n = hits[0] + hits[1] + hits[2] + hits[3];
    if (n > 0) atomicAdd(counts, (unsigned long long)n);
    if (blockIdx.x == 0) atomicAdd(counts + 1, (unsigned long long)Q);
  }
}

}  // namespace qagnn

using namespace qagnn;

extern "C" int qagnn_infer_version(void) { return 1; }

extern "C" int64_t qagnn_bn_relu_absmax_scratch_elems(int32_t R, int32_t Cc) {
  if (R <= 0 || Cc <= 0 || Cc % 4 != 0) return 0;
  return bra_shape(R, Cc).grid;
}

extern "C" int qagnn_bn_relu_absmax_f32(const float* H, int32_t ldh, int32_t R, int32_t Cc, const float* scale, const float* shift, uint32_t* slot,
                                        float* scratch, qagnn_stream_t stream) {
  QAGNN_REQUIRE(H && scale && shift && slot && scratch && R > 0 && Cc > 0, QAGNN_EINVAL, "bn_relu_absmax: bad arguments");
  QAGNN_REQUIRE(Cc % 4 == 0 && ldh >= Cc && ldh % 4 == 0, QAGNN_EINVAL,
                "bn_relu_absmax: Cc=%d must be a multiple of 4 and the pitch ldh=%d a multiple of 4, >= Cc", Cc, ldh);
  QAGNN_REQUIRE(aligned16(H) && aligned16(scale) && aligned16(shift), QAGNN_EINVAL, "bn_relu_absmax: H / scale / shift must be 16-byte aligned");
  return launch_bn_relu_absmax(H, ldh, R, Cc, scale, shift, slot, scratch, (hipStream_t)stream);
}

extern "C" int qagnn_choice_eval_f32(const float* logits, int64_t ldl, const int64_t* labels, int32_t Q, int32_t nc, int64_t* pred, int64_t* counts,
                                     qagnn_stream_t stream) {
  QAGNN_REQUIRE(logits && counts && Q > 0, QAGNN_EINVAL, "choice_eval: bad arguments");
  QAGNN_REQUIRE(nc >= 1 && nc <= 1024 && ldl >= nc, QAGNN_EINVAL, "choice_eval: nc=%d must be in 1..1024 and the pitch ldl=%lld >= nc", nc, (long long)ldl);
  k_choice_eval<<<cdiv(Q, CE_THREADS), CE_THREADS, 0, (hipStream_t)stream>>>(logits, ldl, labels, Q, nc, pred, reinterpret_cast<unsigned long long*>(counts));
  QAGNN_LAUNCH_CHECK("k_choice_eval");
  return QAGNN_OK;
}
