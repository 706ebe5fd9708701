// Detailed evaluation (include/qagnn_hip_explain.h): the attention of an evaluated stack in the caller's edge order, and its trace out of
// the context node of every subgraph -- the interpretability half of QA-GNN (reference qagnn.py:343-430 hands the graphs back so that
// attention can be laid over them).  Shape of pool.hip: a workgroup per subgraph, the running layer in LDS, wave-level reductions for
// the long segments (the context node's in-degree is close to n), one 16-byte load per [.][4] attention row.
#include <limits.h>

#include "common.h"
#include "../../include/qagnn_hip_explain.h"

namespace qagnn {

constexpr int EX_THREADS = 256;
constexpr int TR_THREADS = 256;                 // 4 waves = 16 rows of 16 lanes
constexpr int TR_MAXN = QAGNN_TRACE_MAX_N;
constexpr int TR_LONG = 64;                     // a segment above this many edges is walked by a whole wave, else by a 16-lane row
constexpr int TR_ROWS = TR_THREADS / 16, TR_WAVES = TR_THREADS / 64;

// grid = (ceil(Ep / 256), min(k, 64)); the count of live positions is read here (capacity forms: Ep is a capacity)
__global__ __launch_bounds__(EX_THREADS) void k_attn_export(const int* __restrict__ rowptr_s, const int* __restrict__ eid_s, int N, int Ep,
                                                            const float* __restrict__ a, int64_t ls, int k, float* __restrict__ out, int64_t ols) {
  int cnt = rowptr_s[N];
  cnt = cnt < 0 ? 0 : (cnt > Ep ? Ep : cnt);
  const int p = blockIdx.x * EX_THREADS + threadIdx.x;
  if (p >= cnt) return;
  const int e = eid_s[p];
  if ((unsigned)e >= (unsigned)cnt) return;  // (a corrupt graph: never stored through)
  for (int l = blockIdx.y; l < k; l += gridDim.y) st4(out + l * ols + 4 * (int64_t)e, ld4(a + l * ls + 4 * (int64_t)p));
}

// (value, segment index): the larger value, among equals the earlier index; values are never NaN (a NaN candidate is never taken)
__device__ __forceinline__ void cand_merge(float& v, int& i, float ov, int oi) {
  if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}
template <int WIDTH>  // butterfly over WIDTH lanes (16: inside a DPP row; 64: the wave); every lane ends up with the winner
__device__ __forceinline__ void cand_reduce(float& v, int& i) {
#pragma unroll
  for (int m = WIDTH / 2; m >= 1; m >>= 1) {
    const float ov = __shfl_xor(v, m, 64);
    const int oi = __shfl_xor(i, m, 64);
    cand_merge(v, i, ov, oi);
  }
}

__device__ __forceinline__ float head_mean(float4 v, int head) {
  return head < 0 ? ((v.x + v.y) + (v.z + v.w)) * 0.25f : (head == 0 ? v.x : (head == 1 ? v.y : (head == 2 ? v.z : v.w)));
}

// one lane's share of a segment: i = first, first + step, ... < end, in segment order
__device__ __forceinline__ void walk_segment(int first, int end, int step, const int* __restrict__ src_t, const int* __restrict__ pos_t,
                                             const float* __restrict__ al, int Ep, int row0, int n, int head, const float* __restrict__ fl,
                                             const float* __restrict__ bs, float& f, float& bv, int& bi) {
  for (int i = first; i < end; i += step) {
    int p = pos_t[i], s = src_t[i] - row0;
    p = p < 0 ? 0 : (p >= Ep ? Ep - 1 : p);
    s = s < 0 ? 0 : (s >= n ? n - 1 : s);  // a source outside the block (err[1]): clamped before it forms an address
    const float ab = head_mean(ld4(al + 4 * (int64_t)p), head);
    f += ab * fl[s];
    const float c = ab * bs[s];
    if (c > bv) { bv = c; bi = i; }  // (strict: the earlier edge among equals; false for a NaN)
  }
}

// grid = B, block = 256
__global__ __launch_bounds__(TR_THREADS) void k_attn_trace(const int* __restrict__ rowptr_t, const int* __restrict__ src_t,
                                                          const int* __restrict__ pos_t, const int* __restrict__ eid_s, int N, int Ep,
                                                          const float* __restrict__ a, int64_t ls, int k, int n, int root, int head,
                                                          float* __restrict__ flow, float* __restrict__ best, int* __restrict__ pred) {
  __shared__ float s_flow[2][TR_MAXN];
  __shared__ float s_best[2][TR_MAXN];
  __shared__ int s_pred[TR_MAXN];
  __shared__ int s_rp[TR_MAXN + 1];
  const int b = blockIdx.x, tid = threadIdx.x, row0 = b * n;
  for (int j = tid; j <= n; j += TR_THREADS) {
    const int r = rowptr_t[row0 + j];
    s_rp[j] = r < 0 ? 0 : (r > Ep ? Ep : r);
  }
  for (int j = tid; j < n; j += TR_THREADS) {
    const float v = j == root ? 1.f : 0.f;
    s_flow[0][j] = s_best[0][j] = v;
    flow[row0 + j] = v;
    best[row0 + j] = v;
  }
  __syncthreads();
  const int lane16 = tid & 15, row = tid >> 4, lane = tid & 63, w = tid >> 6;
  for (int l = 0; l < k; ++l) {
    const float* al = a + l * ls;
    const float *fl = s_flow[l & 1], *bs = s_best[l & 1];
    float *fo = s_flow[(l + 1) & 1], *bo = s_best[(l + 1) & 1];
    // segments of up to TR_LONG edges: a 16-lane row each (the loop bounds are the block's: every lane reaches the reductions)
    for (int j0 = 0; j0 < n; j0 += TR_ROWS) {
      const int j = j0 + row;
      int beg = 0, end = 0;
      if (j < n) { beg = s_rp[j]; end = s_rp[j + 1]; }
      const bool mine = j < n && end - beg <= TR_LONG;
      float f = 0.f, bv = 0.f;
      int bi = INT_MAX;
      if (mine) walk_segment(beg + lane16, end, 16, src_t, pos_t, al, Ep, row0, n, head, fl, bs, f, bv, bi);
      f = row16_sum(f);
      cand_reduce<16>(bv, bi);
      if (mine && lane16 == 0) {
        fo[j] = f;
        bo[j] = bv;
        s_pred[j] = bv > 0.f ? bi : -1;
      }
    }
    // longer ones (the context node, hubs): a wave each
    for (int j = w; j < n; j += TR_WAVES) {
      const int beg = s_rp[j], end = s_rp[j + 1];
      if (end - beg <= TR_LONG) continue;  // (the same for the whole wave)
      float f = 0.f, bv = 0.f;
      int bi = INT_MAX;
      walk_segment(beg + lane, end, 64, src_t, pos_t, al, Ep, row0, n, head, fl, bs, f, bv, bi);
      f = wave_sum(f);
      cand_reduce<64>(bv, bi);
      if (lane == 0) {
        fo[j] = f;
        bo[j] = bv;
        s_pred[j] = bv > 0.f ? bi : -1;
      }
    }
    __syncthreads();
    for (int j = tid; j < n; j += TR_THREADS) {
      flow[(int64_t)(l + 1) * N + row0 + j] = fo[j];
      best[(int64_t)(l + 1) * N + row0 + j] = bo[j];
      const int i = s_pred[j];
      int e = -1;
      if (i >= 0) {
        int p = pos_t[i];
        p = p < 0 ? 0 : (p >= Ep ? Ep - 1 : p);
        e = eid_s[p];
      }
      pred[(int64_t)l * N + row0 + j] = e;
    }
    // (the next layer writes the buffers this one read, and s_pred: behind every reader of both)
    __syncthreads();
  }
}

static int check_attention(const char* what, const qagnn_graph* g, const float* a, int64_t layer_stride, int32_t k) {
  QAGNN_REQUIRE(g && g->N >= 1 && g->Ep >= g->N, QAGNN_EINVAL, "%s: no graph", what);
  QAGNN_REQUIRE(k >= 0, QAGNN_EINVAL, "%s: k = %d layers", what, k);
  if (k > 0) {
    QAGNN_REQUIRE(a && aligned16(a), QAGNN_EINVAL, "%s: a is null or not 16-byte aligned", what);
    QAGNN_REQUIRE(layer_stride >= 4 * (int64_t)g->Ep && layer_stride % 4 == 0, QAGNN_EINVAL,
                  "%s: layer_stride = %lld floats, need a multiple of 4 at or above 4 * Ep = %lld", what, (long long)layer_stride,
                  4 * (long long)g->Ep);
  }
  return QAGNN_OK;
}

}  // namespace qagnn

using namespace qagnn;

extern "C" int qagnn_explain_version(void) { return 1; }

extern "C" int qagnn_attn_export_f32(const qagnn_graph* g, const float* a, int64_t layer_stride, int32_t k, float* out, int64_t out_layer_stride,
                                     qagnn_stream_t stream) {
  if (int rc = check_attention("attn_export", g, a, layer_stride, k)) return rc;
  if (k == 0) return QAGNN_OK;
  QAGNN_REQUIRE(out && aligned16(out), QAGNN_EINVAL, "attn_export: out is null or not 16-byte aligned");
  QAGNN_REQUIRE(out_layer_stride >= 4 * (int64_t)g->Ep && out_layer_stride % 4 == 0, QAGNN_EINVAL,
                "attn_export: out_layer_stride = %lld floats, need a multiple of 4 at or above 4 * Ep = %lld", (long long)out_layer_stride,
                4 * (long long)g->Ep);
  const dim3 grid(cdiv(g->Ep, EX_THREADS), k < 64 ? k : 64);
  k_attn_export<<<grid, EX_THREADS, 0, (hipStream_t)stream>>>(g->rowptr_s, g->eid_s, g->N, g->Ep, a, layer_stride, k, out, out_layer_stride);
  QAGNN_LAUNCH_CHECK("k_attn_export");
  return QAGNN_OK;
}

extern "C" int qagnn_attn_trace_f32(const qagnn_graph* g, const float* a, int64_t layer_stride, int32_t k, int32_t B, int32_t n, int32_t root,
                                    int32_t head, float* flow, float* best, int32_t* pred, qagnn_stream_t stream) {
  if (int rc = check_attention("attn_trace", g, a, layer_stride, k)) return rc;
  QAGNN_REQUIRE(n >= 1 && n <= TR_MAXN, QAGNN_EINVAL,"attn_trace: n = %d node slots per subgraph outside [1, %d]", n, TR_MAXN);
  QAGNN_REQUIRE(B >= 1 && (int64_t)B * n == g->N, QAGNN_EINVAL, "attn_trace: the graph has N = %d node rows, not B * n = %d * %d", g->N, B, n);
  QAGNN_REQUIRE(g->block_n == n, QAGNN_EINVAL, "attn_trace: the graph was prepared for blocks of %d node rows, not n = %d", g->block_n, n);
  QAGNN_REQUIRE(root >= 0 && root < n, QAGNN_EINVAL, "attn_trace: root = %d outside [0, n = %d)", root, n);
  QAGNN_REQUIRE(head >= -1 && head <= 3, QAGNN_EINVAL, "attn_trace: head = %d outside [-1, 3]", head);
  QAGNN_REQUIRE(flow && best && (pred || k == 0), QAGNN_EINVAL, "attn_trace: null output");
  k_attn_trace<<<B, TR_THREADS, 0, (hipStream_t)stream>>>(g->rowptr_t, g->src_t, g->pos_t, g->eid_s, g->N, g->Ep, a, layer_stride, k, n, root, head,
                                                          flow, best, pred);
  QAGNN_LAUNCH_CHECK("k_attn_trace");
  return QAGNN_OK;
}
