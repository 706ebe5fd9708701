// The gradient of a trainable entity table (include/qagnn_hip_rows.h): positions grouped by row id, segment sums, row scatter.
#include "common.h"
#include "../../include/qagnn_hip_rows.h"

namespace qagnn {

// ---- grouping: a stable LSD radix sort of the live positions by row id, two digits of RG_BITS bits -------------------------------------
// The design of graph_prep.hip's counting sort by class: per block of RG_BLK positions a histogram in LDS, the blocks' bases by a column
// walk and one block-wide scan, then a stable scatter by ONE wave per block that ranks 64 positions at a time with ballots.
#define RG_BITS 13
#define RG_BUCKETS 8192
#define RG_BLK 1024
#define RG_SCAN_ITEMS 8
#define RS_WAVES 4
static_assert(RG_BUCKETS == 1 << RG_BITS, "one bucket per digit value");
static_assert(RG_BUCKETS == 1024 * RG_SCAN_ITEMS, "k_rg_scan takes the bucket totals in one round");
static_assert((int64_t)QAGNN_ROWS_MAX_TABLE <= (int64_t)RG_BUCKETS * RG_BUCKETS, "two digits cover every admitted row id");
static_assert(QAGNN_ROWS_CHUNK == 64, "one wave ranks the chunk starts of QAGNN_ROWS_CHUNK positions with one ballot");

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// position and key of slot j of pass PASS, or p = -1 where the slot is not live.  Pass 0 reads the positions themselves (live: an id
// inside the table), pass 1 the M positions pass 0 left in `src`, M = *m_dev.
template <int PASS>
__device__ __forceinline__ int rg_slot(const int64_t* __restrict__ ridx, const int* __restrict__ src, const int* __restrict__ m_dev, int N,
                                       int64_t table_rows, int j, int& digit) {
  digit = 0;
  if (PASS == 0) {
    if (j >= N) return -1;
    const int64_t id = ridx[j];
    if (id < 0 || id >= table_rows) return -1;
    digit = (int)(id & (RG_BUCKETS - 1));
    return j;
  }
  if (j >= clampi(*m_dev, 0, N)) return -1;
  const int p = src[j];
  if ((unsigned)p >= (unsigned)N) return -1;
  digit = (int)((ridx[p] >> RG_BITS) & (RG_BUCKETS - 1));
  return p;
}

template <int PASS>
__global__ __launch_bounds__(256) void k_rg_hist(const int64_t* __restrict__ ridx, const int* __restrict__ src, const int* __restrict__ m_dev,
                                                 int N, int64_t table_rows, int* __restrict__ hist) {
  __shared__ int lh[RG_BUCKETS];
  for (int c = threadIdx.x; c < RG_BUCKETS; c += 256) lh[c] = 0;
  __syncthreads();
  const int base = blockIdx.x * RG_BLK;
  for (int i = threadIdx.x; i < RG_BLK; i += 256) {
    int d;
    if (rg_slot<PASS>(ridx, src, m_dev, N, table_rows, base + i, d) >= 0) atomicAdd(&lh[d], 1);  // (integer counts: the order does not show)
  }
  __syncthreads();
  for (int c = threadIdx.x; c < RG_BUCKETS; c += 256) hist[(int64_t)blockIdx.x * RG_BUCKETS + c] = lh[c];
}

// hist[b][c] <- the number of bucket c's slots in the blocks before b; total[c] = all of them.  One thread per bucket (coalesced rows).
__global__ __launch_bounds__(256) void k_rg_colscan(int* __restrict__ hist, int* __restrict__ total, int nblk) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  int run = 0;
  for (int b = 0; b < nblk; ++b) {
    const int v = hist[(int64_t)b * RG_BUCKETS + c];
    hist[(int64_t)b * RG_BUCKETS + c] = run;
    run += v;
  }
  total[c] = run;
}

// One round of a 1024-thread exclusive scan: a thread brings the sum of its own items and gets the sum of the threads before it; the
// block's total comes back through `all`.  wtot: 16 ints of LDS.  (Two barriers; a third in front of the next round is the caller's.)
__device__ __forceinline__ int block_scan_round(int tsum, int* __restrict__ wtot, int& all) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  int incl = tsum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(incl, o, 64);
    if (lane >= o) incl += u;
  }
  if (lane == 63) wtot[wid] = incl;
  __syncthreads();
  if (wid == 0) {
    int w = lane < 16 ? wtot[lane] : 0;
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
      const int u = __shfl_up(w, o, 64);
      if (lane >= o) w += u;
    }
    if (lane < 16) wtot[lane] = w;  // inclusive over waves
  }
  __syncthreads();
  all = wtot[15];
  return (wid ? wtot[wid - 1] : 0) + incl - tsum;
}

// start[c] = first slot of bucket c, start[RG_BUCKETS] = the number of live slots
__global__ __launch_bounds__(1024) void k_rg_scan(const int* __restrict__ total, int* __restrict__ start) {
  __shared__ int wtot[16];
  const int i0 = threadIdx.x * RG_SCAN_ITEMS;
  int v[RG_SCAN_ITEMS], tsum = 0;
#pragma unroll
  for (int k = 0; k < RG_SCAN_ITEMS; ++k) {
    v[k] = total[i0 + k];
    tsum += v[k];
  }
  int all;
  int run = block_scan_round(tsum, wtot, all);
#pragma unroll
  for (int k = 0; k < RG_SCAN_ITEMS; ++k) {
    start[i0 + k] = run;
    run += v[k];
  }
  if (threadIdx.x == 0) start[RG_BUCKETS] = all;
}

// Stable scatter of one block's slots into the digit order, one wave per block (k_cls_scatter's ranking)
template <int PASS>
__global__ __launch_bounds__(64) void k_rg_scatter(const int64_t* __restrict__ ridx, const int* __restrict__ src, const int* __restrict__ m_dev,
                                                   int N, int64_t table_rows, const int* __restrict__ hist, const int* __restrict__ start,
                                                   int* __restrict__ dst) {
  __shared__ int cnt[RG_BUCKETS];  // next slot of bucket c for this block
  const int lane = threadIdx.x, base = blockIdx.x * RG_BLK;
  for (int c = lane; c < RG_BUCKETS; c += 64) cnt[c] = hist[(int64_t)blockIdx.x * RG_BUCKETS + c] + start[c];
  __syncthreads();
  const unsigned long long lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));  // lanes below this one
  for (int q = 0; q < RG_BLK / 64; ++q) {
    int d;
    const int p = rg_slot<PASS>(ridx, src, m_dev, N, table_rows, base + q * 64 + lane, d);
    const bool live = p >= 0;
    const int c = live ? d : -1;
    const int first = live ? cnt[c] : 0;  // slot of the chunk's first position of bucket c
    int rank = 0, total = 0;
    unsigned long long todo = __ballot(live);
    while (todo) {
      const int cl = __builtin_amdgcn_readlane(c, __builtin_ctzll(todo));
      const unsigned long long m = __ballot(c == cl);
      if (c == cl) {
        rank = __builtin_popcountll(m & lt);
        total = __builtin_popcountll(m);
      }
      todo &= ~m;
    }
    __syncthreads();  // (one wave: orders the reads of cnt above against the writes below)
    if (live) {
      if (rank == 0) cnt[c] = first + total;  // exactly one lane per bucket of the chunk
      const int at = first + rank;
      if ((unsigned)at < (unsigned)N) dst[at] = p;
    }
    __syncthreads();
  }
}

// Head flags and their scan over the sorted positions, one block: seg, uniq and count, and the tails of all four outputs.
__global__ __launch_bounds__(1024) void k_rg_segments(const int64_t* __restrict__ ridx, int* __restrict__ order, const int* __restrict__ m_dev,
                                                      int N, int* __restrict__ seg, int64_t* __restrict__ uniq, int* __restrict__ count) {
  __shared__ int wtot[16];
  const int tid = threadIdx.x;
  const int M = clampi(*m_dev, 0, N);
  int carry = 0;
  for (int base = 0; base < M; base += 1024 * RG_SCAN_ITEMS) {
    const int i0 = base + tid * RG_SCAN_ITEMS;
    int64_t id[RG_SCAN_ITEMS + 1];  // id[k + 1]: slot i0 + k; id[0]: the slot in front
    id[0] = i0 > 0 && i0 <= M ? ridx[order[i0 - 1]] : -1;
    int tsum = 0;
#pragma unroll
    for (int k = 0; k < RG_SCAN_ITEMS; ++k) {
      id[k + 1] = i0 + k < M ? ridx[order[i0 + k]] : -1;
      tsum += (i0 + k < M && id[k + 1] != id[k]) ? 1 : 0;
    }
    int all;
    int run = carry + block_scan_round(tsum, wtot, all);
#pragma unroll
    for (int k = 0; k < RG_SCAN_ITEMS; ++k) {
      if (i0 + k < M && id[k + 1] != id[k]) {
        seg[run] = i0 + k;
        uniq[run] = id[k + 1];
        ++run;
      }
    }
    carry += all;
    __syncthreads();  // (wtot is written again in the next round)
  }
  const int U = carry;  // <= M <= N
  if (tid == 0) count[0] = U;
  for (int u = U + tid; u <= N; u += 1024) seg[u] = M;
  for (int u = U + tid; u < N; u += 1024) uniq[u] = -1;
  for (int j = M + tid; j < N; j += 1024) order[j] = -1;
}

// ---- segment sums ------------------------------------------------------------------------------------------------------------------------
// The sorted slots are cut into TILES of 64 (the launch's unit, by capacity); a segment is cut into CHUNKS of 64 counted from its own
// start (the arithmetic's unit).  A wave takes a tile and sums every chunk that STARTS in it -- at most 128 rows, whatever the segments
// look like.  A one-chunk segment's partial is its row of G.  The partials of a longer segment go to the workspace, slot
// 2 * (tile of the chunk's start) + (first chunk of its segment ? 1 : 0): a tile holds at most one start of either kind, because full
// chunks of one segment are 64 apart and a segment longer than 64 keeps the next such start more than 64 away.
// lane's slot j of the tile -> its segment u = the last one that starts at or before j, [s, e)
__device__ __forceinline__ int seg_of(const int* __restrict__ seg, int U, int M, int j, int& s, int& e) {
  int lo = 0, hi = U - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (seg[mid] <= j) lo = mid; else hi = mid - 1;
  }
  s = clampi(seg[lo], 0, M);
  e = clampi(seg[lo + 1], s, M);
  return lo;
}

__global__ __launch_bounds__(64 * RS_WAVES) void k_seg_partial(const float* __restrict__ X, int64_t ldx, int c4, const int* __restrict__ order,
                                                               const int* __restrict__ seg, const int* __restrict__ count, int N,
                                                               float* __restrict__ G, int64_t ldg, int g_rows, float* __restrict__ P) {
  const int lane = threadIdx.x & 63, tile = blockIdx.x * RS_WAVES + (threadIdx.x >> 6);
  const int U = clampi(*count, 0, g_rows);
  if (U == 0) return;
  const int M = clampi(seg[U], 0, N);
  if ((int64_t)tile * 64 >= M) return;  // (the whole wave)
  const int j = tile * 64 + lane;
  int u = 0, s = 0, e = 0;
  bool is_start = false;
  if (j < M) {
    u = seg_of(seg, U, M, j, s, e);
    is_start = j >= s && j < e && ((j - s) & (QAGNN_ROWS_CHUNK - 1)) == 0;
  }
  unsigned long long todo = __ballot(is_start);
  while (todo) {
    const int l = __builtin_ctzll(todo);
    todo &= todo - 1;
    const int su = __builtin_amdgcn_readlane(s, l), eu = __builtin_amdgcn_readlane(e, l), uu = __builtin_amdgcn_readlane(u, l);
    const int j0 = tile * 64 + l;
    const int len = min(eu - j0, QAGNN_ROWS_CHUNK);
    const int row = lane < len ? order[j0 + lane] : -1;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    bool first = true;
    for (int i = 0; i < len; i += 4) {  // four rows in flight, added in their order
      float4 v[4];
      bool ok[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int r = __builtin_amdgcn_readlane(row, (i + q) & 63);
        ok[q] = i + q < len && lane < c4 && (unsigned)r < (unsigned)N;
        if (ok[q]) v[q] = ld4(X + (int64_t)r * ldx + lane * 4);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (ok[q]) {
          acc = first ? v[q] : add4(acc, v[q]);
          first = false;
        }
    }
    if (lane < c4) {
      if (eu - su <= QAGNN_ROWS_CHUNK) st4(G + (int64_t)uu * ldg + lane * 4, acc);
      else st4(P + ((int64_t)2 * tile + (j0 == su ? 1 : 0)) * (c4 * 4) + lane * 4, acc);
    }
  }
}

// A wave takes a tile again: the segment longer than one chunk that starts in it (at most one) gets its partials added in ascending
// order; and rows [64 tile, 64 tile + 64) of G that lie behind the last segment are written as zeros.
__global__ __launch_bounds__(64 * RS_WAVES) void k_seg_final(int c4, const int* __restrict__ seg, const int* __restrict__ count, int N,
                                                             float* __restrict__ G, int64_t ldg, int g_rows, const float* __restrict__ P) {
  const int lane = threadIdx.x & 63, tile = blockIdx.x * RS_WAVES + (threadIdx.x >> 6);
  const int U = clampi(*count, 0, g_rows);
  if (lane < c4)
    for (int u = max(U, tile * 64); u < min(g_rows, tile * 64 + 64); ++u) st4(G + (int64_t)u * ldg + lane * 4, make_float4(0.f, 0.f, 0.f, 0.f));
  if (U == 0) return;
  const int M = clampi(seg[U], 0, N);
  if ((int64_t)tile * 64 >= M) return;
  const int j = tile * 64 + lane;
  int u = 0, s = 0, e = 0;
  bool is_long = false;
  if (j < M) {
    u = seg_of(seg, U, M, j, s, e);
    is_long = j == s && e - s > QAGNN_ROWS_CHUNK;
  }
  unsigned long long todo = __ballot(is_long);
  while (todo) {
    const int l = __builtin_ctzll(todo);
    todo &= todo - 1;
    const int su = __builtin_amdgcn_readlane(s, l), eu = __builtin_amdgcn_readlane(e, l), uu = __builtin_amdgcn_readlane(u, l);
    if (lane < c4) {
      const int nch = (eu - su + QAGNN_ROWS_CHUNK - 1) / QAGNN_ROWS_CHUNK;
      const float* p = P + lane * 4;
      float4 acc = ld4(p + ((int64_t)2 * (su >> 6) + 1) * (c4 * 4));
#pragma unroll 4
      for (int k = 1; k < nch; ++k) acc = add4(acc, ld4(p + (int64_t)2 * ((su + k * QAGNN_ROWS_CHUNK) >> 6) * (c4 * 4)));
      st4(G + (int64_t)uu * ldg + lane * 4, acc);
    }
  }
}

// ---- scatter: one block per row of R -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rows_scatter(const float* __restrict__ R, int64_t ldr, int c4, const int64_t* __restrict__ uniq,
                                                      const int* __restrict__ count, int n_rows, float* __restrict__ out, int64_t ldo,
                                                      int64_t table_rows, int accumulate) {
  const int u = blockIdx.x;
  if (u >= clampi(*count, 0, n_rows)) return;
  const int64_t r = uniq[u];
  if (r < 0 || r >= table_rows) return;
  const float* src = R + (int64_t)u * ldr;
  float* dst = out + r * ldo;
  for (int c = threadIdx.x; c < c4; c += 256) {
    float4 v = ld4(src + c * 4);
    if (accumulate) v = add4(ld4(dst + c * 4), v);
    st4(dst + c * 4, v);
  }
}

static inline int64_t up4(int64_t x) { return (x + 3) & ~(int64_t)3; }
static inline bool rows_n_ok(int64_t N) { return N >= 1 && N <= QAGNN_ROWS_MAX_N; }

}  // namespace qagnn

using namespace qagnn;

extern "C" int qagnn_rows_version(void) { return 1; }

// workspace of qagnn_row_groups, int32 words: pos [up4(N)] | hist [nblk][RG_BUCKETS] | total [RG_BUCKETS] | start0, start1 [RG_BUCKETS + 4]
extern "C" int64_t qagnn_row_groups_workspace_elems(int32_t N) {
  if (!rows_n_ok(N)) return 0;
  const int64_t nblk = (N + RG_BLK - 1) / RG_BLK;
  return up4(N) + nblk * RG_BUCKETS + RG_BUCKETS + 2 * (RG_BUCKETS + 4);
}

extern "C" int qagnn_row_groups(const int64_t* ridx, int32_t N, int64_t table_rows, int32_t* order, int32_t* seg, int64_t* uniq, int32_t* count,
                                int32_t* workspace, int64_t ws_elems, qagnn_stream_t stream) {
  QAGNN_REQUIRE(ridx && order && seg && uniq && count && workspace, QAGNN_EINVAL, "row_groups: a NULL pointer");
  QAGNN_REQUIRE(rows_n_ok(N), QAGNN_EINVAL, "row_groups: N=%d must be in 1..%d", N, QAGNN_ROWS_MAX_N);
  QAGNN_REQUIRE(table_rows >= 1 && table_rows <= QAGNN_ROWS_MAX_TABLE, QAGNN_EINVAL, "row_groups: table_rows=%lld must be in 1..%d",
                (long long)table_rows, QAGNN_ROWS_MAX_TABLE);
  QAGNN_REQUIRE(ws_elems >= qagnn_row_groups_workspace_elems(N) && aligned16(workspace), QAGNN_EINVAL,
                "row_groups: the workspace needs %lld int32 words (got %lld) and 16-byte alignment", (long long)qagnn_row_groups_workspace_elems(N),
                (long long)ws_elems);
  hipStream_t st = (hipStream_t)stream;
  const int nblk = (N + RG_BLK - 1) / RG_BLK;
  int* const pos = workspace;
  int* const hist = pos + up4(N);
  int* const total = hist + (int64_t)nblk * RG_BUCKETS;
  int* const start0 = total + RG_BUCKETS;
  int* const start1 = start0 + RG_BUCKETS + 4;
  // low digit: the positions themselves -> pos, M = start0[RG_BUCKETS] of them
  k_rg_hist<0><<<nblk, 256, 0, st>>>(ridx, nullptr, nullptr, N, table_rows, hist);
  QAGNN_LAUNCH_CHECK("k_rg_hist<0>");
  k_rg_colscan<<<RG_BUCKETS / 256, 256, 0, st>>>(hist, total, nblk);
  QAGNN_LAUNCH_CHECK("k_rg_colscan");
  k_rg_scan<<<1, 1024, 0, st>>>(total, start0);
  QAGNN_LAUNCH_CHECK("k_rg_scan");
  k_rg_scatter<0><<<nblk, 64, 0, st>>>(ridx, nullptr, nullptr, N, table_rows, hist, start0, pos);
  QAGNN_LAUNCH_CHECK("k_rg_scatter<0>");
  // high digit: pos -> order
  const int* const m_dev = start0 + RG_BUCKETS;
  k_rg_hist<1><<<nblk, 256, 0, st>>>(ridx, pos, m_dev, N, table_rows, hist);
  QAGNN_LAUNCH_CHECK("k_rg_hist<1>");
  k_rg_colscan<<<RG_BUCKETS / 256, 256, 0, st>>>(hist, total, nblk);
  QAGNN_LAUNCH_CHECK("k_rg_colscan");
  k_rg_scan<<<1, 1024, 0, st>>>(total, start1);
  QAGNN_LAUNCH_CHECK("k_rg_scan");
  k_rg_scatter<1><<<nblk, 64, 0, st>>>(ridx, pos, m_dev, N, table_rows, hist, start1, order);
  QAGNN_LAUNCH_CHECK("k_rg_scatter<1>");
  k_rg_segments<<<1, 1024, 0, st>>>(ridx, order, m_dev, N, seg, uniq, count);
  QAGNN_LAUNCH_CHECK("k_rg_segments");
  return QAGNN_OK;
}

static inline bool seg_cols_ok(int32_t cols) { return cols >= 4 && cols <= 256 && cols % 4 == 0; }

// two partial rows per tile of 64 slots
extern "C" int64_t qagnn_row_segment_sum_workspace_elems(int32_t N, int32_t cols) {
  if (!rows_n_ok(N) || !seg_cols_ok(cols)) return 0;
  return (int64_t)2 * ((N + 63) / 64) * cols;
}

extern "C" int qagnn_row_segment_sum_f32(const float* X, int64_t ldx, int32_t cols, const int32_t* order, const int32_t* seg, const int32_t* count,
                                         int32_t N, float* G, int64_t ldg, int32_t g_rows, float* workspace, int64_t ws_elems,
                                         qagnn_stream_t stream) {
  QAGNN_REQUIRE(X && order && seg && count && G && workspace, QAGNN_EINVAL, "row_segment_sum: a NULL pointer");
  QAGNN_REQUIRE(rows_n_ok(N) && g_rows >= 1 && g_rows <= N, QAGNN_EINVAL, "row_segment_sum: N=%d must be in 1..%d and g_rows=%d in 1..N", N,
                QAGNN_ROWS_MAX_N, g_rows);
  QAGNN_REQUIRE(seg_cols_ok(cols), QAGNN_EINVAL, "row_segment_sum: cols=%d must be a multiple of 4 in 4..256", cols);
  QAGNN_REQUIRE(ldx >= cols && ldg >= cols && ldx % 4 == 0 && ldg % 4 == 0 && aligned16(X) && aligned16(G), QAGNN_EINVAL,
                "row_segment_sum: the pitches ldx=%lld, ldg=%lld must be multiples of 4 and >= cols=%d, X and G 16-byte aligned", (long long)ldx,
                (long long)ldg, cols);
  QAGNN_REQUIRE(ws_elems >= qagnn_row_segment_sum_workspace_elems(N, cols) && aligned16(workspace), QAGNN_EINVAL,
                "row_segment_sum: the workspace needs %lld floats (got %lld) and 16-byte alignment",
                (long long)qagnn_row_segment_sum_workspace_elems(N, cols), (long long)ws_elems);
  hipStream_t st = (hipStream_t)stream;
  const int grid = ((N + 63) / 64 + RS_WAVES - 1) / RS_WAVES;
  k_seg_partial<<<grid, 64 * RS_WAVES, 0, st>>>(X, ldx, cols / 4, order, seg, count, N, G, ldg, g_rows, workspace);
  QAGNN_LAUNCH_CHECK("k_seg_partial");
  k_seg_final<<<grid, 64 * RS_WAVES, 0, st>>>(cols / 4, seg, count, N, G, ldg, g_rows, workspace);
  QAGNN_LAUNCH_CHECK("k_seg_final");
  return QAGNN_OK;
}

extern "C" int qagnn_rows_scatter_f32(const float* R, int64_t ldr, int32_t cols, const int64_t* uniq, const int32_t* count, int32_t n_rows,
                                      float* out, int64_t ldo, int64_t table_rows, int32_t accumulate, qagnn_stream_t stream) {
  QAGNN_REQUIRE(R && uniq && count && out, QAGNN_EINVAL, "rows_scatter: a NULL pointer");
  QAGNN_REQUIRE(rows_n_ok(n_rows) && table_rows >= 1, QAGNN_EINVAL, "rows_scatter: n_rows=%d must be in 1..%d and table_rows=%lld >= 1", n_rows,
                QAGNN_ROWS_MAX_N, (long long)table_rows);
  QAGNN_REQUIRE(cols >= 4 && cols % 4 == 0 && ldr >= cols && ldo >= cols && ldr % 4 == 0 && ldo % 4 == 0 && aligned16(R) && aligned16(out),
                QAGNN_EINVAL, "rows_scatter: cols=%d must be a multiple of 4, the pitches ldr=%lld, ldo=%lld multiples of 4 and >= cols, R and out 16-byte aligned",
                cols, (long long)ldr, (long long)ldo);
  k_rows_scatter<<<n_rows, 256, 0, (hipStream_t)stream>>>(R, ldr, cols / 4, uniq, count, n_rows, out, ldo, table_rows, accumulate);
  QAGNN_LAUNCH_CHECK("k_rows_scatter");
  return QAGNN_OK;
}
