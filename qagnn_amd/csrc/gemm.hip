// Dense fp32 GEMMs on the CDNA4 matrix cores (v_mfma_f32_16x16x4_f32: exact fp32, 64 FLOP/clk/SIMD).
//
// These replace the cuBLAS SGEMMs the reference launches per EDGE (modeling_qagnn.py:464-466) by per-NODE
// projections (project-then-gather), plus GATConvE.mlp (:443), Vh/Vx (:92) and emb_score (:73),
// and the autograd backward of all of them.
//
// MFMA 16x16x4 f32 operand layout (wave64), from the CDNA4 ISA:
//   A: lane l holds A[i = l & 15][k = l >> 4]       B: lane l holds B[k = l >> 4][j = l & 15]
//   D: lane l, reg r holds D[row = (l >> 4) * 4 + r][col = l & 15]
//
// The slab epilogue of k_gemm_nn is the one text of gemm_device.h that k_gemm_nn_split and k_gemm_nn2 expand too.
#include <stdlib.h>

#include "gemm_device.h"

namespace qagnn {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int BK = 16;        // k-tile
constexpr int NN_BM = 128;    // rows per block (4 waves x 2 row tiles of 16)
constexpr int PA_NN = BK + 4; // LDS pitch of the row-major A tile: 16-byte aligned rows (ds_write_b128), 2-way on the 2 A reads per k-step

__host__ __device__ constexpr int pitch_b(int bn) { return (bn % 32 == 16) ? bn : bn + 16; }  // rows k, k+1 land 16 banks apart

// ------------------------------------------------------------------------------------------------------------
// NN:  C[M][No] (+)= [A1|A2] * [B1;B2] + bias + rowtab[rowidx]
// block = WAVES x 64 threads; output tile BM x (NT*16) with BM = WAVES*RT*16: wave w owns row tiles w*RT .. w*RT+RT-1 and
// all NT column tiles.  The block walks tiles blockIdx.x, blockIdx.x + gridDim.x, ... (persistent when the grid is smaller
// than the tile count): the row stores of tile t are fire-and-forget, so they drain to HBM under the MFMAs of tile t+1.
// Two shapes are instantiated: <4 waves, RT=2> (one tile per block, the original mapping) and <8 waves, RT=1> (same
// 128-row tile shared by 8 waves, launched persistent).
// ------------------------------------------------------------------------------------------------------------
template <int V> struct ic { static constexpr int value = V; };  // compile-time buffer index for generic lambdas

// Scheduling shape of one unrolled k-tile (4 k-steps of NM MFMAs each, fragments read from LDS): the fragment reads of
// k-step kk+1 are interleaved 1 : 2 with the MFMAs of k-step kk, so an MFMA never waits on a read issued just before it
// (hipcc's own order is read -> lgkmcnt(0) -> 2 MFMAs, which exposes one LDS latency per MFMA pair).  Speed only: +2-3 % on
// the TN strip kernel (90 registers, room for the fragments in flight); the NN kernel sits at its 128-register cap and loses.
template <int NM>
__device__ __forceinline__ void sched_ktile_pipeline() {
  constexpr int DS = 0x100, MFMA = 0x008, NR = (NM + 1) / 2 + 1;  // ds_read(2) instructions per k-step incl. the A fragment
#pragma unroll
  for (int r = 0; r < NR; ++r) __builtin_amdgcn_sched_group_barrier(DS, 1, 0);
#pragma unroll
  for (int kk = 0; kk < 3; ++kk) {
#pragma unroll
    for (int t = 0; t < NR; ++t) {
      __builtin_amdgcn_sched_group_barrier(MFMA, 2, 0);
      __builtin_amdgcn_sched_group_barrier(DS, 1, 0);
    }
  }
  __builtin_amdgcn_sched_group_barrier(MFMA, 2 * NR, 0);
}

// Register budget: QAGNN_NN_OCC co-resident blocks per CU (LDS allows 2).  The budget is a trade: 2 blocks per CU let one
// block's epilogue stores overlap the other's MFMAs, but cap a wave at 512 / (OCC * WAVES / 4) registers.
#if QAGNN_NN_OCC > 0
#define QAGNN_NN_ATTR __attribute__((amdgpu_waves_per_eu(QAGNN_NN_OCC * WAVES / 4, QAGNN_NN_OCC * WAVES / 4)))
#else
#define QAGNN_NN_ATTR
#endif

template <int NT, bool AFFINE, int WAVES, int RT>
__global__ __launch_bounds__(WAVES * 64) QAGNN_NN_ATTR void k_gemm_nn(qagnn_gemm_nn_args a, int ntiles) {
  constexpr int NTHR = WAVES * 64, BM = WAVES * RT * 16;
  constexpr int BN = NT * 16;
  constexpr int PB = pitch_b(BN);
  constexpr int B_F4 = BK * BN / 4;                 // float4 per B tile
  constexpr int B_IT = (B_F4 + NTHR - 1) / NTHR;
  // one LDS array: the k-loop tiles (A BM x 20, B 16 x PB) and, afterwards, the epilogue staging slabs (one per wave)
  constexpr int PS = BN + 4;                        // staging pitch: PS % 8 == 4 -> the 4 row groups of a store land 16 banks apart
  constexpr int SLAB_ROWS = WAVES <= 4 ? 16 : 8;    // rows a wave transposes at a time (keeps 8 waves inside 64 KB)
  constexpr int SUB = 16 / SLAB_ROWS;
  constexpr int A_F = BM * PA_NN, B_F = BK * PB, BUF_F = A_F + B_F;
  constexpr int KLOOP_F = 2 * BUF_F, STAGE_F = WAVES * SLAB_ROWS * PS;   // double-buffered k-tiles | epilogue slabs
  __shared__ __attribute__((aligned(16))) float smem[KLOOP_F > STAGE_F ? KLOOP_F : STAGE_F];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ncb = (a.No + BN - 1) / BN;
  const int nk1 = a.K1 / BK, nkt = nk1 + a.K2 / BK;
  const int ar = tid >> 2, ac4 = tid & 3;  // A tile: NTHR/4 rows x 4 float4 per pass, RT passes

  for (int vb = blockIdx.x; vb < ntiles; vb += gridDim.x) {
    // Workgroup b runs on XCD b % 8 (observed; speed only), so tiles are re-indexed with xcd_remap(): each XCD gets a
    // CONTIGUOUS range of tiles, and the column blocks of one row block (consecutive tile ids) read their shared A rows
    // through ONE L2 instead of up to three.  (gridDim.x is a multiple of 8 or equals ntiles, so vb % 8 is the XCD too.)
    const int tile = a.xcd_remap ? xcd_remap(vb, ntiles) : vb;
    const int m0 = (tile / ncb) * BM, n0 = (tile % ncb) * BN;

    f32x4 acc[RT][NT];
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    float4 raS[2][RT];
    float4 rb[B_IT];
    int64_t arow[RT];  // source row of A1 for this thread's tile rows (gathered or identity); -1 = zero row
#pragma unroll
    for (int p = 0; p < RT; ++p) {
      const int row = m0 + ar + p * (NTHR / 4);
      arow[p] = row < a.M ? (a.a_rowidx ? a.a_rowidx[row] : (int64_t)row) : -1;
    }

    // global -> register staging.  A (the HBM stream: 64-byte row segments, ~2 us under load) is fetched TWO k-tiles ahead
    // into alternating register sets; B (weights, L2-resident) one k-tile ahead.  B is issued before the younger A loads so
    // that the in-order vmcnt wait in front of the LDS store leaves exactly the A loads of tile kt+2 in flight.
    // Every load is unconditional (addresses clamped into the operand; rows >= M and columns >= No only ever feed
    // accumulator rows / columns that are never stored): with branches around the loads hipcc falls back to vmcnt(0).
    auto gloadA = [&](int kt, float4 (&dst)[RT]) {
      const bool first = kt < nk1;
      const float* A = first ? a.A1 : a.A2;
      const int lda = first ? a.lda1 : a.lda2;
      const int k0 = (first ? kt : kt - nk1) * BK;
#pragma unroll
      for (int p = 0; p < RT; ++p) {
        const int64_t srow = first ? (arow[p] >= 0 ? arow[p] : 0) : (int64_t)min(m0 + ar + p * (NTHR / 4), a.M - 1);
        dst[p] = ld4(A + srow * lda + k0 + ac4 * 4);
      }
    };
    auto gloadB = [&](int kt) {
      const bool first = kt < nk1;
      const float* B = first ? a.B1 : a.B2;
      const int ldb = first ? a.ldb1 : a.ldb2;
      const int k0 = (first ? kt : kt - nk1) * BK;
#pragma unroll
      for (int it = 0; it < B_IT; ++it) {
        const int idx = min(tid + it * NTHR, B_F4 - 1);
        const int kr = idx / (BN / 4), c4 = idx % (BN / 4);
        rb[it] = ld4(B + (int64_t)(k0 + kr) * ldb + min(n0 + c4 * 4, a.No - 4));
      }
    };
    auto lstore = [&](auto bufc, int kt, const float4 (&src)[RT]) {  // tile kt -> LDS buffer buf (BN affine + ReLU applied here)
      constexpr int buf = decltype(bufc)::value;
      float* As = smem + buf * BUF_F;
      float* Bs = As + A_F;
#pragma unroll
      for (int p = 0; p < RT; ++p) {
        float4 v = src[p];
        if (AFFINE && kt < nk1) {
          const int k0 = kt * BK;
          const float4 sc = ld4(a.a_scale + k0 + ac4 * 4), sh = ld4(a.a_shift + k0 + ac4 * 4);
          v.x = floor_nan(fmaf(v.x, sc.x, sh.x), 0.f);
          v.y = floor_nan(fmaf(v.y, sc.y, sh.y), 0.f);
          v.z = floor_nan(fmaf(v.z, sc.z, sh.z), 0.f);
          v.w = floor_nan(fmaf(v.w, sc.w, sh.w), 0.f);
        }
        if (a.a_rowidx && kt < nk1 && arow[p] < 0) v = make_float4(0.f, 0.f, 0.f, 0.f);  // gathered "-1" rows are zero rows
        st4(As + (ar + p * (NTHR / 4)) * PA_NN + ac4 * 4, v);
      }
#pragma unroll
      for (int it = 0; it < B_IT; ++it) {
        const int idx = tid + it * NTHR;
        if (idx < B_F4) {
          const int kr = idx / (BN / 4), c4 = idx % (BN / 4);
          st4(Bs + kr * PB + c4 * 4, rb[it]);
        }
      }
    };
    const float* const Aw = smem + (w * RT * 16 + (lane & 15)) * PA_NN + (lane >> 4);
    const float* const Bw = smem + A_F + (lane >> 4) * PB + (lane & 15);
    auto ktile = [&](auto curc, int kt) {  // cur = kt & 1 names both the LDS buffer of tile kt and the A register set of tile kt+2
      constexpr int cur = decltype(curc)::value;
      gloadB(min(kt + 1, nkt - 1));               // past the last tile: a redundant reload, never consumed
      gloadA(min(kt + 2, nkt - 1), raS[cur]);
      __builtin_amdgcn_sched_barrier(0);  // keep the loads up here: the scheduler otherwise sinks them next to the LDS store
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        float av[RT];
#pragma unroll
        for (int i = 0; i < RT; ++i) av[i] = Aw[cur * BUF_F + i * 16 * PA_NN + kk * 4];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const float bv = Bw[cur * BUF_F + kk * 4 * PB + j * 16];
#pragma unroll
          for (int i = 0; i < RT; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv, acc[i][j], 0, 0, 0);
        }
      }
      lstore(ic<cur ^ 1>{}, min(kt + 1, nkt - 1), raS[cur ^ 1]);  // after the MFMAs: the loads had one k-tile (B) / two (A) to land
      __syncthreads();
    };

    // double-buffered k-loop, ONE barrier per k-tile (it publishes tile kt+1 and retires everybody's reads of tile kt)
    gloadA(0, raS[0]);
    gloadB(0);
    gloadA(min(1, nkt - 1), raS[1]);
    __syncthreads();  // the previous output tile's slab reads are done before the k-loop buffers are overwritten
    lstore(ic<0>{}, 0, raS[0]);
    __syncthreads();
    for (int kt = 0; kt < nkt; kt += 2) {
      ktile(ic<0>{}, kt);
      if (kt + 1 < nkt) ktile(ic<1>{}, kt + 1);
    }

    // epilogue: SLAB_ROWS rows at a time through the wave's private LDS slab, then whole-row 16-byte stores (gemm_device.h)
    float* const St = smem + w * SLAB_ROWS * PS;
#pragma unroll
    for (int i = 0; i < RT; ++i) {
#pragma unroll
      for (int h = 0; h < SUB; ++h) {
        __syncthreads();  // k-loop reads (first pass) / the previous pass's slab reads are done before the slab is overwritten
        const int lr0 = (lane >> 4) * 4 - h * SLAB_ROWS;  // this lane's first row inside the slab (in range for its half only)
        if (lr0 >= 0 && lr0 < SLAB_ROWS) { QAGNN_NN_SLAB_FILL(acc[i], lr0) }
        __syncthreads();
        QAGNN_NN_SLAB_STORE(m0 + (w * RT + i) * 16 + h * SLAB_ROWS, a.M, a.No)
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------
// TN:  P[chunk][Ka][No] = sum over the chunk's rows of A[r][ka] * B[r][no]; a second kernel sums the chunks in order.
// One WAVE per 16-row tile of the output: the block has NW = blockDim.x / 64 waves and owns BM = 16*NW output rows x
// NT*16 columns, so the host picks NW to tile Ka exactly (Ka = 208 -> 13 waves, 112 -> 7, 1024 -> 16): no MFMA is
// spent on tile padding (the previous fixed 64-row tile wasted 19 % on 208).  With BM = 16*NW the A k-tile is exactly
// one float4 per thread.  k-tiles of 16 rows, double-buffered, one barrier per tile.
// ------------------------------------------------------------------------------------------------------------
__host__ __device__ constexpr int pitch16(int w) { return (w % 32 == 16) ? w : w + 16; }  // rows k, k+1 land 16 banks apart

template <int NT, bool AFFINE>
__global__ __launch_bounds__(1024) void k_gemm_tn(const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb,
                                                  float* __restrict__ P, int R, int Ka, int No, const float* __restrict__ a_scale,
                                                  const float* __restrict__ a_shift, const int64_t* __restrict__ a_rowidx,
                                                  float* __restrict__ Pcs, const int64_t* __restrict__ b_rowidx, int groups,
                                                  int chunk_rows) {
  constexpr int BN = NT * 16;
  constexpr int PB = pitch_b(BN);
  constexpr int B_F4 = BK * BN / 4;
  constexpr int B_IT = (NT + 3) / 4;  // float4 of the B tile per thread when the block has >= 4 waves (fewer waves: loop below)
  extern __shared__ __attribute__((aligned(16))) float smem_tn[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nthr = blockDim.x, BM = (nthr >> 6) * 16;
  const int PA = pitch16(BM), TA_F = BK * PA, TBUF_F = TA_F + BK * PB + BK;  // + 16 group ids of the tile's rows
  // optional by-product: column sums of B (per row group) taken from the B tiles already sitting in LDS
  const bool do_cs = Pcs != nullptr && blockIdx.y == 0 && tid < BN;
  float cs0 = 0.f, cs1 = 0.f, cs2 = 0.f, cs3 = 0.f;
  int rg = 0;  // group id of tile row `tid` (threads 0..15), staged through LDS with the tile
  const int n0 = blockIdx.x * BN, m0 = blockIdx.y * BM, chunk = blockIdx.z;
  const int r_beg = chunk * chunk_rows, r_end = min(R, r_beg + chunk_rows);
  const int nkt = (r_end - r_beg + BK - 1) / BK;

  f32x4 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float4 ra, rb[B_IT];
  const int a_f4 = BM / 4;                       // float4 per A tile row; 16 * a_f4 == nthr
  const int akr = tid / a_f4, ac4 = tid % a_f4;  // this thread's (k row, float4 column) of the A tile
  const int acol = m0 + ac4 * 4;
  float4 a_sc = make_float4(0.f, 0.f, 0.f, 0.f), a_sh = a_sc;  // the thread's A columns never change: load the BN affine once
  if (AFFINE && acol < Ka) { a_sc = ld4(a_scale + acol); a_sh = ld4(a_shift + acol); }

  auto gload = [&](int kt) {
    const int r0 = r_beg + kt * BK;
    {
      const int row = r0 + akr;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      const int64_t srow = (row < r_end && acol < Ka) ? (a_rowidx ? a_rowidx[row] : (int64_t)row) : -1;
      if (srow >= 0) {
        v = ld4(A + srow * lda + acol);
        if (AFFINE) {
          v.x = floor_nan(fmaf(v.x, a_sc.x, a_sh.x), 0.f);
          v.y = floor_nan(fmaf(v.y, a_sc.y, a_sh.y), 0.f);
          v.z = floor_nan(fmaf(v.z, a_sc.z, a_sh.z), 0.f);
          v.w = floor_nan(fmaf(v.w, a_sc.w, a_sh.w), 0.f);
        }
      }
      ra = v;
    }
#pragma unroll
    for (int it = 0; it < B_IT; ++it) {
      const int idx = tid + it * nthr;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (idx < B_F4) {
        const int kr = idx / (BN / 4), c4 = idx % (BN / 4);
        const int row = r0 + kr, col = n0 + c4 * 4;
        if (row < r_end && col < No) v = ld4(B + (int64_t)row * ldb + col);
      }
      rb[it] = v;
    }
    if (Pcs && b_rowidx && tid < BK) rg = (r0 + tid < r_end) ? (int)b_rowidx[r0 + tid] : 0;
  };
  auto lstore = [&](int buf) {
    float* As = smem_tn + buf * TBUF_F;
    float* Bs = As + TA_F;
    if (Pcs && tid < BK) reinterpret_cast<int*>(Bs + BK * PB)[tid] = rg;
    st4(As + akr * PA + ac4 * 4, ra);
#pragma unroll
    for (int it = 0; it < B_IT; ++it) {
      const int idx = tid + it * nthr;
      if (idx < B_F4) {
        const int kr = idx / (BN / 4), c4 = idx % (BN / 4);
        st4(Bs + kr * PB + c4 * 4, rb[it]);
      }
    }
  };
  auto mma = [&](int buf, int kk) {
    const float* Aw = smem_tn + buf * TBUF_F + (lane >> 4) * PA + w * 16 + (lane & 15);
    const float* Bw = smem_tn + buf * TBUF_F + TA_F + (lane >> 4) * PB + (lane & 15);
    const float av = Aw[kk * 4 * PA];
#pragma unroll
    for (int j = 0; j < NT; ++j)
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, Bw[kk * 4 * PB + j * 16], acc[j], 0, 0, 0);
  };
  auto colsum_tile = [&](int buf) {  // thread `tid` owns column tid of the B tile; rows in tile order = row order
    const float* Bs = smem_tn + buf * TBUF_F + TA_F;
    const int* grp = reinterpret_cast<const int*>(Bs + BK * PB);
#pragma unroll
    for (int k = 0; k < BK; ++k) {
      const float v = Bs[k * PB + tid];
      const int g = groups > 1 ? grp[k] : 0;
      if (g == 0) cs0 += v;
      else if (g == 1) cs1 += v;
      else if (g == 2) cs2 += v;
      else cs3 += v;
    }
  };

  if (nkt > 0) {
    gload(0);
    lstore(0);
  }
  __syncthreads();
  for (int kt = 0; kt < nkt; ++kt) {
    const int cur = kt & 1;
    const bool more = kt + 1 < nkt;
    if (more) gload(kt + 1);
    mma(cur, 0);
    mma(cur, 1);
    if (do_cs) colsum_tile(cur);
    mma(cur, 2);
    mma(cur, 3);
    if (more) lstore(cur ^ 1);  // as late as possible: the global loads get the whole tile's MFMA time to land
    __syncthreads();
  }
  if (do_cs && n0 + tid < No) {
    float* pc = Pcs + (int64_t)chunk * groups * No + n0 + tid;
    pc[0] = cs0;
    if (groups > 1) pc[No] = cs1;
    if (groups > 2) pc[2 * No] = cs2;
    if (groups > 3) pc[3 * No] = cs3;
  }
  float* Pc = P + (int64_t)chunk * Ka * No;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = m0 + w * 16 + (lane >> 4) * 4 + r;
    if (row >= Ka) continue;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int col = n0 + j * 16 + (lane & 15);
      if (col < No) Pc[(int64_t)row * No + col] = acc[j][r];
    }
  }
}

// ------------------------------------------------------------------------------------------------------------
// TN, compile-time strip shape: the k_gemm_tn mapping (wave w owns output rows 16w .. 16w+15 and all NT column tiles)
// with the wave count NWT fixed at compile time and the two LDS buffers addressed by constants (k-loop unrolled by two),
// so every LDS fragment read is `base VGPR + immediate` and the k-loop carries no address arithmetic: the run-time
// version spends 2-4 VALU instructions per MFMA on addresses and sits at ~48 % MFMA-busy.
// ------------------------------------------------------------------------------------------------------------
template <int NT, int NWT, bool AFFINE, bool COLSUM>
__global__ __launch_bounds__(NWT * 64) void k_gemm_tn_strip(const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb,
                                                            float* __restrict__ P, int R, int Ka, int No,
                                                            const float* __restrict__ a_scale, const float* __restrict__ a_shift,
                                                            const int64_t* __restrict__ a_rowidx, int chunk_rows,
                                                            float* __restrict__ Pcs, const int64_t* __restrict__ b_rowidx, int groups) {
  constexpr int NTHR = NWT * 64, BM = NWT * 16;
  constexpr int BN = NT * 16;
  constexpr int PA = pitch16(BM), PB = pitch_b(BN);
  constexpr int TA_F = BK * PA, TBUF_F = TA_F + BK * PB;
  constexpr int B_F4 = BK * BN / 4, B_IT = (B_F4 + NTHR - 1) / NTHR;
  constexpr int A_F4 = BM / 4;  // float4 per A tile row; 16 * A_F4 == NTHR: one float4 per thread
  __shared__ __attribute__((aligned(16))) float smem[2 * TBUF_F];
  __shared__ int grp_s[2][BK];  // COLSUM with row groups: group id of the tile's 16 rows
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int n0 = blockIdx.x * BN, m0 = blockIdx.y * BM, chunk = blockIdx.z;
  const int r_beg = chunk * chunk_rows, r_end = min(R, r_beg + chunk_rows);
  const int nkt = (r_end - r_beg + BK - 1) / BK;

  f32x4 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float4 ra, rb[B_IT];
  const int akr = tid / A_F4, ac4 = tid % A_F4;
  const int acol = m0 + ac4 * 4;
  // optional by-product (first row block only): column sums of B per row group, taken from the B tiles sitting in LDS --
  // thread `tid` < BN owns column tid; saves the separate pass over B that a bias / type-table gradient would need
  const bool do_cs = COLSUM && blockIdx.y == 0 && tid < BN;
  float cs[4] = {0.f, 0.f, 0.f, 0.f};
  int rg = 0;

  auto gload = [&](int kt) {
    const int r0 = r_beg + kt * BK;
    {
      const int row = r0 + akr;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      const int64_t srow = (row < r_end && acol < Ka) ? (a_rowidx ? a_rowidx[row] : (int64_t)row) : -1;
      if (srow >= 0) {
        v = ld4(A + srow * lda + acol);
        if (AFFINE) {  // BN affine of these 4 columns: re-read per tile (L1 hit) rather than held in 8 registers
          const float4 a_sc = ld4(a_scale + acol), a_sh = ld4(a_shift + acol);
          v.x = floor_nan(fmaf(v.x, a_sc.x, a_sh.x), 0.f);
          v.y = floor_nan(fmaf(v.y, a_sc.y, a_sh.y), 0.f);
          v.z = floor_nan(fmaf(v.z, a_sc.z, a_sh.z), 0.f);
          v.w = floor_nan(fmaf(v.w, a_sc.w, a_sh.w), 0.f);
        }
      }
      ra = v;
    }
#pragma unroll
    for (int it = 0; it < B_IT; ++it) {
      const int idx = tid + it * NTHR;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (idx < B_F4) {
        const int kr = idx / (BN / 4), c4 = idx % (BN / 4);
        const int row = r0 + kr, col = n0 + c4 * 4;
        if (row < r_end && col < No) v = ld4(B + (int64_t)row * ldb + col);
      }
      rb[it] = v;
    }
    if (COLSUM && b_rowidx && tid < BK) rg = (r0 + tid < r_end) ? (int)b_rowidx[r0 + tid] : 0;
  };
  float* const a_dst = smem + akr * PA + ac4 * 4;
  auto lstore = [&](auto bufc) {
    constexpr int buf = decltype(bufc)::value;
    if (COLSUM && tid < BK) grp_s[buf][tid] = rg;
    st4(a_dst + buf * TBUF_F, ra);
#pragma unroll
    for (int it = 0; it < B_IT; ++it) {
      const int idx = tid + it * NTHR;
      if (idx < B_F4) {
        const int kr = idx / (BN / 4), c4 = idx % (BN / 4);
        st4(smem + buf * TBUF_F + TA_F + kr * PB + c4 * 4, rb[it]);
      }
    }
  };
  const float* const a_frag = smem + (lane >> 4) * PA + w * 16 + (lane & 15);
  const float* const b_frag = smem + TA_F + (lane >> 4) * PB + (lane & 15);
  auto ktile = [&](auto curc, int kt) {
    constexpr int cur = decltype(curc)::value;
    const bool more = kt + 1 < nkt;
    if (more) gload(kt + 1);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const float av = a_frag[cur * TBUF_F + kk * 4 * PA];
      float bv[NT];
#pragma unroll
      for (int j = 0; j < NT; ++j) bv[j] = b_frag[cur * TBUF_F + kk * 4 * PB + j * 16];
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[j], acc[j], 0, 0, 0);
    }
    sched_ktile_pipeline<NT>();
    if (do_cs) {  // rows in tile order = row order: the summation order is fixed
      const float* Bs = smem + cur * TBUF_F + TA_F + tid;
#pragma unroll
      for (int kq = 0; kq < BK; ++kq) {
        const float v = Bs[kq * PB];
        const int g = groups > 1 ? grp_s[cur][kq] : 0;
        if (g == 0) cs[0] += v;
        else if (g == 1) cs[1] += v;
        else if (g == 2) cs[2] += v;
        else cs[3] += v;
      }
    }
    if (more) lstore(ic<cur ^ 1>{});  // as late as possible: the global loads get the whole tile's MFMA time to land
    __syncthreads();
  };

  if (nkt > 0) {
    gload(0);
    lstore(ic<0>{});
  }
  __syncthreads();
  for (int kt = 0; kt < nkt; kt += 2) {
    ktile(ic<0>{}, kt);
    if (kt + 1 < nkt) ktile(ic<1>{}, kt + 1);
  }
  if (do_cs && n0 + tid < No) {
    float* pc = Pcs + (int64_t)chunk * groups * No + n0 + tid;
    pc[0] = cs[0];
    if (groups > 1) pc[No] = cs[1];
    if (groups > 2) pc[2 * No] = cs[2];
    if (groups > 3) pc[3 * No] = cs[3];
  }
  float* Pc = P + (int64_t)chunk * Ka * No;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = m0 + w * 16 + (lane >> 4) * 4 + r;
    if (row >= Ka) continue;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int col = n0 + j * 16 + (lane & 15);
      if (col < No) Pc[(int64_t)row * No + col] = acc[j][r];
    }
  }
}

__global__ void k_sum_chunks(const float* __restrict__ P, float* __restrict__ C, int ldc, int Ka, int No, int nchunks,
                             int accumulate) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)Ka * No) return;
  const int row = (int)(i / No), col = (int)(i % No);
  float s = 0.f;
#pragma unroll 8
  for (int c = 0; c < nchunks; ++c) s += P[(int64_t)c * Ka * No + i];
  float* d = C + (int64_t)row * ldc + col;
  *d = accumulate ? *d + s : s;
}

// Same reduction, latency-shaped: a thread owns one float4 column, the block's 16 waves split the chunks (wave g takes chunks g,
// g+16, ...) and every wave issues FOUR of its loads back to back before it adds anything, so the ~84 partials of a 64 000-row
// weight gradient are fetched in two round trips per thread instead of five (the partials were written by the kernel in front and
// sit in L2 / Infinity Cache: the kernel is bound by load latency, not by bytes -- it ran at 1.5 TB/s with 2 loads in flight
// over 8 waves: profiles/r2_run60_by_shape.txt).  The 16 partial sums meet in LDS and are added in wave order.  The summation
// order is fixed by (nchunks), never by timing.
constexpr int SC_G = 16;
__global__ __launch_bounds__(SC_G * 64) void k_sum_chunks4(const float* __restrict__ P, float* __restrict__ C, int ldc, int Ka, int No,
                                                           int nchunks, int accumulate) {
  __shared__ float4 part[SC_G][64];
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int64_t n4 = (int64_t)Ka * No / 4, i4 = (int64_t)blockIdx.x * 64 + lane;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i4 < n4) {
    const float4* src = reinterpret_cast<const float4*>(P) + i4;
    for (int c0 = g; c0 < nchunks; c0 += 4 * SC_G) {
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = src[(int64_t)min(c0 + u * SC_G, nchunks - 1) * n4];  // clamped: unconditional, in flight together
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (c0 + u * SC_G < nchunks) s = add4(s, v[u]);
    }
  }
  part[g][lane] = s;
  __syncthreads();
  if (g == 0 && i4 < n4) {
    float4 t = part[0][lane];
#pragma unroll
    for (int k = 1; k < SC_G; ++k) t = add4(t, part[k][lane]);
    const int64_t e = i4 * 4;
    float* d = C + (e / No) * ldc + (e % No);
    if (accumulate) t = add4(t, ld4(d));
    st4(d, t);
  }
}

// k_sum_chunks4 for the live-tile form of k_gemm_tn_ws (common.h: tn_work): P holds S tiles [Ka][208] -- the cK partials of the K
// columns, the cK of the Q columns, the cM of the M columns -- and a float4 of C sums the tiles of its column block in slot order, with
// the association of k_sum_chunks4 (wave g takes slots g, g + 16, ...; the waves' sums added in wave order).  The counts come from the
// device's live-tile count through the function the producing kernel used.
__global__ __launch_bounds__(SC_G * 64) void k_sum_chunks4_live(const float* __restrict__ P, float* __restrict__ C, int ldc, int Ka, TnLive lv,
                                                                int accumulate) {
  __shared__ float4 part[SC_G][64];
  constexpr int BC = TN_LIVE_BC, No = 3 * BC;
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int64_t n4 = (int64_t)Ka * No / 4, i4 = (int64_t)blockIdx.x * 64 + lane;
  const TnWork w = tn_work(lv.S, lv.T, lv.n_live[0], lv.chunk_tiles);
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i4 < n4) {
    const int64_t e = i4 * 4;
    const int row = (int)(e / No), col = (int)(e % No), cb = col / BC, lc = col - cb * BC;
    const int first = cb == 0 ? 0 : cb == 2 ? w.cK : 2 * w.cK, n = cb == 1 ? w.cM : w.cK;  // first + n <= S: inside the workspace
    const int64_t t4 = (int64_t)Ka * BC / 4;
    const float4* src = reinterpret_cast<const float4*>(P) + (int64_t)first * t4 + ((int64_t)row * BC + lc) / 4;
    for (int c0 = g; c0 < n; c0 += 4 * SC_G) {
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = src[(int64_t)min(c0 + u * SC_G, n - 1) * t4];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (c0 + u * SC_G < n) s = add4(s, v[u]);
    }
  }
  part[g][lane] = s;
  __syncthreads();
  if (g == 0 && i4 < n4) {
    float4 t = part[0][lane];
#pragma unroll
    for (int k = 1; k < SC_G; ++k) t = add4(t, part[k][lane]);
    const int64_t e = i4 * 4;
    float* d = C + (e / No) * ldc + (e % No);
    if (accumulate) t = add4(t, ld4(d));
    st4(d, t);
  }
}

// ---- launchers: one per kernel template, shaped by the product's route (gemm_dispatch.hip) ----------------------------------------
// NN: 8-wave blocks walking the tiles persistently, QAGNN_NN_OCC (= 2) blocks per CU, XCD-aware tile order.  Measured at M = 64000
// (profiles/r1_gemm_micro.txt, r1_run23_nn_xcd_ab.txt, r1_run32_gemm_ab.txt): 10-18 % faster than one 128-row tile per 4-wave block.
int launch_nn(const NnRoute& r, const qagnn_gemm_nn_args& a, hipStream_t stream) {
  qagnn_gemm_nn_args b = a;
  b.xcd_remap = 1;
  return dispatch_int<13, 8, 7, 4, 2>(r.nt, [&](auto nt) {
    return dispatch_bool(r.affine, [&](auto aff) {
      k_gemm_nn<nt.value, aff.value, 8, 1><<<r.grid, 512, 0, stream>>>(b, r.ntiles);
      QAGNN_LAUNCH_CHECK("k_gemm_nn");
      return QAGNN_OK;
    });
  });
}

#define QAGNN_TN_ARGS p.A1, p.lda1, p.B, p.ldb, p.ws, p.R, p.Ka1, p.No, p.a_scale, p.a_shift, p.a_rowidx
int launch_tn(const TnRoute& r, const TnProduct& p, float* Pcs, hipStream_t stream) {
  return dispatch_int<13, 8, 7, 4, 2>(r.nt, [&](auto nt) {
    return dispatch_bool(r.affine, [&](auto aff) {
      // B tile loop covers B_IT * nthreads float4: needs (NT + 3) / 4 * waves * 64 >= 16 * NT * 4  <=>  waves >= 4  (tn_route)
      const size_t lds = 2 * (size_t)(BK * pitch16(r.waves * 16) + BK * pitch_b(nt.value * 16) + BK) * sizeof(float);
      k_gemm_tn<nt.value, aff.value><<<r.grid, r.waves * 64, lds, stream>>>(QAGNN_TN_ARGS, Pcs, p.b_rowidx, p.groups, r.chunk_rows);
      QAGNN_LAUNCH_CHECK("k_gemm_tn");
      return QAGNN_OK;
    });
  });
}
// compile-time strip (NT = 13 and 7 / 13 / 16 waves: every weight gradient of the stack at d = 200)
int launch_tn_strip(const TnRoute& r, const TnProduct& p, float* Pcs, hipStream_t stream) {
  return dispatch_int<7, 13, 16>(r.waves, [&](auto nw) {
    return dispatch_bool(r.colsum, [&](auto cs) {
      return dispatch_bool(r.affine, [&](auto aff) {
        k_gemm_tn_strip<13, nw.value, aff.value, cs.value><<<r.grid, nw.value * 64, 0, stream>>>(QAGNN_TN_ARGS, r.chunk_rows, Pcs, p.b_rowidx, p.groups);
        QAGNN_LAUNCH_CHECK("k_gemm_tn_strip");
        return QAGNN_OK;
      });
    });
  });
}
#undef QAGNN_TN_ARGS

int launch_sum_chunks_live(const float* P, float* C, int ldc, int rows, const TnLive& lv, int accumulate, hipStream_t stream) {
  const int64_t tot = (int64_t)rows * 3 * TN_LIVE_BC;
  k_sum_chunks4_live<<<cdiv(tot / 4, 64), SC_G * 64, 0, stream>>>(P, C, ldc, rows, lv, accumulate);
  QAGNN_LAUNCH_CHECK("k_sum_chunks4_live");
  return QAGNN_OK;
}

int launch_sum_chunks(const float* P, float* C, int ldc, int rows, int No, int nchunks, int accumulate, bool by4, hipStream_t stream) {
  const int64_t tot = (int64_t)rows * No;
  if (by4) k_sum_chunks4<<<cdiv(tot / 4, 64), SC_G * 64, 0, stream>>>(P, C, ldc, rows, No, nchunks, accumulate);
  else k_sum_chunks<<<cdiv(tot, 256), 256, 0, stream>>>(P, C, ldc, rows, No, nchunks, accumulate);
  QAGNN_LAUNCH_CHECK("k_sum_chunks");
  return QAGNN_OK;
}

}  // namespace qagnn
