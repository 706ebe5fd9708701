// Device code shared by the GEMM kernels (gemm.hip, gemm_split.hip, gemm_nn2.hip): ONE definition of what more than one kernel runs --
// the buffer load, the exact 3 x bf16 split, the prologue and the final store of the two split-K weight-gradient kernels, the slab
// epilogue of the NN kernels and its column-statistics by-product.  The kernels are at their register limit (256 VGPRs), so the
// shared pieces are shaped to compile to the code the kernels held in place: scripts/kernel_isa_diff.py compares the device assembly
// of every kernel of the three sources against another revision.
#pragma once
#include "common.h"

namespace qagnn {

// per-lane byte offset beyond any operand these kernels are launched on: the buffer load answers with zeros (+ any offset a kernel adds
// stays out of range)
constexpr uint32_t OOB = 0x80000000u;

// 16-byte load through a buffer descriptor: per-lane byte offset + wave-uniform byte offset; out of range reads return zeros
template <class V>
__device__ __forceinline__ V bload(__amdgpu_buffer_rsrc_t rsrc, uint32_t voff, uint32_t soff = 0) {
  return __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)voff, (int)soff, 0));
}

// x = h1 + h2 + h3 exactly, each h a bf16 number carried in the high half of a dword (the arithmetic: gemm_split.hip's header)
__device__ __forceinline__ void split3(uint32_t u, uint32_t& h1, uint32_t& h2, uint32_t& h3) {
  h1 = u & 0xFFFF0000u;
  const float r1 = __builtin_bit_cast(float, u) - __builtin_bit_cast(float, h1);  // exact
  h2 = __builtin_bit_cast(uint32_t, r1) & 0xFFFF0000u;
  const float r2 = r1 - __builtin_bit_cast(float, h2);  // exact, <= 8 significant bits
  h3 = __builtin_bit_cast(uint32_t, r2);                // <= 8 significant bits: the low half is already zero
}
__device__ __forceinline__ void split3(float x, uint32_t& h1, uint32_t& h2, uint32_t& h3) { split3(__builtin_bit_cast(uint32_t, x), h1, h2, h3); }
// two fp32 bit patterns whose low halves are zero -> one dword of two bf16 (element 0 = lo, in the low half)
__device__ __forceinline__ uint32_t pack_hi(uint32_t lo, uint32_t hi) { return __builtin_amdgcn_perm(hi, lo, 0x07060302u); }

// ---- the split-K weight-gradient kernels k_gemm_tn_split and k_gemm_tn_ws (gemm_split.hip) ------------------------------------------
// NP <= 2: the words holding max |A|, max |A2|, max |B| (bit patterns)
struct TnAmax { const uint32_t* a; const uint32_t* a2; const uint32_t* b; };
// The prologue of both kernels, ONE TEXT expanded in each (a __forceinline__ function that returns these values in a struct compiles to
// the same counts but not to the same code, and one for the final store regroups its address arithmetic and moves registers:
// profiles/gemm_device_code_isa.txt).  Expects the kernel's A, lda, Ka, A2, lda2, Ka2, chunk_rows, amax and the constants AC, BC, NP;
// leaves ka_total, chunk, row_shift, fa, fb, sa, sb, n0, m0, has switched (A, lda, Ka) to the block's operand and made chunk_rows positive.
// LIVE_ (k_gemm_tn_ws): the block's unit of work comes from the live-tile table LV_ and is left in `slot` (common.h: tn_work).
#define QAGNN_TN_BLOCK(LIVE_, LV_)                                                                                                       \
  const int ka_total = Ka + (A2 ? Ka2 : 0);                                                                                              \
  /* XCD-aware block order (chunk_rows < 0: off): the blocks of one chunk read the same rows of A and B, so they belong on ONE XCD,   */ \
  /* next to each other in time -- in launch order they are dealt out over all eight L2s and every operand row crosses the fabric     */ \
  /* once per block that uses it (744 MB instead of 242 MB for the two-operand product: the kernel ran at the speed of those re-reads) */ \
  int bx = blockIdx.x, by = blockIdx.y, chunk = blockIdx.z, row_shift = 0;                                                               \
  TnSlot slot = {};                                                                                                                      \
  if constexpr (LIVE_) {                                                                                                               \
    /* the row blocks of a unit are neighbours in the XCD-contiguous order, then the units in tn_slot's order (K_j, Q_j, their M ranges) */ \
    const int lin = bx + (int)gridDim.x * (by + (int)gridDim.y * chunk);                                                                 \
    const int v = xcd_remap(lin, (int)(gridDim.x * gridDim.y * gridDim.z));                                                              \
    by = v % (int)gridDim.y;                                                                                                             \
    const int L = __builtin_amdgcn_readfirstlane((LV_).n_live[0]);                                                                       \
    slot = tn_slot(tn_work((LV_).S, (LV_).T, L, (LV_).chunk_tiles), (LV_).S, (LV_).T, min(v / (int)gridDim.y, (LV_).S - 1));             \
    bx = slot.cb;                                                                                                                        \
  } else if (chunk_rows < 0) {                                                                                                           \
    chunk_rows = -chunk_rows;                                                                                                            \
  } else {                                                                                                                               \
    const int lin = bx + (int)gridDim.x * (by + (int)gridDim.y * chunk);                                                                 \
    const int v = xcd_remap(lin, (int)(gridDim.x * gridDim.y * gridDim.z));                                                              \
    bx = v % (int)gridDim.x;                                                                                                             \
    by = (v / (int)gridDim.x) % (int)gridDim.y;                                                                                          \
    chunk = v / (int)(gridDim.x * gridDim.y);                                                                                            \
  }                                                                                                                                      \
  /* Two A operands (A2 != nullptr): the product [A | A2]^T B, rows [0, Ka) of the output from A, rows [Ka, Ka + Ka2) from A2 -- the  */ \
  /* row tiles of A2 follow those of A in blockIdx.y, and such a block simply works on the other operand (one launch and one chunk    */ \
  /* sum for the two weight gradients that share dK|dM|dQ: X^T dKMQ and S^T dKMQ)                                                     */ \
  bool second = false;                                                                                                                   \
  if (A2 != nullptr) {                                                                                                                   \
    const int n1 = (Ka + AC - 1) / AC;                                                                                                   \
    if (by >= n1) { by -= n1; row_shift = Ka; A = A2; lda = lda2; Ka = Ka2; second = true; }                                             \
  }                                                                                                                                      \
  uint32_t fa = 127u, fb = 127u;                                                                                                         \
  float sa = 1.f, sb = 1.f;                                                                                                              \
  if constexpr (NP <= 2) {                                                                                                               \
    fa = __builtin_amdgcn_readfirstlane(h2_scale_field(second ? amax.a2[0] : amax.a[0]));                                                \
    fb = __builtin_amdgcn_readfirstlane(h2_scale_field(amax.b[0]));                                                                      \
    sa = h2_field_to_scale(fa);                                                                                                          \
    sb = h2_field_to_scale(fb);                                                                                                          \
  }                                                                                                                                      \
  const int n0 = bx * BC, m0 = by * AC;
// The accumulators C_ of one 16 x 16 tile (row strip, column tile of the block) -> the chunk's partial Pc (the same one text; expects Pc,
// inv, lane and the prologue's names).  OWN_TILE_: Pc is one [ka_total][BC] tile of the workspace (the live-tile form), else the chunk's
// [ka_total][No].  NP <= 2: the operand scales come out again, exactly (inv = h2_inv_scale)
#define QAGNN_TN_PUT(OWN_TILE_, STRIP_, CTILE_, C_)                                                                                      \
  _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                                                        \
    const int row = m0 + (STRIP_) * 16 + (lane >> 4) * 4 + r, col = n0 + (CTILE_) * 16 + (lane & 15);                                    \
    if (row < Ka && col < No)                                                                                                            \
      Pc[(OWN_TILE_) ? (int64_t)(row + row_shift) * BC + (col - n0) : (int64_t)(row + row_shift) * No + col] = NP <= 2 ? (C_)[r] * inv : (C_)[r]; \
  }

// ---- the slab epilogue of the NN kernels k_gemm_nn (gemm.hip), k_gemm_nn_split (gemm_split.hip), k_gemm_nn2 (gemm_nn2.hip) -----------
// The MFMA layout gives a lane ONE column of 4 rows per accumulator; storing that directly is 104 dword stores per lane in 64-byte row
// fragments (store-issue bound).  Instead each wave transposes SLAB_ROWS rows at a time through its private LDS slab St (pitch PS = BN + 4:
// PS % 8 == 4, the 4 row groups of a store land 16 banks apart) and writes whole rows with 16-byte lanes: 4x fewer store instructions,
// full 128-byte lines.  ONE TEXT again (these kernels sit at 256 VGPRs: the epilogue as a function template moved registers in every
// instantiation).  Expects the kernel's a (qagnn_gemm_nn_args), St, lane, n0 and the constants NT, BN, PS, SLAB_ROWS.
// the accumulators ACC_[NT] of one 16-row tile -> the slab; LR0_: the lane's first row inside the slab
#define QAGNN_NN_SLAB_FILL(ACC_, LR0_)                                                                                                   \
  _Pragma("unroll") for (int j = 0; j < NT; ++j)                                                                                         \
    _Pragma("unroll") for (int r = 0; r < 4; ++r) St[((LR0_) + r) * PS + j * 16 + (lane & 15)] = (ACC_)[j][r];
// the slab -> the rows ROW0_ .. of C (M_ x NO_): product + bias + table row + old value
#define QAGNN_NN_SLAB_STORE(ROW0_, M_, NO_)                                                                                              \
  {                                                                                                                                      \
    constexpr int ROW_F4 = BN / 4, TILE_F4 = SLAB_ROWS * ROW_F4, ST_IT = (TILE_F4 + 63) / 64;                                            \
    _Pragma("unroll") for (int it = 0; it < ST_IT; ++it) {                                                                               \
      const int idx = lane + it * 64;                                                                                                    \
      if (idx >= TILE_F4) break;                                                                                                         \
      const int slr = idx / ROW_F4, c4 = idx % ROW_F4;                                                                                   \
      const int row = (ROW0_) + slr, col = n0 + c4 * 4;                                                                                  \
      if (row >= (M_) || col >= (NO_)) continue;                                                                                         \
      float4 v = ld4(St + slr * PS + c4 * 4);                                                                                            \
      if (a.bias) v = add4(v, ld4(a.bias + col));                                                                                        \
      if (a.rowtab) v = add4(v, ld4(a.rowtab + (int64_t)a.rowidx[row] * a.ldt + col));                                                   \
      float* dst = a.C + (int64_t)row * a.ldc + col;                                                                                     \
      if (a.accumulate) v = add4(v, ld4(dst));                                                                                           \
      st4(dst, v);                                                                                                                       \
    }                                                                                                                                    \
  }
// STATS, the by-product of that epilogue (k_gemm_nn_split, k_gemm_nn2): per 128-row tile and output column, x0 = the tile's first value,
// S1 = sum (x - x0) and S2 = sum (x - x0)^2 over the tile's rows of C in a.colstat_part [tile][3][No] -- the BatchNorm batch statistics.
// bn_stats_finalize reads either kernel's partials, so both must give the same bits.  A lane holds the columns lane, lane + 64, ... (SC of
// them) in x0r, cs1, cs2.  One slab pass: every wave's slab is complete; S0_ = row 0 of the first slab of the 128-row tile (its first row,
// the shift of the tile's sums), FIRST_: this is the wave's first pass, ROWS_: rows of this slab inside the matrix (<= 0 past M)
#define QAGNN_NN_SLAB_STATS(S0_, FIRST_, ROWS_, NO_)                                                                                     \
  _Pragma("unroll") for (int cc = 0; cc < SC; ++cc) {                                                                                    \
    const int c = lane + cc * 64;                                                                                                        \
    if (c < BN && n0 + c < (NO_)) {                                                                                                      \
      const float bc = a.bias ? a.bias[n0 + c] : 0.f;                                                                                    \
      if (FIRST_) x0r[cc] = (S0_)[c] + bc;                                                                                               \
      const int rows = (ROWS_);                                                                                                          \
      float v[SLAB_ROWS];                                                                                                                \
      _Pragma("unroll") for (int r = 0; r < SLAB_ROWS; ++r) v[r] = St[r * PS + c]; /* 16 LDS reads in flight, then the arithmetic */     \
      _Pragma("unroll") for (int r = 0; r < SLAB_ROWS; ++r) {                                                                            \
        const float dlt = r < rows ? (v[r] + bc) - x0r[cc] : 0.f; /* the value the store loop writes, minus the shift */                 \
        cs1[cc] += dlt;                                                                                                                  \
        cs2[cc] = fmaf(dlt, dlt, cs2[cc]);                                                                                               \
      }                                                                                                                                  \
    }                                                                                                                                    \
  }
// After the passes: the waves' sums meet in cstat [wave][2][BN] and are added in wave order, one partial per 128 rows (the contract of
// colstat_part).  A block of 32-row waves holds TILES_ such tiles (its halves): thread (hw, lane) of half hf = column hw * 64 + lane of
// that half, and its own x0r[hw] is that column's shift.  HALVES_ = false says so at compile time for the block that is always one
// tile of four waves (hw = w, column = tid: k_gemm_nn_split keeps its code).  (cstat is rewritten only after the next tile's k-loop and
// slab barriers)
#define QAGNN_NN_STATS_PUT(HALVES_, TILES_, M_, NO_)                                                                                     \
  {                                                                                                                                      \
    _Pragma("unroll") for (int cc = 0; cc < SC; ++cc) {                                                                                  \
      const int c = lane + cc * 64;                                                                                                      \
      if (c < BN) { cstat[w][0][c] = cs1[cc]; cstat[w][1][c] = cs2[cc]; }                                                                \
    }                                                                                                                                    \
    __syncthreads();                                                                                                                     \
    const int hw = (HALVES_) ? w & 3 : w, hf = (HALVES_) ? w >> 2 : 0, col = (HALVES_) ? hw * 64 + lane : tid;                           \
    if (col < BN && n0 + col < (NO_) && (!(HALVES_) || m0 + hf * 128 < (M_))) {                                                          \
      float x0c = x0r[0];                                                                                                                \
      _Pragma("unroll") for (int cc = 1; cc < SC; ++cc) x0c = (hw == cc) ? x0r[cc] : x0c;                                                \
      float* const pt = a.colstat_part + ((int64_t)(tile / ncb) * (TILES_) + hf) * 3 * (NO_) + n0 + col;                                 \
      const int w0 = hf * 4;                                                                                                             \
      pt[0] = x0c;                                                                                                                       \
      pt[(NO_)] = (cstat[w0][0][col] + cstat[w0 + 1][0][col]) + (cstat[w0 + 2][0][col] + cstat[w0 + 3][0][col]);                         \
      pt[2 * (NO_)] = (cstat[w0][1][col] + cstat[w0 + 1][1][col]) + (cstat[w0 + 2][1][col] + cstat[w0 + 3][1][col]);                     \
    }                                                                                                                                    \
  }

}  // namespace qagnn
