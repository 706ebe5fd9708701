// Host side of the dense products: what stands between the GEMM entry points of include/qagnn_hip.h and the kernels of gemm.hip (fp32
// MFMA, weight gradients at run-time shapes, chunk sums), gemm_split.hip (3 x bf16 split, first generation; split weight gradients) and
// gemm_nn2.hip (second-generation NN kernel, B images); the device code those three share is in gemm_device.h.  No kernel lives here.
//
// An entry point fills a product description (NnProduct / TnProduct, common.h) and calls gemm_nn() / gemm_tn(): validate, ask
// nn_route() / tn_route() for the product's route, hand route and product to the one launcher of the kernel template it names.  The
// route is the only place where a kernel family, a tile shape, an arithmetic form, a chunking or a scratch size is chosen; the
// scratch queries below return what the route says, and hop.hip calls gemm_nn() / gemm_tn() like the entry points do.
#include <stdlib.h>

#include <atomic>
#include <initializer_list>

#include "common.h"
#include "../../include/qagnn_hip_dual.h"

namespace qagnn {

// column-tile count per block: the widest instantiation that divides No, else the one wasting the least (k_gemm_nn, k_gemm_tn)
static int pick_nt(int No) {
  const int cands[5] = {13, 7, 8, 4, 2};
  for (int c : cands)
    if (No % (c * 16) == 0) return c;
  int best = 4;
  int64_t best_cost = INT64_MAX;
  for (int c : cands) {
    const int64_t cost = (int64_t)cdiv(No, c * 16) * c * 16;
    if (cost < best_cost) { best_cost = cost; best = c; }
  }
  return best;
}

// ---- NN -----------------------------------------------------------------------------------------------------------------------------
// One process-wide threshold (qagnn_packed_min_rows: tests lower it to run small products in the packed forms): from that many rows on
// B is packed once per product wherever the caller hands over scratch, and the scaled fp16 forms pay (they need a packed image).
static std::atomic<int64_t> g_pack_min_m{8192};
bool nn_rows_packed(int64_t M) { return M >= g_pack_min_m.load(std::memory_order_relaxed); }

// what the second-generation kernel takes: 32-bit operand offsets, segments that are multiples of 8
static bool nn2_ok(const qagnn_gemm_nn_args& a, int ldn1, int ldn2) {
  const int64_t lim = (int64_t)0x7FFFFFFF;
  // (a gathered A1: the table's extent must be known and addressable with the kernels' 32-bit offsets; one segment)
  if (a.a_rowidx && !(a.a_rows > 0 && a.a_rows * (int64_t)a.lda1 * 4 < lim && a.K2 == 0)) return false;
  if (a.K1 % 8 != 0 || a.K2 % 8 != 0) return false;
  if ((int64_t)a.M * a.lda1 * 4 >= lim || (int64_t)a.No * ldn1 * 4 >= lim || (int64_t)a.M * a.ldc * 4 >= lim) return false;
  if (a.K2 > 0 && ((int64_t)a.M * a.lda2 * 4 >= lim || (int64_t)a.No * ldn2 * 4 >= lim)) return false;
  if (a.K2 > 0 && (a.K1 & 31) != 0 && a.K2 < 32 - (a.K1 & 31)) return false;  // (the straddling tile must lie inside segment 2)
  if (a.a_scale && a.K1 > 256) return false;  // (the scale / shift vectors live in LDS next to the two B images)
  return true;
}
// The staggered 8-wave block wherever a six-MFMA product on an image has at least one 256-row tile per CU.  Measured at M = 64 000
// (tools/nn2_ablate.hip, profiles/r4_run16_nn2_stagger.txt), 4-wave blocks -> staggered block: [208|112] -> 624 141 -> 122 us, 624 -> 208
// 96..101 -> 79, but 208 -> 208 38 -> 39 and 624 -> 112 (NT = 7) 53 -> 54: with one block per CU nothing runs under a tile's first loads,
// and the last tiles' stores are a tail at HBM speed, which 10 k-tiles of 13 column tiles amortise and 7 k-tiles or 7 column tiles do not.
static bool nn2_staggered(int nt, const qagnn_gemm_nn_args& a) {
  return nt >= 8 && nn2::walk_tiles(a.K1, a.K2) >= 10 && (int64_t)cdiv(a.No, nt * 16) * cdiv(a.M, 256) * 10 >= num_cus() * 9;
}

// fewer than about 1.5 blocks per CU at `nt` column tiles per block: nn_route narrows the column tile then (its comment, below)
static bool nn_few_blocks(int M, int No, int nt) { return cdiv(M, 128) * cdiv(No, nt * 16) < num_cus() * 3 / 2; }

NnRoute nn_route(const NnProduct& p) {
  const qagnn_gemm_nn_args& a = *p.a;
  NnRoute r = {};
  r.np = 3;
  r.affine = a.a_scale != nullptr;
  if (!p.split) {  // exact fp32 MFMA: persistent 8-wave blocks on 128-row tiles
    r.family = NnFamily::FP32;
    r.nt = pick_nt(a.No);
    r.wv = 8;
    nn_grid(r, a.M, a.No, 128, QAGNN_NN_OCC > 0 ? QAGNN_NN_OCC : 1);
    return r;
  }
  const int nt16 = cdiv(a.No, 16);
  r.nt = nt16 >= 13 ? 13 : nt16 >= 8 ? 8 : nt16 >= 7 ? 7 : nt16 >= 4 ? 4 : 2;
  // Few row tiles (the host-bound configurations: 10 subgraphs are 16 row tiles, a 64-subgraph MedQA shard 100, on 256 CUs): a
  // block's time is its own serial k-loop, which scales with the column tiles it carries, and the other CUs idle -- so the column
  // tile narrows until there are about 1.5 blocks per CU (or it is 32 columns wide).  Measured, rocprofv3 kernel durations
  // (profiles/r3_run5_nn_small_m.txt): 2 000 x 208 x 208 25.3 -> 9.4 us at 32 columns; 12 800 rows 27.3 -> 16.3 us at 64 columns
  // (18.6 at 32); 624 -> 208 at 12 800 rows 63 -> 37 us.  The arithmetic per output element does not depend on the tile shape:
  // results are bit-identical.
  for (int c : {7, 4, 2})
    if (nn_few_blocks(a.M, a.No, r.nt) && c < r.nt) r.nt = c;
  r.wv = 4;
  r.stats = a.colstat_part != nullptr;
  if (!nn2_ok(a, p.ldn1, p.ldn2)) {  // first generation: 4-wave blocks on 128-row tiles, two per CU
    const int64_t lim = (int64_t)0x7FFFFFFF;
    r.family = NnFamily::SPLIT;
    r.flat = a.a_rowidx || (int64_t)a.M * a.lda1 * 4 >= lim || (int64_t)a.M * a.lda2 * 4 >= lim || (int64_t)a.No * p.ldn1 * 4 >= lim ||
             (int64_t)a.No * p.ldn2 * 4 >= lim;
    nn_grid(r, a.M, a.No, 128, 2);
    return r;
  }
  r.family = NnFamily::NN2;
  // B in `np` pieces: a registered image (qagnn_gemm_nn_prepack_f32: one launch for all weights of a step), or one packed into the
  // caller's scratch (the scaled forms pass a misaligned scratch by, the six-MFMA form reports it)
  auto image = [&](int np) {
    const int64_t need = nn2_pack_bytes(a.No, a.K1, a.K2, np);
    if ((r.image = nn2_prepack_lookup(p.B1n, p.ldn1, a.K1, p.B2n, p.ldn2, a.K2, a.No, np))) r.b = NnB::IMAGE;
    else if (p.ws && nn_rows_packed(a.M) && p.ws_bytes >= need && (np == 3 || aligned16(p.ws))) { r.b = NnB::PACK; r.ws_bytes = need; }
    else return false;
    r.np = np;
    return true;
  };
  // the scaled forms where the operand maxima are known: three MFMAs per product, or one on request (pieces == 1: reduced precision);
  // 4-wave blocks at every shape (tools/nn2_ablate.hip, profiles/r6_run1_three_product_ablation.txt)
  const bool scaled = nn_rows_packed(a.M) && a.a_amax1 && (a.K2 == 0 || a.a_amax2);
  if (!(scaled && image(a.pieces == 1 ? 1 : 2)) && !image(3)) r.b = NnB::IN_KERNEL;
  if (r.b != NnB::IN_KERNEL && r.np == 3 && nn2_staggered(r.nt, a)) r.wv = 8;
  nn_grid(r, a.M, a.No, r.wv * 32, r.wv == 8 ? 1 : 2);
  return r;
}

int nn_validate(const NnProduct& p) {
  QAGNN_REQUIRE(p.a, QAGNN_EINVAL, "gemm_nn: null pointer");
  const qagnn_gemm_nn_args& a = *p.a;
  const float* B1 = p.split ? p.B1n : a.B1, *B2 = p.split ? p.B2n : a.B2;
  const int ldb1 = p.split ? p.ldn1 : a.ldb1, ldb2 = p.split ? p.ldn2 : a.ldb2, km = p.split ? 4 : 16;  // (fp32 kernel: k-tiles of 16)
  QAGNN_REQUIRE(a.A1 && B1 && a.C, QAGNN_EINVAL, "gemm_nn: null pointer");
  QAGNN_REQUIRE(a.M > 0 && a.No > 0 && a.K1 > 0, QAGNN_EINVAL, "gemm_nn: bad sizes M=%d No=%d K1=%d", a.M, a.No, a.K1);
  QAGNN_REQUIRE(a.K1 % km == 0 && a.K2 % km == 0 && a.K2 >= 0, QAGNN_EINVAL, "gemm_nn: K1=%d K2=%d must be multiples of %d", a.K1, a.K2, km);
  QAGNN_REQUIRE(a.No % 4 == 0, QAGNN_EINVAL, "gemm_nn: No=%d must be a multiple of 4", a.No);
  QAGNN_REQUIRE(a.lda1 % 4 == 0 && ldb1 % 4 == 0 && (!p.split || ldb1 >= a.K1) && aligned16(a.A1) && aligned16(B1), QAGNN_EINVAL,
                "gemm_nn: operand 1 must be 16-byte aligned with pitches multiple of 4");
  QAGNN_REQUIRE(a.K2 == 0 || (a.A2 && B2 && a.lda2 % 4 == 0 && ldb2 % 4 == 0 && (!p.split || ldb2 >= a.K2) && aligned16(a.A2) && aligned16(B2)),
                QAGNN_EINVAL, "gemm_nn: operand 2 must be 16-byte aligned with pitches multiple of 4");
  QAGNN_REQUIRE(!a.rowtab || a.rowidx, QAGNN_EINVAL, "gemm_nn: rowtab without rowidx");
  QAGNN_REQUIRE(a.ldc % 4 == 0 && aligned16(a.C) && (!a.bias || aligned16(a.bias)) && (!a.rowtab || (aligned16(a.rowtab) && a.ldt % 4 == 0)),
                QAGNN_EINVAL, "gemm_nn: C / bias / rowtab must be 16-byte aligned with pitches multiple of 4");
  QAGNN_REQUIRE(!a.a_scale || (a.a_shift && aligned16(a.a_scale) && aligned16(a.a_shift)), QAGNN_EINVAL,
                "gemm_nn: a_scale/a_shift must both be given and 16-byte aligned");
  // every pitch spans the width it strides (the fp32 route reads B as [K][ldb]; the split routes' [No][ldn] is checked above)
  QAGNN_REQUIRE(a.lda1 >= a.K1 && (a.K2 == 0 || a.lda2 >= a.K2), QAGNN_EINVAL, "gemm_nn: lda1=%d / lda2=%d below K1=%d / K2=%d", a.lda1, a.lda2,
                a.K1, a.K2);
  QAGNN_REQUIRE(p.split || (ldb1 >= a.No && (a.K2 == 0 || ldb2 >= a.No)), QAGNN_EINVAL, "gemm_nn: ldb1=%d / ldb2=%d below No=%d", ldb1, ldb2, a.No);
  QAGNN_REQUIRE(a.ldc >= a.No && (!a.rowtab || a.ldt >= a.No), QAGNN_EINVAL, "gemm_nn: ldc=%d / ldt=%d below No=%d", a.ldc, a.ldt, a.No);
  if (p.split && a.colstat_part) {
    const int64_t lim = (int64_t)0x7FFFFFFF;
    QAGNN_REQUIRE(cdiv(a.No, 16) == 13 && !a.a_scale && !a.a_rowidx && !a.rowtab && !a.accumulate && a.K2 == 0, QAGNN_EUNSUPPORTED,
                  "gemm_nn: column statistics need 193..208 output columns and a bias-only epilogue (No=%d)", a.No);
    QAGNN_REQUIRE((int64_t)a.M * a.lda1 * 4 < lim && (int64_t)a.No * ldb1 * 4 < lim, QAGNN_EUNSUPPORTED,
                  "gemm_nn: column statistics with operands of 2 GB and more");
  }
  return QAGNN_OK;
}

int gemm_nn(const NnProduct& p, hipStream_t stream) {
  TimedScope timed(0, stream);
  if (int rc = nn_validate(p)) return rc;
  const qagnn_gemm_nn_args& a = *p.a;
  const NnRoute r = nn_route(p);
  if (r.family == NnFamily::FP32) return launch_nn(r, a, stream);
  if (r.family == NnFamily::SPLIT) return launch_nn_split(r, a, p.B1n, p.ldn1, p.B2n, p.ldn2, stream);
  if (r.b == NnB::IN_KERNEL) return launch_nn2(r, a, p.B1n, p.ldn1, p.B2n, p.ldn2, stream);
  if (r.b == NnB::PACK) {
    QAGNN_REQUIRE(aligned16(p.ws), QAGNN_EINVAL, "gemm_nn: the pack workspace must be 16-byte aligned");
    if (int rc = launch_pack_b(r.np, a, p.B1n, p.ldn1, p.B2n, p.ldn2, p.ws, stream)) return rc;
  }
  return launch_nn2(r, a, static_cast<const float*>(r.b == NnB::PACK ? p.ws : r.image), cdiv(a.No, 16), nullptr, 0, stream);
}

// ---- two NN products over one A operand as one launch (include/qagnn_hip_dual.h) ---------------------------------------------------
// The switch hop.hip asks (QAGNN_NN_DUAL starts it; qagnn_nn_dual_enable moves it) and the count of launches tests read.  0: off; 1: on
// where the separate launches would keep their full 13 / 7 column tiles; 2: on at every row count the packed forms take (tests)
static std::atomic<int> g_nn_dual{-1};  // -1: not set by a call -- the environment decides
static std::atomic<int64_t> g_nn_dual_launches{0};
static int nn_dual_mode() {
  static const int env = [] { const char* e = getenv("QAGNN_NN_DUAL"); const int v = e ? atoi(e) : 1; return v < 0 ? 0 : (v > 2 ? 2 : v); }();
  const int v = g_nn_dual.load(std::memory_order_relaxed);
  return v < 0 ? env : v;
}
bool nn_dual_enabled() { return nn_dual_mode() != 0; }

// Which pairs take k_gemm_nn2_dual: the conditions of the header, in its order; p1 and p2 have passed nn_validate.  The kernel's blocks
// are 128 rows x (13 + 7) column tiles at every M, so with few row tiles (10 subgraphs' worth up to about 49 000 rows on 256 CUs) the
// launch would be a handful of long serial blocks where nn_route narrows the separate products' column tiles to fill the chip: there
// the pair keeps its two launches.
NnDualRoute nn_dual_route(const NnProduct& p1, const NnProduct& p2) {
  NnDualRoute r = {};
  if (!p1.split || !p2.split) return r;
  const qagnn_gemm_nn_args& a = *p1.a, &b = *p2.a;
  if (a.A1 != b.A1 || a.lda1 != b.lda1 || a.K1 != b.K1 || a.M != b.M || a.a_amax1 != b.a_amax1 || !a.a_amax1) return r;
  if (a.pieces == 1 || b.pieces == 1) return r;  // (the one-MFMA form stays on its two launches)
  for (const qagnn_gemm_nn_args* q : {&a, &b})
    if (q->K2 != 0 || q->bias || q->rowtab || q->a_scale || q->a_shift || q->colstat_part || q->a_rowidx) return r;
  if (cdiv(a.No, 16) != 13 || cdiv(b.No, 16) != 7) return r;
  if (!nn2_ok(a, p1.ldn1, 0) || !nn2_ok(b, p2.ldn1, 0) || !nn_rows_packed(a.M)) return r;
  if (nn_dual_mode() != 2 && (nn_few_blocks(a.M, a.No, 13) || nn_few_blocks(b.M, b.No, 7))) return r;  // (nn_route would narrow either)
  // the two-piece images: registered, or packed into the scratch one behind the other
  const NnProduct* ps[2] = {&p1, &p2};
  int64_t used = 0;
  for (int i = 0; i < 2; ++i) {
    const qagnn_gemm_nn_args& q = *ps[i]->a;
    r.d.image[i] = nn2_prepack_lookup(ps[i]->B1n, ps[i]->ldn1, q.K1, nullptr, 0, 0, q.No, 2);
    if (!r.d.image[i]) {
      const int64_t need = (nn2_pack_bytes(q.No, q.K1, 0, 2) + 15) & ~(int64_t)15;
      if (!p1.ws || !aligned16(p1.ws) || used + need > p1.ws_bytes) return r;
      r.pack[i] = true;
      r.ws_off[i] = used;
      r.d.image[i] = static_cast<const unsigned char*>(p1.ws) + used;
      used += need;
    }
  }
  r.d.A = a.A1; r.d.lda = a.lda1; r.d.K = a.K1; r.d.M = a.M; r.d.a_amax = a.a_amax1;
  r.d.C[0] = a.C; r.d.ldc[0] = a.ldc; r.d.No[0] = a.No; r.d.accumulate[0] = a.accumulate;
  r.d.C[1] = b.C; r.d.ldc[1] = b.ldc; r.d.No[1] = b.No; r.d.accumulate[1] = b.accumulate;
  r.ok = true;
  return r;
}

// the launch of an accepted pair (r.ok): the images the scratch has to hold, then the one kernel; one timing entry
int gemm_nn_dual(const NnProduct& p1, const NnProduct& p2, const NnDualRoute& r, hipStream_t stream) {
  TimedScope timed(0, stream);
  const NnProduct* ps[2] = {&p1, &p2};
  for (int i = 0; i < 2; ++i)
    if (r.pack[i])
      if (int rc = launch_pack_b(2, *ps[i]->a, ps[i]->B1n, ps[i]->ldn1, nullptr, 0, static_cast<unsigned char*>(p1.ws) + r.ws_off[i], stream)) return rc;
  if (int rc = launch_nn2_dual(r.d, stream)) return rc;
  g_nn_dual_launches.fetch_add(1, std::memory_order_relaxed);
  return QAGNN_OK;
}

// ---- TN (weight gradients): split-K over row chunks, partials summed in order ------------------------------------------------------
// Rows per chunk.  Every chunk costs one Ka x No partial (written, then re-read by the chunk sum), so a launch whose chunk already
// spans several blocks takes longer chunks: just enough blocks for `per_cu` per CU; a multiple of the kernel's k-tile, never below `lo`.
static int tn_chunk_rows(int R, int blocks_per_chunk, int per_cu, int ktile, int lo) {
  const int target = num_cus() * per_cu / blocks_per_chunk;
  const int rows = cdiv(cdiv(R, target > 0 ? target : 1), ktile) * ktile, lo_k = cdiv(lo, ktile) * ktile;
  return rows > lo_k ? rows : lo_k;
}
// The shortest chunk: 256 rows (>= 1 block per CU for the 208 x 208 gradients at N = 64 000); for reductions over <= 4096 rows (class
// tables; 10 subgraphs = 2 000 node rows) the k-loop of a chunk is serial and the chip idle: 64 rows, and ONE 32-row k-tile in the split
// kernels (2 000 x 208 x 208: 126 blocks instead of 64, half the serial work each: profiles/r3_run18_small_batch_ab.txt).
static int tn_min_chunk(int R, bool split) { return R > 4096 ? 256 : split ? 32 : 64; }
// the scratch every route fits in (tn_route's chunks are never shorter than the shortest split chunk; up to 4 groups of column sums)
static int64_t tn_ws_bound(int R, int Ka, int No) { return (int64_t)cdiv(R, tn_min_chunk(R, true)) * ((int64_t)Ka * No + 4 * (int64_t)No); }
// chunks of that many 32-row k-tiles and more run k_gemm_tn_ws (one 8-wave block per CU leaves a block's first loads and its
// partial-sum stores uncovered, which only a long chunk amortises).  Measured with 8 - 24 k-tiles per block (tools/tn_ablate.hip,
// profiles/r4_run17_tn_ws.txt): 208 x 624 115 -> 126 us, 208 x 208 43 -> 57, 112 x 624 72 -> 74; at 36 per block 201 -> 171 us; at the
// 2-tile chunks of a 10-subgraph batch 29 us against the 4-wave kernel's ~14 (profiles/r5_run5_tn_ws_min_tiles_ab_b10.txt)
constexpr int TN_WS_MIN_TILES = 28;

// waves per block = 16-row output tiles per block: the count in [4, 16] that wastes the fewest rows of Ka (ties -> more waves)
static int pick_tn_waves(int Ka) {
  int best = 4, best_waste = INT32_MAX;
  for (int nw = 16; nw >= 4; --nw) {
    const int bm = nw * 16, waste = cdiv(Ka, bm) * bm - Ka;
    if (waste < best_waste) { best_waste = waste; best = nw; }
  }
  return best;
}
// What the bf16-split kernels take.  QAGNN_GEMM_SPLIT=0 pins the fp32-MFMA kernels of gemm.hip: the one numerically distinct fallback
// (the module mirror reads the same variable for the NN products: qagnn_amd/_lib.py)
static bool tn_split_ok(const TnProduct& p, int Ka, int lda) {
  static const int mode = getenv("QAGNN_GEMM_SPLIT") ? atoi(getenv("QAGNN_GEMM_SPLIT")) : 1;
  const bool gather = p.a_rowidx != nullptr;
  const int64_t big = (int64_t)p.R * ((lda > p.ldb && !gather) ? lda : p.ldb) * 4;  // (a gathered A goes through flat loads)
  if (gather && (Ka <= 112 || p.a_scale)) return false;
  return mode != 0 && Ka >= 64 && p.No >= 104 && p.R >= 1024 && big < (int64_t)0x7FFFFFFF;  // 32-bit buffer offsets
}

// the switch of qagnn_tn_live_tiles
static std::atomic<int> g_tn_live{1};
bool tn_live_enabled() { return g_tn_live.load(std::memory_order_relaxed) != 0; }
// a graph whose node rows are the product's rows, and K | M | Q in the kernel's three 208-column blocks
static bool tn_live_ok(const TnProduct& p) {
  return p.g && tn_live_enabled() && p.two && p.No == 3 * TN_LIVE_BC && p.g->N == p.R && p.g->err && !p.a_scale;
}

TnRoute tn_route(const TnProduct& p) {
  TnRoute r = {};
  r.np = 3;
  r.affine = p.a_scale != nullptr;
  r.gather = p.a_rowidx != nullptr;
  r.colsum = p.bsum != nullptr;
  r.sum_by4 = p.ldc % 4 == 0 && aligned16(p.C);
  // the two-operand product is ONE launch and ONE chunk sum where the split kernels take both halves, else two products
  const bool split = !r.colsum && tn_split_ok(p, p.Ka1, p.lda1) && (!p.two || (r.sum_by4 && tn_split_ok(p, p.Ka2, p.lda2)));
  const int lo = tn_min_chunk(p.R, split);
  int row_blocks;
  if (split) {
    // the scaled fp16 forms (three MFMAs, or one) where every operand's maximum is known
    if (r.sum_by4 && !r.gather && p.amax[0] && p.amax[2] && (!p.two || p.amax[1])) r.np = p.np;
    r.kt = (p.two || p.Ka1 <= 112) ? 7 : 13;  // (KT, NT) = (7, 13): the wide B tile, else (13, 7); two operands: 112-row tiles over A1's
    r.nt = 20 - r.kt;                         // columns, then over A2's
    row_blocks = cdiv(p.Ka1, r.kt * 16) + (p.two ? cdiv(p.Ka2, r.kt * 16) : 0);
    const int bpc = cdiv(p.No, r.nt * 16) * row_blocks;
    r.chunk_rows = tn_chunk_rows(p.R, bpc, 2, 32, lo);
    r.family = TnFamily::SPLIT;
    // Long two-operand products run k_gemm_tn_ws, ONE 8-wave block per CU: chunks sized for one block per CU (28 chunks of 72 k-tiles at
    // 64 000 rows instead of 56 of 36) halve the partial sums that are written and summed again
    if (p.two) {
      const int rows1 = tn_chunk_rows(p.R, bpc, 1, 32, lo);
      if (rows1 >= 2 * TN_WS_MIN_TILES * 32) r.chunk_rows = rows1;
      if (r.chunk_rows >= TN_WS_MIN_TILES * 32) r.family = TnFamily::WS;
      // ... and with the graph of a K | M | Q gradient at hand, balanced by its live k-tiles (common.h: tn_work).  nchunks >= 3 chunk
      // slots per column block; a slot's tiles fit the kernel's LDS list: lists hold <= 4.5 T / S tiles, ranges <= T / (S / 3 - 2)
      if (r.family == TnFamily::WS && tn_live_ok(p)) {
        const int T = cdiv(p.R, 32), nch = cdiv(p.R, r.chunk_rows);
        r.live = nch >= 3 && 5 * (T / (3 * nch) + 1) <= TN_LIST_CAP && cdiv(T, nch - 2) <= TN_LIST_CAP;
      }
    }
  } else if (p.two) {
    r.family = TnFamily::PAIR;
    return r;
  } else {  // the strip kernel is compiled for NT = 13 and 7 / 13 / 16 waves; k_gemm_tn serves every other width
    r.nt = pick_nt(p.No);
    r.waves = pick_tn_waves(p.Ka1);
    r.family = r.nt == 13 && (r.waves == 7 || r.waves == 13 || r.waves == 16) ? TnFamily::STRIP : TnFamily::RUNTIME;
    row_blocks = cdiv(p.Ka1, r.waves * 16);
    r.chunk_rows = tn_chunk_rows(p.R, cdiv(p.No, r.nt * 16) * row_blocks, r.waves <= 8 ? 2 : 1, 16, lo);
  }
  r.nchunks = cdiv(p.R, r.chunk_rows);
  r.grid = dim3(cdiv(p.No, r.nt * 16), row_blocks, r.nchunks);
  r.ws_elems = (int64_t)r.nchunks * ((int64_t)(p.Ka1 + p.Ka2) * p.No + (r.colsum ? (int64_t)p.groups * p.No : 0));
  return r;
}

static int tn_validate(const TnProduct& p) {
  QAGNN_REQUIRE(p.A1 && p.B && p.C && p.ws && (!p.two || p.A2), QAGNN_EINVAL, "gemm_tn: null pointer");
  QAGNN_REQUIRE(p.R > 0 && p.Ka1 > 0 && p.No > 0 && p.Ka1 % 4 == 0 && p.No % 4 == 0 && (!p.two || (p.Ka2 > 0 && p.Ka2 % 4 == 0)), QAGNN_EINVAL,
                "gemm_tn: bad sizes R=%d Ka1=%d Ka2=%d No=%d (Ka, No multiples of 4)", p.R, p.Ka1, p.Ka2, p.No);
  QAGNN_REQUIRE(p.lda1 % 4 == 0 && p.ldb % 4 == 0 && aligned16(p.A1) && aligned16(p.B) && (!p.two || (p.lda2 % 4 == 0 && aligned16(p.A2))),
                QAGNN_EINVAL, "gemm_tn: operands must be 16-byte aligned with pitches multiple of 4");
  QAGNN_REQUIRE(!p.a_scale || (!p.two && p.a_shift && aligned16(p.a_scale) && aligned16(p.a_shift)), QAGNN_EINVAL,
                "gemm_tn: a_scale/a_shift must both be given and 16-byte aligned (one-operand products only)");
  QAGNN_REQUIRE(p.lda1 >= p.Ka1 && (!p.two || p.lda2 >= p.Ka2) && p.ldb >= p.No && p.ldc >= p.No, QAGNN_EINVAL,
                "gemm_tn: a pitch below its width (lda1=%d Ka1=%d lda2=%d Ka2=%d ldb=%d ldc=%d No=%d)", p.lda1, p.Ka1, p.lda2, p.Ka2, p.ldb, p.ldc,
                p.No);
  QAGNN_REQUIRE(!p.bsum || (p.groups >= 1 && p.groups <= 4 && (p.groups == 1 || p.b_rowidx)), QAGNN_EINVAL, "gemm_tn: colsum groups=%d (1..4)",
                p.groups);
  return QAGNN_OK;
}

static int tn_run(const TnProduct& p, hipStream_t stream) {
  if (int rc = tn_validate(p)) return rc;
  const TnRoute r = tn_route(p);
  if (r.family == TnFamily::PAIR) {  // in the six-MFMA form, whatever maxima are known
    TnProduct q = p;
    q.two = false; q.A2 = nullptr; q.lda2 = q.Ka2 = 0;
    q.amax[0] = q.amax[1] = q.amax[2] = nullptr;
    if (int rc = tn_run(q, stream)) return rc;
    q.A1 = p.A2; q.lda1 = p.lda2; q.Ka1 = p.Ka2; q.C = p.C + (int64_t)p.Ka1 * p.ldc;
    return tn_run(q, stream);
  }
  const int Ka = p.Ka1 + p.Ka2;
  QAGNN_REQUIRE(r.ws_elems <= tn_ws_bound(p.R, Ka, p.No), QAGNN_EINVAL, "gemm_tn: the route outgrows qagnn_gemm_tn_workspace_elems()");
  float* Pcs = r.colsum ? p.ws + (int64_t)r.nchunks * Ka * p.No : nullptr;
  const int rc = r.family == TnFamily::WS      ? launch_tn_ws(r, p, stream)
                 : r.family == TnFamily::SPLIT ? launch_tn_split(r, p, stream)
                 : r.family == TnFamily::STRIP ? launch_tn_strip(r, p, Pcs, stream)
                                               : launch_tn(r, p, Pcs, stream);
  if (rc != QAGNN_OK) return rc;
  if (r.live) {
    const LiveTiles lt = live_tiles_of(p.g);
    return launch_sum_chunks_live(p.ws, p.C, p.ldc, Ka, TnLive{lt.list, lt.n_live, lt.n_tiles, 3 * r.nchunks, r.chunk_rows / 32}, p.accumulate, stream);
  }
  if (int rc2 = launch_sum_chunks(p.ws, p.C, p.ldc, Ka, p.No, r.nchunks, p.accumulate, r.sum_by4, stream)) return rc2;
  return r.colsum ? launch_sum_chunks(Pcs, p.bsum, p.No, p.groups, p.No, r.nchunks, 0, false, stream) : QAGNN_OK;
}

int gemm_tn(const TnProduct& p, hipStream_t stream) {
  TimedScope timed(1, stream);
  return tn_run(p, stream);
}

}  // namespace qagnn

using namespace qagnn;

// ---- the C ABI: each entry point fills a product description ------------------------------------------------------------------------
extern "C" int64_t qagnn_packed_min_rows(int64_t rows) { return rows < 0 ? g_pack_min_m.load() : g_pack_min_m.exchange(rows > 1 ? rows : 1); }

extern "C" int64_t qagnn_gemm_nn_pack_bytes(int32_t No, int32_t K1, int32_t K2) { return nn2_pack_bytes(No, K1, K2, 3) + 256; }  // (>= the two-piece image + its scale words)

extern "C" int64_t qagnn_gemm_nn_ws_bytes(const qagnn_gemm_nn_args* a, const float* B1n, int32_t ldn1, const float* B2n, int32_t ldn2) {
  alignas(16) static char any_ws;  // what the route packs when the scratch is there and large enough
  return a && B1n ? nn_route(NnProduct{a, true, B1n, ldn1, B2n, ldn2, &any_ws, INT64_MAX}).ws_bytes : 0;
}

extern "C" int qagnn_gemm_nn_f32(const qagnn_gemm_nn_args* a, qagnn_stream_t stream) {
  return gemm_nn(NnProduct{a, false, nullptr, 0, nullptr, 0, nullptr, 0}, (hipStream_t)stream);
}

extern "C" int qagnn_gemm_nn_split_f32(const qagnn_gemm_nn_args* a, const float* B1n, int32_t ldn1, const float* B2n, int32_t ldn2,
                                       qagnn_stream_t stream) {
  return gemm_nn(NnProduct{a, true, B1n, ldn1, B2n, ldn2, nullptr, 0}, (hipStream_t)stream);
}

extern "C" int qagnn_gemm_nn_split_ws_f32(const qagnn_gemm_nn_args* a, const float* B1n, int32_t ldn1, const float* B2n, int32_t ldn2,
                                          void* ws, int64_t ws_bytes, qagnn_stream_t stream) {
  return gemm_nn(NnProduct{a, true, B1n, ldn1, B2n, ldn2, ws, ws_bytes}, (hipStream_t)stream);
}

extern "C" int qagnn_dual_version(void) { return 1; }

extern "C" int qagnn_gemm_nn_dual_f32(const qagnn_gemm_nn_args* p1, const float* B1n, int32_t ldn1, const qagnn_gemm_nn_args* p2, const float* B2n,
                                      int32_t ldn2, void* pack_ws, int64_t pack_bytes, qagnn_stream_t stream) {
  const NnProduct q1{p1, true, B1n, ldn1, nullptr, 0, pack_ws, pack_bytes}, q2{p2, true, B2n, ldn2, nullptr, 0, nullptr, 0};
  QAGNN_REQUIRE(p1 && p2, QAGNN_EINVAL, "gemm_nn_dual: null pointer");
  QAGNN_REQUIRE(p1->K2 == 0 && p2->K2 == 0, QAGNN_EUNSUPPORTED, "gemm_nn_dual: one K segment per product (K2 = %d / %d)", p1->K2, p2->K2);
  if (int rc = nn_validate(q1)) return rc;
  if (int rc = nn_validate(q2)) return rc;
  const NnDualRoute r = nn_dual_route(q1, q2);
  QAGNN_REQUIRE(r.ok, QAGNN_EUNSUPPORTED, "gemm_nn_dual: not a pair the two-output launch takes (include/qagnn_hip_dual.h)");
  return gemm_nn_dual(q1, q2, r, (hipStream_t)stream);
}

extern "C" int qagnn_gemm_nn_dual_query(const qagnn_gemm_nn_args* p1, const float* B1n, int32_t ldn1, const qagnn_gemm_nn_args* p2, const float* B2n,
                                        int32_t ldn2, const void* pack_ws, int64_t pack_bytes) {
  alignas(16) static char any_ws;  // (pack_ws == NULL, pack_bytes < 0: as if both images were registered -- any scratch, of any size)
  const bool assume = !pack_ws && pack_bytes < 0;
  const NnProduct q1{p1, true, B1n, ldn1, nullptr, 0, assume ? &any_ws : const_cast<void*>(pack_ws), assume ? INT64_MAX : pack_bytes};
  const NnProduct q2{p2, true, B2n, ldn2, nullptr, 0, nullptr, 0};
  if (nn_validate(q1) != QAGNN_OK || nn_validate(q2) != QAGNN_OK) return 0;
  return nn_dual_route(q1, q2).ok ? 1 : 0;
}

extern "C" int64_t qagnn_dual_launches(void) { return g_nn_dual_launches.load(); }

extern "C" int qagnn_dual_blocks_per_cu(void) { return nn2_dual_blocks_per_cu(); }

extern "C" int qagnn_nn_dual_enable(int32_t on) {
  const int was = nn_dual_mode();
  if (on >= 0) g_nn_dual.store(on > 2 ? 2 : on);
  return was;
}

extern "C" int64_t qagnn_gemm_tn_workspace_elems(int32_t R, int32_t Ka, int32_t No) { return tn_ws_bound(R, Ka, No); }

extern "C" int qagnn_gemm_tn_colsum_f32(const float* A, int32_t lda, const float* B, int32_t ldb, float* C, int32_t ldc, int32_t R,
                                        int32_t Ka, int32_t No, const float* a_scale, const float* a_shift, const int64_t* a_rowidx,
                                        int32_t accumulate, float* bsum, const int64_t* b_rowidx, int32_t groups, float* workspace,
                                        qagnn_stream_t stream) {
  TnProduct p = tn_product(A, lda, Ka, nullptr, 0, 0, B, ldb, C, ldc, R, No, a_scale, a_shift, workspace);
  p.a_rowidx = a_rowidx; p.accumulate = accumulate; p.bsum = bsum; p.b_rowidx = b_rowidx; p.groups = groups;
  return gemm_tn(p, (hipStream_t)stream);
}

extern "C" int qagnn_gemm_tn_f32(const float* A, int32_t lda, const float* B, int32_t ldb, float* C, int32_t ldc, int32_t R,
                                 int32_t Ka, int32_t No, const float* a_scale, const float* a_shift, const int64_t* a_rowidx,
                                 int32_t accumulate, float* workspace, qagnn_stream_t stream) {
  TnProduct p = tn_product(A, lda, Ka, nullptr, 0, 0, B, ldb, C, ldc, R, No, a_scale, a_shift, workspace);
  p.a_rowidx = a_rowidx; p.accumulate = accumulate;
  return gemm_tn(p, (hipStream_t)stream);
}

// C [Ka1 + Ka2, No] = [A1 | A2]^T B: the two weight gradients that share their B operand (X^T dK|dM|dQ and S^T dK|dM|dQ of a hop)
extern "C" int qagnn_gemm_tn2_f32(const float* A1, int32_t lda1, int32_t Ka1, const float* A2, int32_t lda2, int32_t Ka2, const float* B,
                                  int32_t ldb, float* C, int32_t ldc, int32_t R, int32_t No, float* workspace, qagnn_stream_t stream) {
  TnProduct p = tn_product(A1, lda1, Ka1, A2, lda2, Ka2, B, ldb, C, ldc, R, No, nullptr, nullptr, workspace);
  p.two = true;
  return gemm_tn(p, (hipStream_t)stream);
}

// The same products in the scaled fp16 forms (gemm_nn2.hip's header): _h2 three MFMAs per product, _h1 ONE (reduced precision: operands
// rounded to fp16 under the same scales; on request only -- qagnn_hop_args.gemm_split == 3).  A2 == nullptr / Ka2 == 0: one operand.
// Shapes the split kernels do not take, or a missing maximum, fall back to the six-MFMA route.
extern "C" int qagnn_gemm_tn_h2_f32(const float* A1, int32_t lda1, int32_t Ka1, const float* A2, int32_t lda2, int32_t Ka2, const float* B,
                                    int32_t ldb, float* C, int32_t ldc, int32_t R, int32_t No, const float* a_scale, const float* a_shift,
                                    const uint32_t* amax_a1, const uint32_t* amax_a2, const uint32_t* amax_b, float* workspace,
                                    qagnn_stream_t stream) {
  return gemm_tn(tn_product(A1, lda1, Ka1, A2, lda2, Ka2, B, ldb, C, ldc, R, No, a_scale, a_shift, workspace, amax_a1, amax_a2, amax_b, 2),
                 (hipStream_t)stream);
}

extern "C" int qagnn_gemm_tn_graph_f32(const float* A1, int32_t lda1, int32_t Ka1, const float* A2, int32_t lda2, int32_t Ka2, const float* B,
                                       int32_t ldb, float* C, int32_t ldc, int32_t R, int32_t No, const uint32_t* amax_a1, const uint32_t* amax_a2,
                                       const uint32_t* amax_b, int32_t pieces, const qagnn_graph* g, float* workspace, qagnn_stream_t stream) {
  QAGNN_REQUIRE(pieces >= 1 && pieces <= 3, QAGNN_EINVAL, "gemm_tn_graph: pieces=%d (1..3)", pieces);
  const bool h = pieces < 3;
  TnProduct p = tn_product(A1, lda1, Ka1, A2, lda2, Ka2, B, ldb, C, ldc, R, No, nullptr, nullptr, workspace, h ? amax_a1 : nullptr,
                           h ? amax_a2 : nullptr, h ? amax_b : nullptr, h ? pieces : 3);
  p.g = g;
  return gemm_tn(p, (hipStream_t)stream);
}

extern "C" int qagnn_gemm_tn_route_query(int32_t R, int32_t Ka1, int32_t Ka2, int32_t No, int32_t* h_out) {
  QAGNN_REQUIRE(h_out && R > 0 && Ka1 > 0 && Ka2 >= 0 && No > 0, QAGNN_EINVAL, "gemm_tn_route_query: bad arguments");
  alignas(16) static float any[4];  // (the route looks at the presence and the alignment of pointers only)
  qagnn_graph any_g = {};
  TnProduct p = tn_product(any, Ka1, Ka1, Ka2 > 0 ? any : nullptr, Ka2, Ka2, any, No, any, No, R, No, nullptr, nullptr, any);
  any_g.N = R;
  any_g.err = reinterpret_cast<int32_t*>(any);
  p.g = &any_g;
  const TnRoute r = tn_route(p);
  h_out[0] = (int)r.family; h_out[1] = r.chunk_rows; h_out[2] = r.nchunks; h_out[3] = r.live ? 1 : 0;
  return QAGNN_OK;
}

extern "C" int qagnn_tn_live_tiles(int32_t on) { return on < 0 ? g_tn_live.load() : g_tn_live.exchange(on ? 1 : 0); }

extern "C" int qagnn_gemm_tn_h1_f32(const float* A1, int32_t lda1, int32_t Ka1, const float* A2, int32_t lda2, int32_t Ka2, const float* B,
                                    int32_t ldb, float* C, int32_t ldc, int32_t R, int32_t No, const float* a_scale, const float* a_shift,
                                    const uint32_t* amax_a1, const uint32_t* amax_a2, const uint32_t* amax_b, float* workspace,
                                    qagnn_stream_t stream) {
  return gemm_tn(tn_product(A1, lda1, Ka1, A2, lda2, Ka2, B, ldb, C, ldc, R, No, a_scale, a_shift, workspace, amax_a1, amax_a2, amax_b, 1),
                 (hipStream_t)stream);
}
