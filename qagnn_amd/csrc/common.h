// Shared helpers for the gfx950 kernels of libqagnn_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "../../include/qagnn_hip.h"
#include "../../include/qagnn_hip_tn.h"
#include "../../include/qagnn_hip_infer.h"

namespace qagnn {

void set_error(const char* fmt, ...);

// ---- the dense products (gemm_dispatch.hip) -------------------------------------------------------------------
// A product's ROUTE -- kernel family, tile shape, arithmetic form, where B comes from, chunking, grid, scratch -- is decided once, by
// nn_route() / tn_route(), and travels as a value: the launchers below (one per kernel template, next to their kernels), the scratch
// queries of the C ABI and hop.hip all read it.
struct NnProduct {  // C = [A1|A2] [B1;B2] + epilogue: the ABI's argument block + B as [No][K] (the bf16 / fp16 kernels) + pack scratch
  const qagnn_gemm_nn_args* a;
  bool split;  // false: the fp32-MFMA kernel on a->B1 / a->B2 (qagnn_gemm_nn_f32)
  const float* B1n; int ldn1; const float* B2n; int ldn2;
  void* ws; int64_t ws_bytes;
};
enum class NnFamily { FP32, SPLIT, NN2 };         // k_gemm_nn (gemm.hip), k_gemm_nn_split (gemm_split.hip), k_gemm_nn2 (gemm_nn2.hip)
enum class NnB { IN_KERNEL, PACK, IMAGE };        // B split inside the kernel / packed into the scratch per call / a registered image
struct NnRoute {
  NnFamily family;
  int nt, np, wv;             // column tiles per block; pieces per operand (3 = exact 3 x bf16 split, 2 = scaled fp16 pair, 1 = fp16); waves
  bool affine, flat, stats;   // scale / shift prologue; 64-bit flat operand addressing (SPLIT); column statistics in the epilogue
  NnB b; const void* image;   // NN2
  int64_t ws_bytes;           // scratch the route writes (PACK), else 0
  int ntiles, grid;
};
inline int num_cus() {  // of the current device at first use; 256 (an MI355X) where there is none
  static int n = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
    return v;
  }();
  return n;
}
static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
// persistent launch shape: tiles of rows_per_tile x nt * 16 outputs walked by at most per_cu blocks per CU (a multiple of 8: the
// block -> XCD mapping survives the tile walk)
inline void nn_grid(NnRoute& r, int M, int No, int rows_per_tile, int per_cu) {
  r.ntiles = cdiv(No, r.nt * 16) * cdiv(M, rows_per_tile);
  const int cap = (num_cus() * per_cu) & ~7;
  r.grid = r.ntiles < cap ? r.ntiles : cap;
}
NnRoute nn_route(const NnProduct& p);
bool nn_rows_packed(int64_t M);  // rows from which products take packed B images and the scaled forms (qagnn_packed_min_rows)
int nn_validate(const NnProduct& p);  // the argument checks of every NN entry point (gemm_nn runs them itself)
int gemm_nn(const NnProduct& p, hipStream_t stream);
int launch_nn(const NnRoute& r, const qagnn_gemm_nn_args& a, hipStream_t stream);
int launch_nn_split(const NnRoute& r, const qagnn_gemm_nn_args& a, const float* B1n, int ldn1, const float* B2n, int ldn2, hipStream_t stream);
// (b != IN_KERNEL: B1n = the image, ldn1 = its column tiles per k-tile)
int launch_nn2(const NnRoute& r, const qagnn_gemm_nn_args& a, const float* B1n, int ldn1, const float* B2n, int ldn2, hipStream_t stream);
int launch_pack_b(int np, const qagnn_gemm_nn_args& a, const float* B1n, int ldn1, const float* B2n, int ldn2, void* ws, hipStream_t stream);
// Two NN products over ONE A operand as one launch (include/qagnn_hip_dual.h; k_gemm_nn2_dual in gemm_nn2.hip): C[0] = A B[0] over 13 column
// tiles, C[1] = A B[1] over 7, both B as two-piece images.  Filled by nn_dual_route (gemm_dispatch.hip), which is where the shapes are checked.
struct NnDual {
  const float* A; int lda, K, M;
  const uint32_t* a_amax;
  const void* image[2];
  float* C[2]; int ldc[2], No[2], accumulate[2];
};
int launch_nn2_dual(const NnDual& d, hipStream_t stream);
int nn2_dual_blocks_per_cu();  // what the runtime reports for k_gemm_nn2_dual (80 KB of LDS per block: two fill a CU)
// the route of such a pair: ok = the one launch takes it; pack[i]: image i is packed into the scratch at ws_off[i] first (else it is registered)
struct NnDualRoute { bool ok; NnDual d; bool pack[2]; int64_t ws_off[2]; };
NnDualRoute nn_dual_route(const NnProduct& p1, const NnProduct& p2);  // (both validated; the scratch: p1.ws / p1.ws_bytes)
int gemm_nn_dual(const NnProduct& p1, const NnProduct& p2, const NnDualRoute& r, hipStream_t stream);
bool nn_dual_enabled();  // QAGNN_NN_DUAL / qagnn_nn_dual_enable: hop.hip sends a hop's dX and dS through the one launch
namespace nn2 { int walk_tiles(int K1, int K2); }  // k-tiles of 32 that k_gemm_nn2 walks over the two segments
int64_t nn2_pack_bytes(int No, int K1, int K2, int np);
const void* nn2_prepack_lookup(const float* B1n, int ldn1, int K1, const float* B2n, int ldn2, int K2, int No, int np);

struct TnProduct {  // C [Ka1 (+ Ka2), No] (+)= [A1 | A2]^T B over R rows, through split-K partials in ws
  const float* A1; int lda1, Ka1;
  const float* A2; int lda2, Ka2; bool two;        // two: the two-operand product (A2's rows of C follow A1's)
  const float* B; int ldb;
  float* C; int ldc, R, No;
  const float* a_scale; const float* a_shift; const int64_t* a_rowidx; int accumulate;
  float* bsum; const int64_t* b_rowidx; int groups;  // column sums of B per group, by-product of the same pass
  const uint32_t* amax[3]; int np;                   // {max|A1|, max|A2|, max|B|} device words + the scaled form they ask for (2 or 1)
  float* ws;
  const qagnn_graph* g;                              // the graph whose rows are the R rows of a K|M|Q gradient B (live k-tiles), or nullptr
};
// (one operand: A2 == nullptr or Ka2 <= 0)
inline TnProduct tn_product(const float* A1, int lda1, int Ka1, const float* A2, int lda2, int Ka2, const float* B, int ldb, float* C, int ldc, int R,
                            int No, const float* a_scale, const float* a_shift, float* ws, const uint32_t* amax_a1 = nullptr,
                            const uint32_t* amax_a2 = nullptr, const uint32_t* amax_b = nullptr, int np = 3) {
  TnProduct p = {};
  p.A1 = A1; p.lda1 = lda1; p.Ka1 = Ka1;
  if (A2 && Ka2 > 0) { p.A2 = A2; p.lda2 = lda2; p.Ka2 = Ka2; p.two = true; }
  p.B = B; p.ldb = ldb; p.C = C; p.ldc = ldc; p.R = R; p.No = No; p.a_scale = a_scale; p.a_shift = a_shift; p.ws = ws;
  p.amax[0] = amax_a1; p.amax[1] = amax_a2; p.amax[2] = amax_b; p.np = np;
  return p;
}
enum class TnFamily { RUNTIME, STRIP, SPLIT, WS, PAIR };  // k_gemm_tn, k_gemm_tn_strip (gemm.hip); k_gemm_tn_split, k_gemm_tn_ws (gemm_split.hip);
                                                          // PAIR: a two-operand product as two single ones
struct TnRoute {
  TnFamily family;
  int kt, nt, waves, np;      // 16-row / 16-column output tiles per block (kt: SPLIT / WS; waves: RUNTIME / STRIP); pieces
  bool affine, gather, colsum;
  int chunk_rows, nchunks;
  bool sum_by4;               // the chunk sum in float4 steps
  bool live;                  // WS: the blocks take their k-tiles from the graph's live-tile list (tn_work below)
  dim3 grid;
  int64_t ws_elems;           // floats of ws the route writes
};
TnRoute tn_route(const TnProduct& p);
int gemm_tn(const TnProduct& p, hipStream_t stream);
int launch_tn(const TnRoute& r, const TnProduct& p, float* Pcs, hipStream_t stream);        // Pcs: the column-sum partials (colsum)
int launch_tn_strip(const TnRoute& r, const TnProduct& p, float* Pcs, hipStream_t stream);
int launch_tn_split(const TnRoute& r, const TnProduct& p, hipStream_t stream);
int launch_tn_ws(const TnRoute& r, const TnProduct& p, hipStream_t stream);
// C (+)= the chunks' partials P [nchunks][rows][No], summed in order (by4: float4 steps -- ldc, No multiples of 4, C 16-byte aligned)
int launch_sum_chunks(const float* P, float* C, int ldc, int rows, int No, int nchunks, int accumulate, bool by4, hipStream_t stream);

// ---- the two-operand weight gradient balanced by LIVE k-tiles (k_gemm_tn_ws<.., LIVE>) ---------------------------------------------
// B = dK | dM | dQ of a hop: a node row whose only edge is its self loop has dK = dQ = 0 exactly, so a 32-row k-tile of such rows
// ("dead") adds nothing to the K and Q column blocks.  The launch keeps its grid -- 3 column blocks x row blocks x nchunks, S = 3 nchunks
// chunk slots per row block -- and divides the slots by work: cK slots each for K and Q, which walk lists of live tiles, cM = S - 2 cK for
// M, which walk ranges of all tiles, so that every block walks about T (1 + 2 L / T) / S tiles.  Everything below is integer arithmetic on
// (S, T, L): a pure function of the graph, the same in every block, in the chunk sum and on the host.
constexpr int TN_LIST_CAP = 1024;  // k-tiles of one slot (staged in LDS); tn_route keeps longer products off the route
constexpr int TN_LIVE_BC = 208;    // the column block: K, M and Q are 208 columns each (DP = 208)
struct TnLive { const int* list; const int* n_live; int T, S, chunk_tiles; };
struct TnWork { int cK, cM, lenM, qK, rK; };  // qK < 0: no dead tile -- every column block walks today's chunks
struct TnSlot { int cb, list, beg, cnt, pslot; };  // column block; list (1) or range (0) of cnt tiles from beg; partial tile in the workspace
__host__ __device__ inline TnWork tn_work(int S, int T, int L, int chunk_tiles) {
  TnWork w;
  L = L < 0 ? 0 : (L > T ? T : L);
  if (L >= T) {  // the partition of the launch without a table: S / 3 chunks of chunk_tiles for every column block
    w.cK = S / 3; w.cM = S - 2 * w.cK; w.lenM = chunk_tiles; w.qK = -1; w.rK = 0;
    return w;
  }
  const long long den = (long long)T + 2ll * L;
  int c = (int)((2ll * S * L + den) / (2 * den));  // round(S L / (T + 2 L))
  const int hi = (S - 1) / 2;
  c = c < 1 ? 1 : (c > hi ? hi : c);
  w.cK = c; w.cM = S - 2 * c; w.lenM = (T + w.cM - 1) / w.cM; w.qK = L / c; w.rK = L % c;
  return w;
}
// Unit u in [0, S) of a row block, in block order: group j = K slot j, Q slot j, then the M slots [j cM / cK, (j + 1) cM / cK) -- the K and
// Q blocks of one slot index are neighbours (they walk the same list), and the M ranges advance through the rows with the lists.
__host__ __device__ inline TnSlot tn_slot(const TnWork& w, int S, int T, int u) {
  auto start = [&](int j) { return 2 * j + (int)((long long)j * w.cM / w.cK); };
  int j = (int)((long long)u * w.cK / S);
  while (j > 0 && start(j) > u) --j;
  while (j + 1 < w.cK && start(j + 1) <= u) ++j;
  const int off = u - start(j);
  TnSlot s;
  auto range = [&](int i) { s.list = 0; s.beg = i * w.lenM < T ? i * w.lenM : T; s.cnt = T - s.beg < w.lenM ? T - s.beg : w.lenM; };
  if (off < 2) {
    s.cb = off == 0 ? 0 : 2;
    s.pslot = off == 0 ? j : w.cK + j;
    if (w.qK < 0) range(j);
    else { s.list = 1; s.beg = j * w.qK + (j < w.rK ? j : w.rK); s.cnt = w.qK + (j < w.rK ? 1 : 0); }
  } else {
    const int m = (int)((long long)j * w.cM / w.cK) + off - 2;
    s.cb = 1;
    s.pslot = 2 * w.cK + m;
    range(m);
  }
  return s;
}
// the chunk sum of that launch: P holds S tiles [rows][208], the K slots first, then Q's, then M's; summed in slot order
int launch_sum_chunks_live(const float* P, float* C, int ldc, int rows, const TnLive& lv, int accumulate, hipStream_t stream);
bool tn_live_enabled();
// where graph preparation leaves a graph's live tiles: behind the 16 words of g->err (include/qagnn_hip_tn.h)
struct LiveTiles { int n_tiles; int32_t *n_live, *live, *list; };
inline LiveTiles live_tiles_of(const qagnn_graph* g) {
  const int T = (int)(((int64_t)g->N + 31) / 32), T4 = (T + 3) & ~3;
  int32_t* const p = g->err + 16;
  return LiveTiles{T, p, p + 4, p + 4 + T4};
}
// ... and behind the live k-tiles the LIVE CLASSES of the batch: n_live [4] | list [roundup4(C)] -- the classes with at least one edge,
// ascending (graph_prep.hip: k_live_classes).  The class reduction of the edge backward gives blocks to these only.
struct LiveClasses { int32_t *n_live, *list; };
inline LiveClasses live_classes_of(const qagnn_graph* g) {
  const LiveTiles lt = live_tiles_of(g);
  int32_t* const p = lt.list + ((lt.n_tiles + 3) & ~3);
  return LiveClasses{p, p + 4};
}

// producers that can leave max |output| behind for the three-MFMA GEMM form (elementwise.hip; amax = nullptr: plain launch)
int launch_gelu_dropout(const float* X, const float* dY, float* out, int64_t n, float p, uint64_t seed, uint32_t* amax, float* amax_part,
                        hipStream_t stream);
int64_t gelu_amax_scratch_elems(int64_t n);
int launch_bn_relu_bwd_colsum(const float* dR, const float* Hh, float* dH, int ld, int R, int Cc, const float* mean, const float* invstd,
                              const float* scale, const float* shift, const float* gamma, const float* sum_dy, const float* sum_dy_hhat,
                              float inv_rows, const float* roww, float* colsum, float* workspace, uint32_t* amax, bool finalize, hipStream_t stream);
// reductions whose result nothing inside a stack of hops reads, finished for all its layers in one launch each (hop.hip: stack_bwd_impl)
constexpr int DEFER_LAYERS_MAX = 16;
struct LayerOut { float* p[DEFER_LAYERS_MAX]; };  // where each layer's result goes
int64_t bn_colsum_part_elems(int R, int Cc);  // floats of column partials launch_bn_relu_bwd_colsum leaves in its workspace
int launch_colreduce_final_layers(const float* part, int64_t layer_stride, int layers, const LayerOut& outs, int R, int Cc, hipStream_t stream);
int launch_bn_stats_finalize(const float* part, int n_tiles, int R, int Cc, const float* gamma, const float* beta, float eps, float* stats,
                             float* run_mean, float* run_var, int64_t* nbt, int d, float momentum, float unbias, int ones_col, uint32_t* amax_bound,
                             hipStream_t stream);

int launch_edge_attn_fwd(const qagnn_graph* g, const float* KMQ, int32_t ldk, const float* EkEm, int32_t lde, int32_t HP, float qscale,
                         float* score, float* a, float* alpha, float* aggr, int32_t lda, float* amax_part /* [N] or nullptr */, hipStream_t stream);
int launch_edge_attn_bwd(const qagnn_graph* g, const float* KMQ, int32_t ldk, const float* EkEm, int32_t lde, int32_t HP, float qscale,
                         const float* a, const float* alpha, const float* G, int32_t ldg, float* dKMQ, float* dEkEm, float* ga, float* rs,
                         float* cls_part, float* amax_part /* [3 N] or nullptr */, uint32_t* amax_slot, bool reduce_now, hipStream_t stream);
// the class reduction the call above ends with, for several layers at once (edge_attn.hip)
int launch_cls_reduce(const qagnn_graph* g, int32_t HP, float* cls_part, int64_t layer_stride, int layers, const LayerOut& out, int32_t lde,
                      hipStream_t stream);
int launch_amax_reduce(const float* part, int64_t n, uint32_t* slot, hipStream_t stream);  // max of n non-negative floats -> *slot (elementwise.hip)
// max relu(scale * H + shift) over R x Cc -> *slot, through per-block partials in `part` (infer.hip: qagnn_bn_relu_absmax_f32 after its checks)
int launch_bn_relu_absmax(const float* H, int ldh, int R, int Cc, const float* scale, const float* shift, uint32_t* slot, float* part, hipStream_t stream);

// launch timing (timing.hip): a scope at the top of an entry point brackets everything it launches on `s` while qagnn_timing_enable(1)
struct TimedScope {
  int kind;
  hipStream_t s;
  hipEvent_t e0, e1;
  bool counted;
  TimedScope(int kind, hipStream_t s);
  ~TimedScope();
  TimedScope(const TimedScope&) = delete;
  TimedScope& operator=(const TimedScope&) = delete;
};

#define QAGNN_REQUIRE(cond, code, ...) \
  do {                                 \
    if (!(cond)) {                     \
      qagnn::set_error(__VA_ARGS__);   \
      return (code);                   \
    }                                  \
  } while (0)

#define QAGNN_LAUNCH_CHECK(name)                                               \
  do {                                                                         \
    hipError_t e__ = hipGetLastError();                                        \
    if (e__ != hipSuccess) {                                                   \
      qagnn::set_error("%s launch failed: %s", name, hipGetErrorString(e__));  \
      return QAGNN_EHIP;                                                       \
    }                                                                          \
  } while (0)

// Register budget of k_gemm_nn (gemm.hip): QAGNN_NN_OCC co-resident blocks per CU, which is also what its persistent grid is sized for
#ifndef QAGNN_NN_OCC
#define QAGNN_NN_OCC 2  // 0 = leave it to the compiler (it takes ~300 registers for NT = 13: one block per CU)
#endif

// run-time value -> compile-time constant: f(std::integral_constant<int, V>{}) for the V of the list that equals v (the last V if none does)
template <int V0, int... Vs, class F>
inline int dispatch_int(int v, F&& f) {
  if constexpr (sizeof...(Vs) == 0) return f(std::integral_constant<int, V0>{});
  else return v == V0 ? f(std::integral_constant<int, V0>{}) : dispatch_int<Vs...>(v, f);
}
template <class F>
inline int dispatch_bool(bool v, F&& f) { return v ? f(std::true_type{}) : f(std::false_type{}); }

// a kernel that needs more than the default 64 KB of dynamic LDS has its limit raised, once per device
template <auto KERNEL>
inline int raise_lds_limit(int bytes, const char* name) {
  static bool raised[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  if (bytes <= 64 * 1024 || raised[dev & 63]) return QAGNN_OK;
  hipError_t e = hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e != hipSuccess) { set_error("%s: cannot raise the dynamic LDS limit: %s", name, hipGetErrorString(e)); return QAGNN_EHIP; }
  raised[dev & 63] = true;
  return QAGNN_OK;
}

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// MI355X: 8 XCDs, workgroup b is observed to run on XCD b % 8 (speed only, never correctness).
// Remap so that each XCD walks a contiguous range of logical work items: neighbouring node rows (one
// subgraph = n consecutive rows, all its edges stay inside) then share one L2.  Bijective for any grid size.
__device__ __forceinline__ int xcd_remap(int b, int nblocks) {
  const int q = nblocks >> 3, r = nblocks & 7;
  const int xcd = b & 7, slot = b >> 3;
  const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + slot;
}

// The balanced form for the node-side edge kernels (graph_prep.hip: k_xcd_partition): XCD k walks the 4-node blocks
// [base[k], base[k + 1]); the grid is 8 x edge_xcd_cap(N) blocks and a block past its XCD's run has nothing to do (-1).
__host__ __device__ __forceinline__ int edge_xcd_cap(int N) {
  const int per = (((N + 3) >> 2) + 7) >> 3;
  return (per * 5 + 3) >> 2;  // 1.25 x an equal share
}
__device__ __forceinline__ int xcd_remap_balanced(int b, const int* __restrict__ base) {
  const int xcd = b & 7, lb = base[xcd] + (b >> 3);
  return lb < base[xcd + 1] ? lb : -1;
}

// Dropout seeds under hipGraph replay.  Every dropout launch takes its seed BY VALUE, which a captured graph would replay verbatim:
// the same keep masks in every training step.  The kernels therefore mix one device-resident word -- the seed EPOCH, one per device,
// 0 unless a caller advances it -- into the seed; a captured step ends with qagnn_seed_epoch_advance(), so each replay draws new
// masks while forward and backward of one replay still agree.  With the epoch at 0 (eager use) the seeds are used as passed.
const unsigned long long* seed_epoch_ptr();  // device address of the current device's epoch word (elementwise.hip)
__device__ __forceinline__ uint64_t epoch_seed(uint64_t seed, const unsigned long long* __restrict__ epoch) {
  return epoch ? seed + (uint64_t)epoch[0] * 0xD1B54A32D192ED03ull : seed;  // (null: the epoch word could not be resolved -- epoch 0)
}

// counter-based uniform in [0,1): splitmix64 finaliser over (seed, element index); same value in fwd and bwd
__device__ __forceinline__ float uniform01(uint64_t seed, uint64_t idx) {
  uint64_t z = seed + (idx + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  return (float)(z >> 40) * (1.0f / 16777216.0f);
}


// Cross-lane reductions.  `__shfl_xor` compiles to ds_bpermute_b32 (an LDS-crossbar round trip, ~100 cycles, with an
// s_waitcnt lgkmcnt(0) behind every step); inside a 16-lane DPP row the same butterfly is four v_add_f32_dpp with
// row_ror:8/4/2/1 (a cyclic rotation inside the row), issued back to back.  After a rotation by r the partial sums are
// periodic with period r and the add is commutative, so all 16 lanes end up with the bit-identical total.
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
constexpr int DPP_ROW_ROR = 0x120;  // + n: rotate right by n lanes inside each row of 16

// sum over the 16 lanes of a DPP row (lanes 16g..16g+15); every lane ends up with the total.  All 64 lanes must be active.
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp_f32<DPP_ROW_ROR + 8>(v);
  v += dpp_f32<DPP_ROW_ROR + 4>(v);
  v += dpp_f32<DPP_ROW_ROR + 2>(v);
  v += dpp_f32<DPP_ROW_ROR + 1>(v);
  return v;
}
__device__ __forceinline__ float row16_max(float v) {
  v = fmaxf(v, dpp_f32<DPP_ROW_ROR + 8>(v));
  v = fmaxf(v, dpp_f32<DPP_ROW_ROR + 4>(v));
  v = fmaxf(v, dpp_f32<DPP_ROW_ROR + 2>(v));
  v = fmaxf(v, dpp_f32<DPP_ROW_ROR + 1>(v));
  return v;
}

// sum over all 64 lanes of the wave; every lane ends up with the total (rows by DPP, the 4 row totals by two bpermutes)
__device__ __forceinline__ float wave_sum(float v) {
  v = row16_sum(v);
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
  v = row16_max(v);
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  v = fmaxf(v, __shfl_xor(v, 32, 64));
  return v;
}

typedef float f32x4s __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4s __attribute__((ext_vector_type(4)));

// ---- the two-piece fp16 GEMM form (NP = 2; gemm_nn2.hip, header): power-of-two operand scales from the bit pattern of max |x| (0 for an all-zero operand; inf / nan: scale 1, the result
// is inf / nan as it would be in fp32).  field = biased exponent of the scale that maps [2^e, 2^(e+1)) onto [2^14, 2^15), clamped so
// that its inverse 254 - field is a normal number too.
__host__ __device__ __forceinline__ uint32_t h2_scale_field(uint32_t amax_bits) {
  const int e = (int)((amax_bits >> 23) & 0xFFu);
  if (e == 0xFF) return 127u;
  int f = 268 - e;  // 2^(14 - (e - 127)) = 2^(f - 127)
  f = f < 1 ? 1 : (f > 253 ? 253 : f);
  return (uint32_t)f;
}
__device__ __forceinline__ float h2_field_to_scale(uint32_t f) { return __builtin_bit_cast(float, f << 23); }
// 1 / (s_a s_b) as a float: exponent fields add; clamped into the normal range (a product that leaves it would have left fp32 too)
__device__ __forceinline__ float h2_inv_scale(uint32_t fa, uint32_t fb) {
  int f = (254 - (int)fa) + (254 - (int)fb) - 127;
  f = f < 1 ? 1 : (f > 254 ? 254 : f);
  return __builtin_bit_cast(float, (uint32_t)f << 23);
}
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
// two numbers -> the hi pieces alone (the one-MFMA reduced-precision form, NP = 1)
__device__ __forceinline__ void split1(float x, float y, float s, uint32_t& hi) {
  const f16x2 h = {(_Float16)(x * s), (_Float16)(y * s)};
  hi = __builtin_bit_cast(uint32_t, h);
}
// two numbers -> (hi, lo) pairs packed as fp16x2 dwords; the subtraction is exact (hi is x s rounded to 11 bits)
__device__ __forceinline__ void split2(float x, float y, float s, uint32_t& hi, uint32_t& lo) {
  const float xs = x * s, ys = y * s;
  const f16x2 h = {(_Float16)xs, (_Float16)ys};
  const f16x2 l = {(_Float16)(xs - (float)h[0]), (_Float16)(ys - (float)h[1])};
  hi = __builtin_bit_cast(uint32_t, h);
  lo = __builtin_bit_cast(uint32_t, l);
}
// the partial products of one tile pair, small terms first; a, b: raw 16-byte fragments [piece] of the A and the B operand.  SWAP: the
// MFMA is issued with its operands exchanged (the transposed output tile: gemm_nn2.hip's direct-store epilogue) -- same products, same
// order, so both orientations give the same bits
#define QAGNN_BF(V) __builtin_bit_cast(bf16x8, V)
#define QAGNN_HF(V) __builtin_bit_cast(f16x8, V)
template <int NP, bool SWAP = false>
__device__ __forceinline__ f32x4s mfma_pieces(const u32x4s* __restrict__ a, const u32x4s* __restrict__ b, f32x4s c) {
#define QAGNN_MF3(I, J) c = SWAP ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(QAGNN_BF(b[J]), QAGNN_BF(a[I]), c, 0, 0, 0) \
                                 : __builtin_amdgcn_mfma_f32_16x16x32_bf16(QAGNN_BF(a[I]), QAGNN_BF(b[J]), c, 0, 0, 0);
#define QAGNN_MF2(I, J) c = SWAP ? __builtin_amdgcn_mfma_f32_16x16x32_f16(QAGNN_HF(b[J]), QAGNN_HF(a[I]), c, 0, 0, 0) \
                                 : __builtin_amdgcn_mfma_f32_16x16x32_f16(QAGNN_HF(a[I]), QAGNN_HF(b[J]), c, 0, 0, 0);
  if constexpr (NP == 3) {
    QAGNN_MF3(2, 0) QAGNN_MF3(0, 2) QAGNN_MF3(1, 1) QAGNN_MF3(1, 0) QAGNN_MF3(0, 1) QAGNN_MF3(0, 0)
  } else if constexpr (NP == 2) {
    QAGNN_MF2(1, 0) QAGNN_MF2(0, 1) QAGNN_MF2(0, 0)
  } else {  // NP == 1: the reduced-precision form -- operands rounded to fp16 (11 significant bits) under the same scales, fp32 accumulation
    QAGNN_MF2(0, 0)
  }
#undef QAGNN_MF3
#undef QAGNN_MF2
  return c;
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float dot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
// max(v, lo) that keeps a NaN of v (fmaxf returns the other operand): the ReLU of the BatchNorm operand prologues is torch's, relu(NaN) = NaN.
// For finite v it equals fmaxf(v, lo) up to the sign of zero.
__device__ __forceinline__ float floor_nan(float v, float lo) { return v < lo ? lo : v; }
__device__ __forceinline__ float4 fma4(float s, float4 a, float4 acc) {
  return make_float4(fmaf(s, a.x, acc.x), fmaf(s, a.y, acc.y), fmaf(s, a.z, acc.z), fmaf(s, a.w, acc.w));
}

// Operand maxima for the three-MFMA GEMM form (gemm_nn2.hip).  Agent-scope atomics are executed at the memory side on this chip (the
// eight L2s are not coherent with each other): ~4 ns EACH and serialised per address -- one atomic per wave of a 13 000-block elementwise
// launch (52 000 of them) doubled the whole training step (round 6, visit 2).  So: at most ~1 000 atomics per launch (fat blocks, one
// atomic per BLOCK), and the one-wave-per-node edge kernels store per-node maxima with plain stores that a 64-block kernel reduces.
// The wave reduction stays in the DPP network: rows by row_ror, then row_bcast:15 into rows 1 and 3 and row_bcast:31 into rows 2 and 3
// leave the total in LANE 63 (no LDS round trip).  All 64 lanes must be active; m >= 0.
__device__ __forceinline__ float wave_amax_lane63(float m) {
  m = row16_max(m);
  int b = __builtin_bit_cast(int, m);
  m = fmaxf(m, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(b, b, 0x142, 0xA, 0xF, false)));
  b = __builtin_bit_cast(int, m);
  m = fmaxf(m, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(b, b, 0x143, 0xC, 0xF, false)));
  return m;
}
// max over the block's waves (<= 16), merged into *amax by ONE integer atomic max on the bit pattern (order-independent, hence
// deterministic).  Every thread of the block must call it (it holds a barrier); red: >= 16 floats of LDS.
__device__ __forceinline__ void block_amax_merge(float m, uint32_t* __restrict__ amax, float* __restrict__ red) {
  m = wave_amax_lane63(m);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  if (lane == 63) red[w] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = red[0];
    for (int i = 1; i < nw; ++i) t = fmaxf(t, red[i]);
    if (t > 0.f) __hip_atomic_fetch_max(amax, __builtin_bit_cast(uint32_t, t), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
__device__ __forceinline__ float absmax4(float4 v) { return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))); }


}  // namespace qagnn
