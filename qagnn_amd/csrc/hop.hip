// One GATConvE hop of the stack as ONE C call each way: the host-side sequencing of the kernels of this library.
//
// Reference: QAGNN_Message_Passing.mp_helper (modeling/modeling_qagnn.py:45-50) calling GATConvE.forward (:411-452) -> message
// (:455-484) -> mlp (:443, def :408) -> GELU -> dropout, and the autograd backward of all of it.  qagnn_amd/ops.py composes the
// same launches from Python (three autograd operators per hop, ~45 C-ABI calls and ~60 tensor allocations per layer and step);
// at the reference's own mini-batch (2 questions x 5 choices) that host work, not the GPU, bounds the step.  Here the sequence
// is native: 2 calls and a handful of allocations per layer.  The launches, their order and their arguments are exactly those
// of the composed path, so the results are bit-identical (tests/test_hip_kernels.py::test_fused_hop_equals_composed_path).
//
// No allocation, no synchronisation: the caller hands in every buffer, including one scratch region whose size comes from
// qagnn_hop_{fwd,bwd}_workspace_elems().
#include "common.h"
#include "../../include/qagnn_hip_defer.h"

#include <mutex>

namespace qagnn {

static inline int64_t up4(int64_t x) { return (x + 3) & ~(int64_t)3; }
static inline int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }

// rows per tile of the column statistics the first Linear's epilogue leaves (colstat_part: [tiles][3][DP]).  Twins: ST_TILE in elementwise.hip
// (the launch that folds the tiles), SBM in gemm_split.hip (the block that writes one)
static inline int hop_stat_tiles(int N) { return cdiv(N, 128); }
// the widths at which that epilogue exists (twin: nn_validate's cdiv(No, 16) == 13 in gemm_dispatch.hip): there the batch statistics, and with
// them the bound of relu(bn(h1)), ride on the first Linear, so only there does a training hop know every maximum its backward needs
static inline bool hop_stat_width(int DP) { return DP > 192 && DP <= 208; }
// scratch for the packed B image of a hop's NN products (qagnn_gemm_nn_split_ws_f32), in floats: sized for the projection
// [DP | <= DP] -> 3 DP, the largest of them; one buffer, the products of a hop are in order on the main stream
static int64_t hop_pack_elems(int DP) { return up4((qagnn_gemm_nn_pack_bytes(3 * DP, DP, DP) + 3) / 4); }
// rows of the edge backward's class partials (qagnn_hip.h: qagnn_edge_attn_bwd_f32's cls_part; HipGraph.cls_part_rows is the binding's twin)
static inline int hop_cls_part_rows(const qagnn_graph* g) { return QAGNN_CLS_SLICES * g->C + g->max_chunks; }

// The workspace of each direction, stated once: the regions in order (members are initialised in the order they are declared), each padded to 4
// floats.  base == nullptr: only the sizes and `total` mean anything (the size queries, check_hop); else the regions are carved from base.
struct HopWs {
  float* base;
  int64_t total = 0;  // grows region by region
  float* take(int64_t n) { const int64_t o = total; total += up4(n); return base ? base + o : nullptr; }
};
struct HopFwdWs : HopWs {
  const int64_t N, Ep, DP, ampart_elems = max64(N, gelu_amax_scratch_elems(N * DP));
  float* const score = take(Ep * 4);
  float* const crws = take(max64(qagnn_colreduce_workspace_elems(N, DP, 1), hop_stat_tiles(N) * 3 * DP));  // column-reduction / statistics partials
  float* const pkws = take(hop_pack_elems(DP));
  float* const ampart = take(ampart_elems);  // per-node / per-block maxima (qagnn_hop_args.amax)
  static HopFwdWs layout(int N, int Ep, int DP, int /*SP*/, int /*cls_part_rows*/, float* base) { return {{base}, N, Ep, DP}; }
};
struct HopBwdWs : HopWs {
  const int64_t N, Ep, DP, SP, cls_part_rows;
  struct { float *dout, *dh1, *dkmq; } set[2] = {{take(N * DP), take(N * DP), take(N * 3 * DP)},  // what the weight-gradient stream reads,
                                                 {take(N * DP), take(N * DP), take(N * 3 * DP)}};  // twice: it may lag by a whole hop
  float* const drelu = take(N * DP);  // d relu(bn(h1)), then d aggr (main stream only)
  float* const gab = take(Ep * 4);
  float* const rs = take(N * 4);
  float* const cls_part = take(cls_part_rows * 2 * DP);
  float* const tnws = take(max64(max64(qagnn_gemm_tn_workspace_elems(N, DP, DP), qagnn_gemm_tn_workspace_elems(N, DP, 3 * DP)),
                                 SP > 0 ? qagnn_gemm_tn_workspace_elems(N, DP + SP, 3 * DP) : 0));  // split-K partials: weight-gradient stream only
  float* const crws = take(qagnn_colreduce_workspace_elems(N, 3 * DP, 4));  // column-reduction partials: main stream only
  float* const pkws = take(hop_pack_elems(DP));  // packed B images of the data-gradient products: main stream only
  float* const ampart = take(max64(3 * N, gelu_amax_scratch_elems(N * DP)));
  static HopBwdWs layout(int N, int Ep, int DP, int SP, int cls_part_rows, float* base) { return {{base}, N, Ep, DP, SP, cls_part_rows}; }
};

// What a stack's backward may finish after its last hop (include/qagnn_hip_defer.h): the class-table gradient dEkEm and the bias gradient
// db1 of every layer.  Nothing inside the stack reads either, so each hop leaves the partial sums in a region of its own here -- the hops
// share ONE workspace, whose cls_part / crws the next hop overwrites -- and three launches reduce all layers at once.
struct StackDeferWs : HopWs {
  const int64_t N, DP, cls_part_rows, k;
  const int64_t cls_stride = up4(cls_part_rows * 2 * DP), db1_stride = up4(bn_colsum_part_elems((int)N, (int)DP));
  float* const cls_part = take(k * cls_stride);  // layer l: as HopBwdWs::cls_part, l * cls_stride floats in
  float* const db1_part = take(k * db1_stride);  // layer l: the column partials of launch_bn_relu_bwd_colsum
  static StackDeferWs layout(int N, int DP, int cls_part_rows, int k, float* base) { return {{base}, N, DP, cls_part_rows, k}; }
};

static int check_hop(const qagnn_hop_args* h, const char* who, bool bwd = false) {  // bwd: the entry point runs the backward
  QAGNN_REQUIRE(h && h->g, QAGNN_EINVAL, "%s: null argument block / graph", who);
  QAGNN_REQUIRE(h->N == h->g->N && h->N > 0, QAGNN_EINVAL, "%s: N=%d does not match the graph (N=%d)", who, h->N, h->g->N);
  QAGNN_REQUIRE(h->HP > 0 && h->HP % 4 == 0 && h->DP == 4 * h->HP, QAGNN_EINVAL, "%s: DP=%d must be 4*HP (HP=%d)", who, h->DP, h->HP);
  QAGNN_REQUIRE(h->HP <= 64, QAGNN_EUNSUPPORTED, "%s: head pitch HP=%d must be <= 64 (the edge kernels' lane map)", who, h->HP);
  QAGNN_REQUIRE(h->DP % 16 == 0 && h->SP >= 0 && h->SP % 16 == 0, QAGNN_EUNSUPPORTED,
                "%s: DP=%d and SP=%d must be multiples of 16 (GEMM k-tile)", who, h->DP, h->SP);
  QAGNN_REQUIRE(h->T >= 1 && h->T <= 4, QAGNN_EUNSUPPORTED, "%s: %d node types (the type-table gradient handles 1..4)", who, h->T);
  QAGNN_REQUIRE(h->X && h->ntype && h->Wx_t && h->Wx && h->TT && h->EkEm && h->W1t && h->W1 && h->b1 && h->gamma && h->beta &&
                    h->W2t && h->W2 && h->b2,
                QAGNN_EINVAL, "%s: null parameter pointer", who);
  QAGNN_REQUIRE(h->SP == 0 || (h->S && h->Ws_t && h->Ws), QAGNN_EINVAL, "%s: SP=%d but S / Ws_t / Ws missing", who, h->SP);
  QAGNN_REQUIRE(h->KMQ && h->a && h->alpha && h->aggr && h->h1 && h->out && h->stats, QAGNN_EINVAL, "%s: null saved-buffer pointer", who);
  QAGNN_REQUIRE(h->batch_stats || (h->run_mean_p && h->run_var_p), QAGNN_EINVAL, "%s: running statistics missing", who);
  QAGNN_REQUIRE(!h->apply_act || h->y, QAGNN_EINVAL, "%s: apply_act without an output buffer y", who);
  QAGNN_REQUIRE(h->ws, QAGNN_EINVAL, "%s: null workspace", who);
  const int64_t need = bwd ? HopBwdWs::layout(h->N, h->g->Ep, h->DP, h->SP, hop_cls_part_rows(h->g), nullptr).total
                           : HopFwdWs::layout(h->N, h->g->Ep, h->DP, h->SP, 0, nullptr).total;
  QAGNN_REQUIRE(h->ws_elems >= need, QAGNN_EINVAL, "%s: workspace of %lld floats is too small", who, (long long)h->ws_elems);
  return QAGNN_OK;
}

// ---- the three-MFMA GEMM form inside a hop (qagnn_hop_args.amax, gemm_split == 2; arithmetic: gemm_nn2.hip's header) -------------
// Words of a hop's amax block: QAGNN_HOP_AM_*; X and S may live in another hop's block (a chained stack: the previous hop's y IS this hop's X)
struct HopAmax {
  bool on;          // this hop runs the form
  uint32_t* x;      // max |X|   (written by the previous hop's GELU / dropout, or by a reduction pass at the start of the call)
  uint32_t* s;      // max |S|
  uint32_t* y;      // where this hop's GELU / dropout leaves max |y|
  uint32_t* own;    // the hop's own block
  bool h1_pass;     // QAGNN_HOP_AM_H1 from a pass over h1 (the forward-only stack: running statistics give no bound)
};
// The form needs batch statistics (the bound of relu(bn(h1)) comes from them) and pays where products take packed B images
static bool hop_h2(const qagnn_hop_args* h, bool infer = false) {
  // infer (qagnn_stack_infer_f32): running statistics -- max relu(bn(h1)) is then measured, not bounded (HopAmax.h1_pass)
  return h->gemm_split >= 2 && h->amax != nullptr && (infer ? !h->batch_stats : h->batch_stats != 0) && nn_rows_packed(h->N);
}
// the piece count of the scaled forms: two (three MFMAs per product), or with gemm_split == 3 one (the reduced-precision form, one fp16 MFMA)
static int hop_pieces(const qagnn_hop_args* h) { return h->gemm_split == 3 ? 1 : 2; }
// an NN product of the hop in a scaled form: the maxima of its A operands, and the piece count as qagnn_gemm_nn_args takes it (0: its default, two)
static void nn_scaled(const qagnn_hop_args* h, qagnn_gemm_nn_args* a, const uint32_t* am1, const uint32_t* am2 = nullptr) {
  a->a_amax1 = am1, a->a_amax2 = am2, a->pieces = hop_pieces(h) == 1 ? 1 : 0;
}
static HopAmax hop_amax_single(const qagnn_hop_args* h, bool infer = false) {
  HopAmax m{hop_h2(h, infer), nullptr, nullptr, nullptr, h->amax, false};
  m.h1_pass = m.on && infer && hop_stat_width(h->DP);  // (the widths at which the training forward takes the bound: hop_fwd_one)
  if (m.on) {  // (x_amax / s_amax: words the caller's producers filled; read-only here)
    m.x = h->x_amax ? const_cast<uint32_t*>(h->x_amax) : h->amax + QAGNN_HOP_AM_X;
    m.s = h->s_amax ? const_cast<uint32_t*>(h->s_amax) : h->amax + QAGNN_HOP_AM_S;
    m.y = h->amax + QAGNN_HOP_AM_Y;
  }
  return m;
}
// hop l of a stack: X / S words shared along the chain where the tensors are
static HopAmax hop_amax_stack(const qagnn_hop_args* hops, int k, int l, bool infer = false) {
  HopAmax m = hop_amax_single(&hops[l], infer);
  if (!m.on) return m;
  if (l > 0 && hop_h2(&hops[l - 1], infer) && hops[l].X == hops[l - 1].y && hops[l - 1].apply_act && !hops[l].x_amax) m.x = hops[l - 1].amax + QAGNN_HOP_AM_Y;
  if (l > 0 && hop_h2(&hops[0], infer) && hops[l].S == hops[0].S && hops[l].SP == hops[0].SP && !hops[l].s_amax)
    m.s = hops[0].s_amax ? const_cast<uint32_t*>(hops[0].s_amax) : hops[0].amax + QAGNN_HOP_AM_S;
  return m;
}

}  // namespace qagnn

using namespace qagnn;

#define HOP_TRY(call)              \
  do {                             \
    int rc__ = (call);             \
    if (rc__ != QAGNN_OK) return rc__; \
  } while (0)

extern "C" int64_t qagnn_hop_fwd_workspace_elems(int32_t N, int32_t Ep, int32_t DP) { return HopFwdWs::layout(N, Ep, DP, 0, 0, nullptr).total; }
extern "C" int64_t qagnn_hop_bwd_workspace_elems(int32_t N, int32_t Ep, int32_t DP, int32_t SP, int32_t cls_part_rows) {
  return HopBwdWs::layout(N, Ep, DP, SP, cls_part_rows, nullptr).total;
}

// NN product through the kernel family the caller asked for (qagnn_hop_args.gemm_split): the bf16-split kernel takes B in its
// [No][K] layout, which the hop holds for every weight (W and W^T both arrive packed)
static int hop_nn(const qagnn_hop_args* h, const qagnn_gemm_nn_args* a, const float* B1n, int ldn1, const float* B2n, int ldn2, float* pkws, qagnn_stream_t stream) {
  return gemm_nn(NnProduct{a, h->gemm_split != 0, B1n, ldn1, B2n, ldn2, pkws, hop_pack_elems(h->DP) * 4}, (hipStream_t)stream);
}
// weight gradient C = [A1 | A2]^T B over the hop's N rows (A2 == nullptr: one operand); am_*: the operands' maxima -- the scaled form
// the hop asks for where all of them are known (am_b is, in a backward that runs the form), the six-MFMA form otherwise
// g: the hop's graph where B is dK | dM | dQ (the product skips the K / Q work of the graph's dead k-tiles), else nullptr
static int hop_tn(const qagnn_hop_args* h, const float* A1, int Ka1, const float* A2, int Ka2, const float* B, int No, float* C, const float* sc,
                  const float* sh, const uint32_t* am_a1, const uint32_t* am_a2, const uint32_t* am_b, float* tnws, qagnn_stream_t stream,
                  const qagnn_graph* g = nullptr) {
  TnProduct p = tn_product(A1, Ka1, Ka1, A2, Ka2, Ka2, B, No, C, No, h->N, No, sc, sh, tnws, am_a1, am_a2, am_b, hop_pieces(h));
  p.g = g;
  return gemm_tn(p, (hipStream_t)stream);
}

// x_ready / s_ready: the words of X / S already hold this call's maxima (an earlier hop of the stack produced them)
static int hop_fwd_one(const qagnn_hop_args* h, const HopAmax& am, bool x_ready, bool s_ready, qagnn_stream_t stream) {
  const int N = h->N, DP = h->DP, SP = h->SP, Ep = h->g->Ep;
  // (h has passed check_hop, the workspace size included: both entry points validate every hop before the first enqueue)
  const HopFwdWs w = HopFwdWs::layout(N, Ep, DP, SP, 0, h->ws);
  float* mean = h->stats, *var = h->stats + DP, *invstd = h->stats + 2 * DP, *scale = h->stats + 3 * DP, *shift = h->stats + 4 * DP;

  if (am.on) {  // operand maxima nobody left behind: one reduction pass each
    if (!x_ready) HOP_TRY(qagnn_absmax_f32(h->X, (int64_t)N * DP, am.x, stream));
    if (SP > 0 && !s_ready) HOP_TRY(qagnn_absmax_f32(h->S, (int64_t)N * SP, am.s, stream));
  }
  // K | M | Q = [X | S] [Wx ; Ws] + TT[node type]      (project-then-gather: linear_key/msg/query on N node rows, :464-466)
  qagnn_gemm_nn_args ga = {};
  ga.A1 = h->X; ga.lda1 = DP; ga.K1 = DP; ga.B1 = h->Wx_t; ga.ldb1 = 3 * DP;
  if (SP > 0) { ga.A2 = h->S; ga.lda2 = SP; ga.K2 = SP; ga.B2 = h->Ws_t; ga.ldb2 = 3 * DP; }
  ga.C = h->KMQ; ga.ldc = 3 * DP; ga.M = N; ga.No = 3 * DP;
  ga.rowtab = h->TT; ga.ldt = 3 * DP; ga.rowidx = h->ntype;
  if (am.on) nn_scaled(h, &ga, am.x, SP > 0 ? am.s : nullptr);
  HOP_TRY(hop_nn(h, &ga, h->Wx, DP, SP > 0 ? h->Ws : nullptr, SP, w.pkws, stream));
  // attention + aggregation (:442, 455-484)
  HOP_TRY(launch_edge_attn_fwd(h->g, h->KMQ, 3 * DP, h->EkEm, 2 * DP, h->HP, h->qscale, w.score, h->a, h->alpha, h->aggr, DP,
                               am.on ? w.ampart : nullptr, (hipStream_t)stream));
  if (am.on) HOP_TRY(launch_amax_reduce(w.ampart, N, am.own + QAGNN_HOP_AM_AGGR, (hipStream_t)stream));
  // mlp: Linear -> BatchNorm1d -> ReLU -> Linear (:443, 408); BN + ReLU are folded into the second GEMM's operand load
  qagnn_gemm_nn_args g1 = {};
  g1.A1 = h->aggr; g1.lda1 = DP; g1.K1 = DP; g1.B1 = h->W1t; g1.ldb1 = DP; g1.C = h->h1; g1.ldc = DP; g1.M = N; g1.No = DP; g1.bias = h->b1;
  // batch statistics as a by-product of this GEMM's epilogue where the split kernel can provide them (same rule as ops.GatMlpFn)
  const bool fused_stats = h->batch_stats && h->gemm_split && hop_stat_width(DP);
  if (fused_stats) g1.colstat_part = w.crws;
  if (am.on) nn_scaled(h, &g1, am.own + QAGNN_HOP_AM_AGGR);
  HOP_TRY(hop_nn(h, &g1, h->W1, DP, nullptr, 0, w.pkws, stream));
  const double Rd = (double)N;
  const float unbias = (float)(Rd / (Rd - 1.0 > 1.0 ? Rd - 1.0 : 1.0));
  const bool h1_bound = am.on && fused_stats;  // (the bound of relu(bn(h1)) rides on the statistics launch)
  if (fused_stats) {
    QAGNN_REQUIRE(!h->run_mean || (h->run_var && h->d > 0 && h->d % 4 == 0 && h->d <= DP), QAGNN_EINVAL, "hop_fwd: running-stat arguments");
    HOP_TRY(launch_bn_stats_finalize(w.crws, hop_stat_tiles(N), N, DP, h->gamma, h->beta, h->eps, h->stats, h->run_mean, h->run_var, h->num_batches_tracked,
                                     h->d, h->momentum, unbias, h->ones_col, h1_bound ? am.own + QAGNN_HOP_AM_H1 : nullptr, (hipStream_t)stream));
  } else {
    const float* mean_u = mean;
    const float* var_u = var;
    if (h->batch_stats) {
      const float inv_rows = (float)(1.0 / (double)N);  // rounded like the composed path's Python double -> float
      HOP_TRY(qagnn_colreduce_f32(0, h->h1, DP, nullptr, DP, N, DP, nullptr, 1, nullptr, nullptr, nullptr, nullptr, nullptr, inv_rows, mean, w.crws,
                                  stream));
      HOP_TRY(qagnn_colreduce_f32(1, h->h1, DP, nullptr, DP, N, DP, nullptr, 1, mean, nullptr, nullptr, nullptr, nullptr, inv_rows, var, w.crws,
                                  stream));
    } else {
      mean_u = h->run_mean_p;
      var_u = h->run_var_p;
    }
    HOP_TRY(qagnn_bn_finalize_f32(mean_u, var_u, h->gamma, h->beta, h->eps, invstd, scale, shift, DP, h->run_mean, h->run_var,
                                  h->num_batches_tracked, h->dense_pos, h->d, h->momentum, unbias, h->ones_col, stream));
  }
  // the true maximum of relu(bn(h1)): one read of h1 (infer.hip); its partials lie where the edge kernel's were folded from (they fit:
  // qagnn_stack_infer_f32 checks it on the host)
  if (am.h1_pass) {
    HOP_TRY(launch_bn_relu_absmax(h->h1, DP, N, DP, scale, shift, am.own + QAGNN_HOP_AM_H1, w.ampart, (hipStream_t)stream));
  }
  qagnn_gemm_nn_args g2 = {};
  g2.A1 = h->h1; g2.lda1 = DP; g2.K1 = DP; g2.B1 = h->W2t; g2.ldb1 = DP; g2.C = h->out; g2.ldc = DP; g2.M = N; g2.No = DP; g2.bias = h->b2;
  g2.a_scale = scale; g2.a_shift = shift;
  if (h1_bound || am.h1_pass) nn_scaled(h, &g2, am.own + QAGNN_HOP_AM_H1);
  HOP_TRY(hop_nn(h, &g2, h->W2, DP, nullptr, 0, w.pkws, stream));
  if (h->apply_act) {  // X' = dropout(GELU(out))  (:48-49)
    QAGNN_REQUIRE(h->p_drop >= 0.f && h->p_drop < 1.f, QAGNN_EINVAL, "hop_fwd: p=%f", h->p_drop);
    HOP_TRY(launch_gelu_dropout(h->out, nullptr, h->y, (int64_t)N * DP, h->p_drop, h->seed, am.on ? am.y : nullptr, w.ampart, (hipStream_t)stream));
  }
  return QAGNN_OK;
}

extern "C" int qagnn_hop_fwd_f32(const qagnn_hop_args* h, qagnn_stream_t stream) {
  QAGNN_REQUIRE(h, QAGNN_EINVAL, "hop_fwd: null argument block");
  HOP_TRY(check_hop(h, "hop_fwd"));  // (before the first enqueue: a refused hop leaves every buffer as it was)
  const HopAmax am = hop_amax_single(h);
  if (am.on) HOP_TRY(qagnn_zero_words(h->amax, QAGNN_HOP_AMAX_WORDS, stream));
  return hop_fwd_one(h, am, h->x_amax != nullptr, h->s_amax != nullptr, stream);
}

namespace qagnn {

// Events that order the main stream and the weight-gradient stream (qagnn_hop_args.side_stream): created once per device, reused
// round-robin (a wait refers to the record that preceded it, so an event may be recorded again once its wait is enqueued).
constexpr int HOP_MAX_DEV = 16, HOP_EV_POOL = 64;
static hipEvent_t g_hop_ev[HOP_MAX_DEV][HOP_EV_POOL];
static bool g_hop_ev_made[HOP_MAX_DEV];
static std::mutex g_hop_ev_mu;

struct SideSync {
  hipStream_t main, side;  // side == nullptr: everything on `main`, no events
  hipEvent_t* ev;
  int next;
  hipEvent_t take() { return ev[next++ % HOP_EV_POOL]; }
};

static int side_sync_init(SideSync* s, hipStream_t main, hipStream_t side) {
  s->main = main;
  s->side = (side && side != main) ? side : nullptr;
  s->ev = nullptr;
  s->next = 0;
  if (!s->side) return QAGNN_OK;
  int dev = 0;
  hipError_t he = hipGetDevice(&dev);
  QAGNN_REQUIRE(he == hipSuccess && dev >= 0 && dev < HOP_MAX_DEV, QAGNN_EHIP, "hop_bwd: device %d outside the event table", dev);
  std::lock_guard<std::mutex> lk(g_hop_ev_mu);
  if (!g_hop_ev_made[dev]) {
    for (int i = 0; i < HOP_EV_POOL; ++i) {
      he = hipEventCreateWithFlags(&g_hop_ev[dev][i], hipEventDisableTiming);
      QAGNN_REQUIRE(he == hipSuccess, QAGNN_EHIP, "hop_bwd: hipEventCreate failed: %s", hipGetErrorString(he));
    }
    g_hop_ev_made[dev] = true;
  }
  s->ev = g_hop_ev[dev];
  return QAGNN_OK;
}
// `to` continues after everything enqueued on `from` so far
static int stream_after(hipStream_t to, hipStream_t from, hipEvent_t ev) {
  hipError_t he = hipEventRecord(ev, from);
  if (he == hipSuccess) he = hipStreamWaitEvent(to, ev, 0);
  QAGNN_REQUIRE(he == hipSuccess, QAGNN_EHIP, "hop_bwd: stream fork / join failed: %s", hipGetErrorString(he));
  return QAGNN_OK;
}

// One hop's backward.  The four weight-gradient products (and the gradients read off their rows) feed nothing downstream, they are
// latency-bound split-K launches with tiny outputs, and the data-gradient chain next to them is a serial chain of launches: with a
// side stream they leave the chain (fork after each of their operands is complete, join at the end of the stack).  What they read
// from the workspace (d out, d h1, d K|M|Q) lives in buffer set `set`; the caller alternates sets from hop to hop and makes the
// main stream wait for `*done` before it reuses one, so the side stream may lag the main stream by a whole hop.
// d != nullptr: layer l's dEkEm and db1 stop at their partial sums, in d's regions of that layer (stack_bwd_impl finishes them)
static int hop_bwd_one(const qagnn_hop_args* h, const HopAmax& am, SideSync* ss, int set, hipEvent_t* done, const StackDeferWs* d = nullptr, int l = 0) {
  // (h has passed check_hop: stack_bwd_impl validates every hop before the first enqueue)
  QAGNN_REQUIRE(h->dy && h->dWx_t && h->dTT && h->dEkEm && h->dW1t && h->db1 && h->dbn && h->dW2t && h->db2, QAGNN_EINVAL,
                "hop_bwd: null gradient pointer");
  QAGNN_REQUIRE(h->SP == 0 || h->dWs_t, QAGNN_EINVAL, "hop_bwd: dWs_t missing");
  const int N = h->N, DP = h->DP, SP = h->SP, Ep = h->g->Ep;
  const HopBwdWs w = HopBwdWs::layout(N, Ep, DP, SP, hop_cls_part_rows(h->g), h->ws);  // (it fits: check_hop)
  float* const bufA = w.set[set].dout, *const bufC = w.set[set].dh1, *const dKMQ = w.set[set].dkmq, *const bufB = w.drelu;
  const float* mean = h->batch_stats ? h->stats : h->run_mean_p;
  const float* invstd = h->stats + 2 * DP, *scale = h->stats + 3 * DP, *shift = h->stats + 4 * DP;
  const qagnn_stream_t stream = (qagnn_stream_t)ss->main;
  const qagnn_stream_t wstream = (qagnn_stream_t)(ss->side ? ss->side : ss->main);  // where the weight gradients go

  // GELU + dropout backward
  const float* dout = h->dy;
  // (the three-MFMA form in the backward needs every maximum the forward left: the same condition, and h1's bound)
  const bool h2 = am.on && hop_stat_width(DP);
  uint32_t* const w_dout = h2 ? am.own + QAGNN_HOP_AM_DOUT : nullptr, *const w_dh1 = h2 ? am.own + QAGNN_HOP_AM_DH1 : nullptr, *const w_dkmq = h2 ? am.own + QAGNN_HOP_AM_DKMQ : nullptr;
  const uint32_t* const w_h1 = h2 ? am.own + QAGNN_HOP_AM_H1 : nullptr, *const w_aggr = h2 ? am.own + QAGNN_HOP_AM_AGGR : nullptr;
  if (h->apply_act) {
    HOP_TRY(launch_gelu_dropout(h->out, h->dy, bufA, (int64_t)N * DP, h->p_drop, h->seed, w_dout, w.ampart, (hipStream_t)stream));
    dout = bufA;
  } else if (h2) {
    HOP_TRY(qagnn_absmax_f32(dout, (int64_t)N * DP, w_dout, stream));
  }
  if (h->ones_col < 0)
    HOP_TRY(qagnn_colreduce_f32(0, dout, DP, nullptr, DP, N, DP, nullptr, 1, nullptr, nullptr, nullptr, nullptr, nullptr, 1.0f, h->db2, w.crws, stream));
  // second Linear: dW2^T = relu(bn(h1))^T dout, d r = dout W2
  if (ss->side) HOP_TRY(stream_after(ss->side, ss->main, ss->take()));
  HOP_TRY(hop_tn(h, h->h1, DP, nullptr, 0, dout, DP, h->dW2t, scale, shift, w_h1, nullptr, w_dout, w.tnws, wstream));
  // relu(bn(h1)) carries a column of ones there: that row of the weight gradient is the bias gradient (no copy when the caller's db2 IS
  // that row)
  if (h->ones_col >= 0 && h->db2 != h->dW2t + (int64_t)h->ones_col * DP) {
    hipError_t he = hipMemcpyAsync(h->db2, h->dW2t + (int64_t)h->ones_col * DP, (size_t)DP * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)wstream);
    if (he != hipSuccess) { set_error("hop_bwd: db2 copy failed: %s", hipGetErrorString(he)); return QAGNN_EHIP; }
  }
  qagnn_gemm_nn_args gr = {};
  gr.A1 = dout; gr.lda1 = DP; gr.K1 = DP; gr.B1 = h->W2; gr.ldb1 = DP; gr.C = bufB; gr.ldc = DP; gr.M = N; gr.No = DP;
  nn_scaled(h, &gr, w_dout);
  HOP_TRY(hop_nn(h, &gr, h->W2t, DP, nullptr, 0, w.pkws, stream));
  // BatchNorm + ReLU backward: dbn[0] = d beta, dbn[1] = d gamma, then d h1
  HOP_TRY(qagnn_colreduce_f32(2, bufB, DP, h->h1, DP, N, DP, nullptr, 1, mean, invstd, scale, shift, nullptr, 1.0f, h->dbn, w.crws, stream));
  HOP_TRY(launch_bn_relu_bwd_colsum(bufB, h->h1, bufC, DP, N, DP, mean, invstd, scale, shift, h->gamma, h->dbn, h->dbn + DP,
                                    h->batch_stats ? (float)(1.0 / (double)N) : 0.f, nullptr, h->db1, d ? d->db1_part + l * d->db1_stride : w.crws, w_dh1,
                                    d == nullptr, (hipStream_t)stream));
  // first Linear (db1 = colsum(d h1) came out of the pass above)
  if (ss->side) HOP_TRY(stream_after(ss->side, ss->main, ss->take()));
  HOP_TRY(hop_tn(h, h->aggr, DP, nullptr, 0, bufC, DP, h->dW1t, nullptr, nullptr, w_aggr, nullptr, w_dh1, w.tnws, wstream));
  qagnn_gemm_nn_args gg = {};
  gg.A1 = bufC; gg.lda1 = DP; gg.K1 = DP; gg.B1 = h->W1; gg.ldb1 = DP; gg.C = bufB; gg.ldc = DP; gg.M = N; gg.No = DP;
  nn_scaled(h, &gg, w_dh1);
  HOP_TRY(hop_nn(h, &gg, h->W1t, DP, nullptr, 0, w.pkws, stream));
  // attention backward
  HOP_TRY(launch_edge_attn_bwd(h->g, h->KMQ, 3 * DP, h->EkEm, 2 * DP, h->HP, h->qscale, h->a, h->alpha, bufB, DP, dKMQ, h->dEkEm, w.gab, w.rs,
                               d ? d->cls_part + l * d->cls_stride : w.cls_part, h2 ? w.ampart : nullptr, w_dkmq, d == nullptr, (hipStream_t)stream));
  // projection: weight gradients, node-type-table gradient, data gradients
  if (ss->side) HOP_TRY(stream_after(ss->side, ss->main, ss->take()));
  if (SP > 0 && h->dWs_t == h->dWx_t + (int64_t)DP * 3 * DP) {  // the two gradients are one [DP + SP, 3 DP] matrix: one product
    HOP_TRY(hop_tn(h, h->X, DP, h->S, SP, dKMQ, 3 * DP, h->dWx_t, nullptr, nullptr, am.x, am.s, w_dkmq, w.tnws, wstream, h->g));
  } else {
    HOP_TRY(hop_tn(h, h->X, DP, nullptr, 0, dKMQ, 3 * DP, h->dWx_t, nullptr, nullptr, am.x, nullptr, w_dkmq, w.tnws, wstream));
    if (SP > 0) HOP_TRY(hop_tn(h, h->S, SP, nullptr, 0, dKMQ, 3 * DP, h->dWs_t, nullptr, nullptr, am.s, nullptr, w_dkmq, w.tnws, wstream));
  }
  if (SP > 0 && h->tab_col >= 0) {
    // the type indicators ride in S's padding columns: their rows of dWs_t ARE the type-table gradient
    QAGNN_REQUIRE(h->tab_col + h->T <= SP, QAGNN_EINVAL, "hop_bwd: tab_col=%d + T=%d exceeds SP=%d", h->tab_col, h->T, SP);
    if (h->dTT != h->dWs_t + (int64_t)h->tab_col * 3 * DP) {  // (no copy when the caller's dTT IS those rows)
      hipError_t he = hipMemcpyAsync(h->dTT, h->dWs_t + (int64_t)h->tab_col * 3 * DP, (size_t)h->T * 3 * DP * sizeof(float), hipMemcpyDeviceToDevice,
                                     (hipStream_t)wstream);
      if (he != hipSuccess) { set_error("hop_bwd: dTT copy failed: %s", hipGetErrorString(he)); return QAGNN_EHIP; }
    }
  } else {
    HOP_TRY(qagnn_colreduce_f32(0, dKMQ, 3 * DP, nullptr, 3 * DP, N, 3 * DP, h->ntype, h->T, nullptr, nullptr, nullptr, nullptr, nullptr, 1.0f, h->dTT,
                                w.crws, stream));
  }
  if (ss->side) {  // the side stream is done with this buffer set (and with everything queued on it before) once this event fires
    *done = ss->take();
    hipError_t he = hipEventRecord(*done, ss->side);
    QAGNN_REQUIRE(he == hipSuccess, QAGNN_EHIP, "hop_bwd: hipEventRecord failed: %s", hipGetErrorString(he));
  }
  // data gradients dX = dK|dM|dQ Wx and dS = dK|dM|dQ Ws: one launch that reads and splits dK|dM|dQ once where the pair is one the
  // two-output kernel takes (nn_dual_route: the three-MFMA form at (13, 7) column tiles -- bit-identical), else one launch each
  qagnn_gemm_nn_args gx = {}, gs = {};
  if (h->dX) {
    gx.A1 = dKMQ; gx.lda1 = 3 * DP; gx.K1 = 3 * DP; gx.B1 = h->Wx; gx.ldb1 = DP; gx.C = h->dX; gx.ldc = DP; gx.M = N; gx.No = DP;
    gx.accumulate = h->accumulate_dX;
    nn_scaled(h, &gx, w_dkmq);
  }
  if (SP > 0 && h->dS) {
    gs.A1 = dKMQ; gs.lda1 = 3 * DP; gs.K1 = 3 * DP; gs.B1 = h->Ws; gs.ldb1 = SP; gs.C = h->dS; gs.ldc = SP; gs.M = N; gs.No = SP;
    gs.accumulate = h->accumulate_dS;
    nn_scaled(h, &gs, w_dkmq);
  }
  if (h->dX && SP > 0 && h->dS && h->gemm_split != 0 && nn_dual_enabled()) {
    const NnProduct px{&gx, true, h->Wx_t, 3 * DP, nullptr, 0, w.pkws, hop_pack_elems(DP) * 4}, ps{&gs, true, h->Ws_t, 3 * DP, nullptr, 0, nullptr, 0};
    HOP_TRY(nn_validate(px));
    HOP_TRY(nn_validate(ps));
    const NnDualRoute r = nn_dual_route(px, ps);
    if (r.ok) return gemm_nn_dual(px, ps, r, (hipStream_t)stream);
  }
  if (h->dX) HOP_TRY(hop_nn(h, &gx, h->Wx_t, 3 * DP, nullptr, 0, w.pkws, stream));
  if (SP > 0 && h->dS) HOP_TRY(hop_nn(h, &gs, h->Ws_t, 3 * DP, nullptr, 0, w.pkws, stream));
  return QAGNN_OK;
}

// The backward's own maximum words (d out, d h1, d K|M|Q) are merged into by atomic maxima, like every word: they start EVERY backward at
// zero.  The forward zeroes the whole block once; a second backward over the same saved state would otherwise merge into the first one's
// maxima -- still a valid bound, so nothing turns non-finite, the scaled forms only lose the bits by which the gradients have shrunk
// (tests/test_buffer_history.py).  One launch where the hops' blocks are one array (the module mirror's are), one per hop otherwise.
static_assert(QAGNN_HOP_AM_DH1 == QAGNN_HOP_AM_DOUT + 1 && QAGNN_HOP_AM_DKMQ == QAGNN_HOP_AM_DOUT + 2, "the backward's words are three in a row");
__global__ void k_zero_bwd_words(uint32_t* __restrict__ amax, int k) {  // amax: k blocks of QAGNN_HOP_AMAX_WORDS words
  for (int i = threadIdx.x; i < 3 * k; i += blockDim.x) amax[(i / 3) * QAGNN_HOP_AMAX_WORDS + QAGNN_HOP_AM_DOUT + i % 3] = 0u;
}
static int zero_bwd_words(const qagnn_hop_args* hops, int k, hipStream_t main) {
  bool all = true, any = false, one_array = true;
  for (int l = 0; l < k; ++l) {
    const bool h2 = hop_amax_stack(hops, k, l).on && hop_stat_width(hops[l].DP);  // (hop_bwd_one's condition for writing the words)
    all = all && h2;
    any = any || h2;
    one_array = one_array && hops[l].amax != nullptr && hops[l].amax == hops[0].amax + (int64_t)l * QAGNN_HOP_AMAX_WORDS;
  }
  if (!any) return QAGNN_OK;
  if (all && one_array) {
    k_zero_bwd_words<<<1, 64, 0, main>>>(hops[0].amax, k);
    QAGNN_LAUNCH_CHECK("k_zero_bwd_words");
    return QAGNN_OK;
  }
  for (int l = 0; l < k; ++l)
    if (hop_amax_stack(hops, k, l).on && hop_stat_width(hops[l].DP))
      HOP_TRY(qagnn_zero_words(hops[l].amax + QAGNN_HOP_AM_DOUT, 3, (qagnn_stream_t)main));
  return QAGNN_OK;
}

// The deferral needs hops of one shape on one graph (one launch covers all layers) and no more layers than the launches' pointer table
// holds.  A stack that is not is REFUSED when it comes with a deferral workspace: the caller asked for something it would not get
static_assert(DEFER_LAYERS_MAX == QAGNN_DEFER_MAX_HOPS, "the header states the pointer table's length");
static bool stack_defers(const qagnn_hop_args* hops, int k) {
  if (k > DEFER_LAYERS_MAX) return false;
  for (int l = 1; l < k; ++l)
    if (hops[l].g != hops[0].g || hops[l].N != hops[0].N || hops[l].DP != hops[0].DP || hops[l].HP != hops[0].HP) return false;
  return true;
}

// k hops, last first; the buffer sets alternate and the main stream joins the weight-gradient stream before it returns
// defer_ws != nullptr: qagnn_stack_bwd_deferred_f32
static int stack_bwd_impl(const qagnn_hop_args* hops, int k, hipStream_t main, float* defer_ws = nullptr, int64_t defer_elems = 0) {
  // every hop, before an event is recorded or a kernel enqueued: a refused stack leaves every buffer as it was
  for (int l = 0; l < k; ++l) HOP_TRY(check_hop(&hops[l], k > 1 ? "stack_bwd" : "hop_bwd", true));
  const bool defer = defer_ws != nullptr;
  QAGNN_REQUIRE(!defer || stack_defers(hops, k), QAGNN_EUNSUPPORTED,
                "stack_bwd: a deferral workspace with %d hops that do not share one graph, N, DP and HP, or with more than %d hops", k, DEFER_LAYERS_MAX);
  // (without a deferral: the layout of no layers at no address -- nothing reads it)
  const StackDeferWs dws = defer ? StackDeferWs::layout(hops[0].N, hops[0].DP, hop_cls_part_rows(hops[0].g), k, defer_ws) : StackDeferWs::layout(0, 0, 0, 0, nullptr);
  if (defer) {
    QAGNN_REQUIRE(aligned16(defer_ws) && defer_elems >= dws.total, QAGNN_EINVAL, "stack_bwd: deferral workspace of %lld floats is too small (%lld) or unaligned",
                  (long long)defer_elems, (long long)dws.total);
    for (int l = 0; l < k; ++l) QAGNN_REQUIRE(hops[l].dEkEm && hops[l].db1, QAGNN_EINVAL, "stack_bwd: null gradient pointer");
  }
  HOP_TRY(zero_bwd_words(hops, k, main));
  SideSync ss;
  HOP_TRY(side_sync_init(&ss, main, (hipStream_t)hops[k - 1].side_stream));
  hipEvent_t done[2] = {nullptr, nullptr};
  int rc = QAGNN_OK;
  for (int it = 0, l = k - 1; l >= 0 && rc == QAGNN_OK; --l, ++it) {
    const int set = it & 1;
    if (ss.side && done[set]) {  // the hop before last read this set on the side stream
      hipError_t he = hipStreamWaitEvent(ss.main, done[set], 0);
      if (he != hipSuccess) { set_error("stack_bwd: hipStreamWaitEvent failed: %s", hipGetErrorString(he)); rc = QAGNN_EHIP; break; }
    }
    rc = hop_bwd_one(&hops[l], hop_amax_stack(hops, k, l), &ss, set, &done[set], defer ? &dws : nullptr, l);
  }
  // the deferred reductions of all layers, on the main stream behind the last hop: each in the order of additions of its per-hop launch
  if (defer && rc == QAGNN_OK) {
    LayerOut cls = {}, db1 = {};
    for (int l = 0; l < k; ++l) cls.p[l] = hops[l].dEkEm, db1.p[l] = hops[l].db1;
    rc = launch_cls_reduce(hops[0].g, hops[0].HP, dws.cls_part, dws.cls_stride, k, cls, 2 * hops[0].DP, main);
    if (rc == QAGNN_OK) rc = launch_colreduce_final_layers(dws.db1_part, dws.db1_stride, k, db1, hops[0].N, hops[0].DP, main);
  }
  // join even after an error: whatever was forked must not outlive the call (a capture would be left with an unjoined branch)
  if (ss.side) {
    hipEvent_t ev = ss.take();
    hipError_t he = hipEventRecord(ev, ss.side);
    if (he == hipSuccess) he = hipStreamWaitEvent(ss.main, ev, 0);
    if (he != hipSuccess && rc == QAGNN_OK) { set_error("stack_bwd: joining the weight-gradient stream failed: %s", hipGetErrorString(he)); rc = QAGNN_EHIP; }
  }
  return rc;
}

}  // namespace qagnn

extern "C" int qagnn_hop_bwd_f32(const qagnn_hop_args* h, qagnn_stream_t stream) {
  QAGNN_REQUIRE(h, QAGNN_EINVAL, "hop_bwd: null argument block");
  return stack_bwd_impl(h, 1, (hipStream_t)stream);
}

// ---- the whole k-hop stack per call (qagnn_mp_forward / qagnn_mp_backward) -------------------------------------
// hops[l] is a complete qagnn_hop_args; the caller chains them (hops[l+1].X = hops[l].y, hops[l].dy = hops[l+1].dX, shared dS
// with accumulate_dS = 1 on all but the hop whose backward runs first).  Pure sequencing: the same launches, in the same order,
// as k calls of qagnn_hop_fwd_f32 / qagnn_hop_bwd_f32 -- one FFI crossing and one autograd node instead of k for host-bound batches.
static int stack_fwd_impl(const qagnn_hop_args* hops, int32_t k, bool infer, qagnn_stream_t stream) {
  // the hops' amax blocks start at zero: one launch when they are one array (the module mirror's are), one per hop otherwise
  bool any = false, one_array = true;
  for (int l = 0; l < k; ++l) {
    any = any || hop_h2(&hops[l], infer);
    one_array = one_array && hops[l].amax != nullptr && hops[l].amax == hops[0].amax + (int64_t)l * QAGNN_HOP_AMAX_WORDS;
  }
  if (any && one_array) HOP_TRY(qagnn_zero_words(hops[0].amax, (int64_t)k * QAGNN_HOP_AMAX_WORDS, stream));
  for (int l = 0; l < k; ++l) {
    const HopAmax am = hop_amax_stack(hops, k, l, infer);
    if (am.on && !one_array) HOP_TRY(qagnn_zero_words(hops[l].amax, QAGNN_HOP_AMAX_WORDS, stream));
    HOP_TRY(hop_fwd_one(&hops[l], am, am.on && am.x != hops[l].amax + QAGNN_HOP_AM_X, am.on && am.s != hops[l].amax + QAGNN_HOP_AM_S, stream));
  }
  return QAGNN_OK;
}

extern "C" int qagnn_stack_fwd_f32(const qagnn_hop_args* hops, int32_t k, qagnn_stream_t stream) {
  QAGNN_REQUIRE(hops && k > 0, QAGNN_EINVAL, "stack_fwd: no hops");
  for (int l = 0; l < k; ++l) HOP_TRY(check_hop(&hops[l], "stack_fwd"));  // (every hop, before the first enqueue)
  return stack_fwd_impl(hops, k, false, stream);
}

// The forward-only stack (include/qagnn_hip_infer.h): running statistics, no dropout, nothing kept -- the hops may write one shared set
// of result buffers, y alternating between two.  All on one stream, in order: hop l + 1 starts after hop l's last launch, so the only
// aliasing that can go wrong is inside ONE hop, and that is refused here, on the host.
extern "C" int qagnn_stack_infer_f32(const qagnn_hop_args* hops, int32_t k, qagnn_stream_t stream) {
  QAGNN_REQUIRE(hops && k > 0, QAGNN_EINVAL, "stack_infer: no hops");
  for (int l = 0; l < k; ++l) {  // (every hop, before the first enqueue)
    const qagnn_hop_args* h = &hops[l];
    HOP_TRY(check_hop(h, "stack_infer"));
    QAGNN_REQUIRE(!h->batch_stats && h->run_mean_p && h->run_var_p, QAGNN_EINVAL, "stack_infer: hop %d asks for batch statistics", l);
    QAGNN_REQUIRE(!h->run_mean && !h->run_var && !h->num_batches_tracked, QAGNN_EINVAL, "stack_infer: hop %d would update running statistics", l);
    QAGNN_REQUIRE(h->p_drop == 0.f, QAGNN_EINVAL, "stack_infer: hop %d has dropout p=%f", l, h->p_drop);
    // what the hop writes against what it reads, as byte ranges: a result buffer that overlaps X or S anywhere is refused, not only one
    // that starts where they start
    const int64_t row = (int64_t)h->N * h->DP * 4, edges = (int64_t)h->g->Ep * 16;
    const struct { const void* p; int64_t bytes; } wr[] = {{h->KMQ, 3 * row}, {h->a, edges}, {h->alpha, edges}, {h->aggr, row}, {h->h1, row},
                                                           {h->out, row}, {h->stats, (int64_t)5 * h->DP * 4}, {h->apply_act ? h->y : nullptr, row}};
    const struct { const void* p; int64_t bytes; } rd[] = {{h->X, row}, {h->SP > 0 ? h->S : nullptr, (int64_t)h->N * h->SP * 4}};
    for (const auto& w : wr)
      for (const auto& r : rd) {
        const char* const wp = (const char*)w.p, *const rp = (const char*)r.p;
        QAGNN_REQUIRE(!wp || !rp || wp + w.bytes <= rp || rp + r.bytes <= wp, QAGNN_EINVAL,
                      "stack_infer: hop %d writes into one of its own inputs (y over X, or X / S inside its result buffers)", l);
      }
    QAGNN_REQUIRE(qagnn_bn_relu_absmax_scratch_elems(h->N, h->DP) <= HopFwdWs::layout(h->N, h->g->Ep, h->DP, h->SP, 0, nullptr).ampart_elems, QAGNN_EINVAL,
                  "stack_infer: the partial maxima of bn_relu_absmax do not fit the hop workspace");
  }
  return stack_fwd_impl(hops, k, true, stream);
}

extern "C" int qagnn_stack_bwd_f32(const qagnn_hop_args* hops, int32_t k, qagnn_stream_t stream) {
  QAGNN_REQUIRE(hops && k > 0, QAGNN_EINVAL, "stack_bwd: no hops");
  return stack_bwd_impl(hops, k, (hipStream_t)stream);
}

// ---- include/qagnn_hip_defer.h ------------------------------------------------------------------------------------------------------
extern "C" int qagnn_defer_version(void) { return 1; }
extern "C" int64_t qagnn_stack_bwd_defer_elems(int32_t N, int32_t DP, int32_t cls_part_rows, int32_t k) {
  return N > 0 && DP > 0 && cls_part_rows >= 0 && k > 0 ? StackDeferWs::layout(N, DP, cls_part_rows, k, nullptr).total : 0;
}
extern "C" int qagnn_stack_bwd_deferred_f32(const qagnn_hop_args* hops, int32_t k, float* defer_ws, int64_t defer_elems, qagnn_stream_t stream) {
  QAGNN_REQUIRE(hops && k > 0, QAGNN_EINVAL, "stack_bwd: no hops");
  return stack_bwd_impl(hops, k, (hipStream_t)stream, defer_ws, defer_elems);
}
