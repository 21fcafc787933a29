// imx_superglue.cpp -- the SuperGlue side of libimx.so: gemm_form() / gemm(), the forms of a linear layer / 1x1 convolution (also
// SuperPoint's convPb / convDb); plan_superglue(), the ONE place a forward's kernel forms are chosen; and
// sg_forward(), which allocates the workspaces, has the plan built and launches from it.
#include "imx_host.h"

#include <cmath>

namespace imx::host {

// Four forms of a plain launch, each with its reason:
//   gemm_small  M <= 4096 rows (one or two pairs): the latency form ("latency_forms": auto / off / on);
//   gemm_x3     the throughput form: fp32 products as six bf16 term products on the bf16 matrix pipe;
//   gemm_tiled  fp32 MFMA: the "mfma" = "f32" A/B reference of the parity tests and the fallback for shapes gemm_x3 rejects;
//   gemm_h2     (the planner's choice only, for the GNN's whole chain: SgPlan::lin_h2) three fp16 plane products, operands scaled by
//               their actual (side, pair) maxima ("linear" = auto / f16x2).
// Measured per layer inside the C3 step (64 pairs, gemm_x3 vs the fp32-MFMA forms of round 2): mlp.0 1.85 vs 2.57 ms, mlp.3
// 1.11 vs 1.45, convPb 0.23 vs 0.51, convDb 0.25 vs 0.35, q|k|v 2.06 vs 2.08.
GemmForm gemm_form(const Options& o, const GemmW& W, const GemmArgs& g) {
  if (gemm_small_supported(g) && (o.latency_forms >= 0 ? o.latency_forms != 0 : g.M <= 4096)) return GemmForm::Small;
  return !o.mfma_f32 && W.wx3 && gemm_x3_supported(g) ? GemmForm::X3 : GemmForm::Tiled;
}

int gemm(imx_handle_t h, hipStream_t s, const char* name, GemmForm form, const GemmW& W, GemmArgs g) {
  if (g.K0 + g.K1 != W.K) return fail(h, "internal: gemm '%s' K mismatch (%d+%d vs %d)", name, g.K0, g.K1, W.K);
  if (form == GemmForm::H2 && h->debug) {        // developer instrumentation: chunk stamps of the first 64 workgroups (all zeros unless gemm_h2.hip was built with -DGH2_TRACE); the LAST launch's stay
    WS(trc, unsigned long long, (std::string("sg.gh2_trace_") + name).c_str(), (size_t)64 * 128 * sizeof(unsigned long long));
    HIP_OK(h, hipMemsetAsync(trc, 0, (size_t)64 * 128 * sizeof(unsigned long long), s));
    g.trace = trc;
    tap(h, (std::string("gh2_trace_") + name).c_str(), trc, {64, 256});
  }
  RUN(name, form == GemmForm::Small ? launch_gemm_small(g, s) : form == GemmForm::H2 ? launch_gemm_h2(g, W.wh2, s) :
            form == GemmForm::Tiled ? launch_gemm(g, s) : launch_gemm_x3(g, W.wx3, s));
  return 0;
}

// ----------------------------------------------------------------------------- SuperGlue: the plan
namespace {

// shapes and workspaces of one forward (allocated before the plan is built: the kernels' predicates see the real arguments)
struct SgWork {
  int B, N0, N1, N0p, N1p, R, d;
  const int32_t *n0, *n1;
  float *x, *att, *qkv, *hid, *mdesc;
  // "attention" = f16x2: the two-plane fp16 form of the throughput attention scales q, k, v by powers of two taken from their maxima
  // over the valid rows of every (side, pair) -- amax: [2 B][4] words per layer, zeroed once per forward; written by the epilogue of the
  // kernel that produces the layer's q|k|v, else by qkv_amax.  amax_x, behind them: one word per (layer, side, pair) for max |x|, the
  // scale of gemm_h2's / gnn_tail_h2's x operand.  Null: no tables ("attention" = bf16x3, "mfma" = f32)
  unsigned *amax, *amax_x;
};
enum class TailForm : unsigned char { LayerSmall, TailH2, TailX3, Unfused };
struct SgLayerPlan {
  bool project;                  // q|k|v is projected here (else the previous layer's fused tail left it)
  GemmForm qkv, mlp1, mlp2;      // the plain linear launches (qkv where `project`, mlp1 / mlp2 where the tail is unfused)
  unsigned char rows_amax;       // rows_amax computes max |x| (nobody left it): 1 = before the projection, 2 = before the tail, 0 = not at all
  bool qkv_amax;                 // the separate pass computes the q|k|v maxima (no epilogue wrote them)
  bool f16x2;                    // the attention's format
  TailForm tail;                 // (its epilogue leaves the NEXT layer's q|k|v maxima where f16x2, and max |x'|: tail_args)
};
struct SgPlan {
  bool small_form;               // the latency forms (one or two pairs; "latency_forms")
  bool epilogue_max;             // the tables exist and a projection's epilogue writes the q|k|v maxima ("qkv_amax" = kernel: never)
  // "linear" = auto / f16x2: the plain linear layers of the GNN -- every layer's q|k|v, mlp.0' and mlp.3 where the tail is not fused
  // (descriptor_dim 256: C5), layer 0's q|k|v and final_proj otherwise -- as gemm_h2.  Decided for the whole chain: the two-plane
  // attention's tables exist and its kernel runs, the throughput forms apply, every matrix passes the spread guard.
  bool lin_h2;
  SgLayerPlan layers[IMX_MAX_GNN_LAYERS];      // (the layer count is bounded at imx_create: no heap per forward)
  bool final_proj, rows_amax_final;     // final_proj is a launch of its own (the last tail is unfused), as final_form
  GemmForm final_form;
};

enum Site { kQkv, kMlp1, kMlp2, kFinal };
const char* const kSiteName[] = {"qkv_proj", "gnn_mlp1", "gnn_mlp2", "final_proj"};
const GemmW& lin_w(imx_handle_t h, Site st, size_t l) {
  return st == kFinal ? h->final_proj : st == kQkv ? h->layers[l].qkv : st == kMlp1 ? h->layers[l].mlp1 : h->layers[l].mlp2;
}
// the arguments of layer l's plain linear launch `st` as form f (kFinal: l = the number of layers)
GemmArgs lin(imx_handle_t h, const SgWork& w, Site st, size_t l, GemmForm f, bool epilogue_max) {
  const GemmW& W = lin_w(h, st, l);
  const int d = w.d;
  unsigned* const tab = w.amax ? w.amax + 8 * w.B * l : nullptr;                   // the layer's q|k|v maxima; [.][3]: max |hidden|
  unsigned* const xmax = w.amax ? w.amax_x + (size_t)2 * w.B * l : nullptr;
  GemmArgs o{};
  if (f == GemmForm::H2 || f == GemmForm::X3Amax) {              // the (side, pair) row structure, and where a q|k|v epilogue leaves its maxima
    o.an0 = w.n0; o.an1 = w.n1; o.aB = w.B; o.aN0p = w.N0p; o.aN1p = w.N1p; o.aN0 = w.N0; o.aN1 = w.N1;
    o.sa0_stride = o.sa1_stride = o.amax_row_stride = 1;
    if (st == kQkv && epilogue_max) o.amax = tab;
  }
  if (f == GemmForm::H2) {
    o.w_inv = W.wh2_inv;
    o.sa0 = xmax;
    if (st == kMlp1) {                   // [x | att]: max |v| bounds att; the epilogue leaves max |hidden|
      o.sa1 = tab; o.sa1_stride = 4; o.sa1_off = 2; o.sa1_cross = h->cfg.gnn_layer_is_cross[l] ? 1 : 0;
      o.amax_row = tab; o.amax_row_stride = 4; o.amax_row_off = 3;
    } else if (st == kMlp2) {            // hidden; the epilogue leaves max |x'|: the next projection's scale
      o.sa0 = tab; o.sa0_stride = 4; o.sa0_off = 3;
      o.amax_row = xmax + 2 * w.B;
    }
  }
  switch (st) {
    case kQkv: return gemm_args(W, w.x, d, d, nullptr, 0, 0, nullptr, 0, w.qkv, 3 * d, w.R, false, o);
    case kMlp1: return gemm_args(W, w.x, d, d, w.att, d, d, nullptr, 0, w.hid, 2 * d, w.R, true, o);   // merge folded in
    case kMlp2: return gemm_args(W, w.hid, 2 * d, 2 * d, nullptr, 0, 0, w.x, d, w.x, d, w.R, false, o);
    default: return gemm_args(W, w.x, d, d, nullptr, 0, 0, nullptr, 0, w.mdesc, d, w.R, false, o);
  }
}
AttnArgs attn_args(imx_handle_t h, const SgWork& w, size_t l, bool f16x2) {
  AttnArgs a{};
  a.qkv = w.qkv; a.out = w.att; a.B = w.B; a.N0p = w.N0p; a.N1p = w.N1p; a.d = w.d; a.heads = HEADS;
  a.n0 = w.n0; a.n1 = w.n1; a.N0 = w.N0; a.N1 = w.N1; a.cross = h->cfg.gnn_layer_is_cross[l];
  a.mfma_f32 = h->opt.mfma_f32; a.latency_forms = h->opt.latency_forms; a.qblocks = h->opt.attention_qblocks;
  if (f16x2) a.amax = w.amax + 8 * w.B * l;
  return a;
}
// The three products after the attention -- mlp.0', mlp.3 + residual and the NEXT layer's q|k|v (final_proj after the last layer) -- in
// ONE launch.  Latency form: gnn_small.hip, the same arithmetic, bit for bit, as the three gemm_small launches it replaces.
const GemmW& next_w(imx_handle_t h, size_t l) { return l + 1 == h->layers.size() ? h->final_proj : h->layers[l + 1].qkv; }
GnnSmallArgs small_args(imx_handle_t h, const SgWork& w, size_t l) {
  const GnnLayer& L = h->layers[l];
  const GemmW& nx = next_w(h, l);
  return GnnSmallArgs{w.x, w.att, L.mlp1.wf, L.mlp1.b, L.mlp2.wf, L.mlp2.b, nx.wf, nx.b, l + 1 == h->layers.size() ? w.mdesc : w.qkv, w.R, w.d, nx.N};
}
// Throughput form (gnn_tail.hip): on the bf16 pipe (FmtX3; "gnn_tail" = auto takes it whenever the latency forms do not apply, so
// results do not depend on the batch size under "latency_forms" = off -- measured against three gemm_x3 launches: 40 vs 50 us at 8224
// rows, 65 vs 86 at 32768, 256 vs 300 at 131072), or as three fp16 plane products (FmtH2) where the two-plane attention runs: its v
// maxima bound att, the maxima of x come from the previous layer's tail, for layer 0 from rows_amax.
GnnTailArgs tail_args(imx_handle_t h, const SgWork& w, size_t l, TailForm form, bool f16x2) {
  const GnnLayer& L = h->layers[l];
  const GemmW& nx = next_w(h, l);
  const bool last = l + 1 == h->layers.size(), h2 = form == TailForm::TailH2;
  GnnTailArgs t{w.x, w.att, L.tail_stream, L.mlp1.b, L.mlp2.b, nx.b, last ? w.mdesc : w.qkv, w.R, w.d, nx.N};
  const bool max_out = f16x2 && !last;         // the next layer's attention takes the same form (same shapes): its maxima come out of this tail
  if (max_out || h2) { t.n0 = w.n0; t.n1 = w.n1; t.B = w.B; t.N0p = w.N0p; t.N1p = w.N1p; t.N0 = w.N0; t.N1 = w.N1; }
  if (max_out) t.amax = w.amax + 8 * w.B * (l + 1);
  if (h2) {
    t.stream_h2 = L.tail_stream_h2;
    t.w1_inv = L.h2c.w1_inv; t.w2_inv = L.h2c.w2_inv; t.w3_inv = L.h2c.w3_inv;
    t.l1_1 = L.h2c.l1_1; t.l1_2 = L.h2c.l1_2; t.bmax_1 = L.bmax_1; t.bmax_2 = L.bmax_2;
    t.amax_x_in = w.amax_x + (size_t)2 * w.B * l; t.amax_v = w.amax + 8 * w.B * l;
    t.amax_x_out = last ? nullptr : w.amax_x + (size_t)2 * w.B * (l + 1);      // (max |x'| for the next layer)
    t.cross = h->cfg.gnn_layer_is_cross[l];
  }
  return t;
}

// Every form of the forward, from the handle (options, weights and their guards) and the shapes; a form whose kernel predicate
// disagrees fails HERE, before anything is launched.  have_*: what the launches planned so far leave behind for the next one.
int plan_superglue(imx_handle_t h, const SgWork& w, SgPlan& P) {
  const Options& o = h->opt;
  const size_t nl = h->layers.size();
  if (nl > IMX_MAX_GNN_LAYERS) return fail(h, "internal: %zu GNN layers", nl);
  const int d = w.d;
  const bool takes_x3 = attention_takes_x3(attn_args(h, w, 0, false));      // (shapes and options only: the same for every layer)
  P.small_form = o.latency_forms >= 0 ? o.latency_forms != 0 : w.R <= 4096;
  // ("qkv_amax" = "kernel": the maxima of a projected q|k|v by the separate pass even where the projection's epilogue can write them --
  // the A/B switch of tests/test_gpu_superglue.py; the two must agree bit for bit)
  P.epilogue_max = w.amax && o.qkv_amax == 0;
  P.lin_h2 = w.amax && !P.small_form && o.linear != 0 && w.N0p % 128 == 0 && w.N1p % 128 == 0 && linear_chain_h2_ok(h) && takes_x3;
  auto linear = [&](Site st, size_t l, GemmForm& f) -> int {
    const GemmW& W = lin_w(h, st, l);
    if (P.lin_h2) {
      f = GemmForm::H2;
      return gemm_h2_weights_ok(W) && gemm_h2_supported(lin(h, w, st, l, f, P.epilogue_max)) ? 0 : fail(h, "internal: gemm '%s' was planned on fp16 planes but cannot run there", kSiteName[st]);
    }
    f = gemm_form(o, W, lin(h, w, st, l, GemmForm::Tiled, false));
    if (f == GemmForm::X3 && st == kQkv && P.epilogue_max && gemm_x3_amax_supported(lin(h, w, st, l, GemmForm::X3Amax, true))) f = GemmForm::X3Amax;
    return 0;
  };
  bool have_qkv = false, have_qkv_max = false, have_x_max = false;
  for (size_t l = 0; l < nl; ++l) {
    const GnnLayer& L = h->layers[l];
    SgLayerPlan& p = P.layers[l] = SgLayerPlan{};
    const bool last = l + 1 == nl;
    const GemmW& nx = next_w(h, l);
    p.project = !have_qkv;
    if (p.project) {
      if (linear(kQkv, l, p.qkv)) return -1;
      if (P.lin_h2 && !have_x_max) p.rows_amax = 1;
      have_x_max = have_x_max || P.lin_h2;
      have_qkv_max = p.qkv == GemmForm::X3Amax || (p.qkv == GemmForm::H2 && P.epilogue_max);
    }
    p.f16x2 = w.amax && takes_x3 && (attn_f16x2_ok(L) || o.attention == 1);   // ("attention" = f16x2 forces it: the guard's A/B)
    // (the maxima also scale gnn_mlp1's [x | att] on the fp16 planes where lin_h2 holds -- max |v| bounds att -- so they are written for
    // every layer then, also where the guard runs this layer's attention on bf16x3)
    p.qkv_amax = (p.f16x2 || P.lin_h2) && !have_qkv_max;
    have_qkv = have_qkv_max = false;
    p.tail = TailForm::Unfused;
    if (P.small_form && o.latency_forms != 2 && L.mlp1.Npad == 2 * d && L.mlp2.Npad == d && nx.Npad == nx.N && gnn_layer_small_supported(small_args(h, w, l))) {
      p.tail = TailForm::LayerSmall;
    } else if (!P.small_form && !o.mfma_f32 && o.gnn_tail != 0 && L.tail_stream && nx.Npad == nx.N && gnn_tail_x3_supported(tail_args(h, w, l, TailForm::TailX3, p.f16x2))) {
      // "gnn_tail" = auto: the fp16 form only where the bounds that scale the operands are tight enough for both planes (L.h2c.loose_*,
      // computed from the weights at imx_finalize_weights); "fused" forces it, "bf16x3" the other
      const bool h2 = p.f16x2 && o.gnn_tail != 2 && L.tail_stream_h2 && (tail_h2_safe(L) || o.gnn_tail == 1) && gnn_tail_h2_supported(tail_args(h, w, l, TailForm::TailH2, p.f16x2));
      p.tail = h2 ? TailForm::TailH2 : TailForm::TailX3;
    }
    bool x_max_out = false;                    // the tail leaves max |x'| for the next layer
    if (p.tail == TailForm::Unfused) {
      if (linear(kMlp1, l, p.mlp1) || linear(kMlp2, l, p.mlp2)) return -1;
      x_max_out = P.lin_h2;
    } else {
      have_qkv = !last;
      have_qkv_max = p.tail != TailForm::LayerSmall && p.f16x2 && !last;
      x_max_out = p.tail == TailForm::TailH2 && !last;
    }
    if ((p.tail == TailForm::TailH2 || (p.tail == TailForm::Unfused && P.lin_h2)) && !have_x_max) p.rows_amax = 2;
    have_x_max = x_max_out;
  }
  P.final_proj = nl == 0 || P.layers[nl - 1].tail == TailForm::Unfused;
  P.rows_amax_final = P.final_proj && P.lin_h2 && !have_x_max;
  return P.final_proj ? linear(kFinal, nl, P.final_form) : 0;
}

}  // namespace

// ----------------------------------------------------------------------------- SuperGlue: the launches
int sg_forward(imx_handle_t h, int B, const SgSide sd[2], int64_t* m0, int64_t* m1, float* ms0, float* ms1, hipStream_t s) {
  if (!h->finalized[IMX_NET_SUPERGLUE]) return fail(h, "SuperGlue weights not finalized");
  const imx_config_t& c = h->cfg;
  const int d = c.descriptor_dim;
  const int N0 = sd[0].N, N1 = sd[1].N;
  if (B <= 0 || N0 < 0 || N1 < 0) return fail(h, "bad SuperGlue shapes B=%d N0=%d N1=%d", B, N0, N1);
  const size_t f = sizeof(float);
  h->sg_last.valid = false;   // (imx_match_loss: nothing of an earlier forward is readable from here on)
  h->sg_last.S = nullptr;
  if (N0 == 0 || N1 == 0) {   // superglue_test.py:235-242 (dtype handling is the Python side's)
    if (N0) { HIP_OK(h, hipMemsetAsync(m0, 0xFF, (size_t)B * N0 * 8, s)); HIP_OK(h, hipMemsetAsync(ms0, 0, (size_t)B * N0 * f, s)); }
    if (N1) { HIP_OK(h, hipMemsetAsync(m1, 0xFF, (size_t)B * N1 * 8, s)); HIP_OK(h, hipMemsetAsync(ms1, 0, (size_t)B * N1 * f, s)); }
    return 0;
  }
  const int N0p = pad32(N0), N1p = pad32(N1);
  const int R = B * (N0p + N1p);
  const size_t off1 = (size_t)B * N0p;   // first row of side 1
  int maxw = d;
  for (int i = 0; i < c.kenc_n; ++i) maxw = std::max(maxw, pad32(c.kenc_channels[i]));      // (as finalize_superglue pads the widths)
  WS(x, float, "sg.x", (size_t)R * d * f);
  WS(ta, float, "sg.ta", (size_t)R * maxw * f);
  WS(tb, float, "sg.tb", (size_t)R * maxw * f);
  WS(qkv, float, "sg.qkv", (size_t)R * 3 * d * f);
  WS(att, float, "sg.att", (size_t)R * d * f);
  WS(hid, float, "sg.hid", (size_t)R * 2 * d * f);
  WS(mdesc, float, "sg.mdesc", (size_t)R * d * f);
  WS(S, float, "sg.S", (size_t)B * N0p * N1p * f);
  WS(uv, float, "sg.uv", ((size_t)B * (N0p + 1) + (size_t)B * (N1p + 1)) * f);     // u then v, contiguous: ONE memset zeroes both
  float* u = uv;
  float* v = uv + (size_t)B * (N0p + 1);
  WS(max0, float, "sg.max0", (size_t)B * N0p * f);
  WS(max1, float, "sg.max1", (size_t)B * N1p * f);
  WS(idx0, int, "sg.idx0", (size_t)B * N0p * 4);
  WS(idx1, int, "sg.idx1", (size_t)B * N1p * 4);

  // every form of the forward, before anything is launched (the tables of maxima: SgWork)
  SgWork w{B, N0, N1, N0p, N1p, R, d, sd[0].n, sd[1].n, x, att, qkv, hid, mdesc, nullptr, nullptr};
  const size_t nl = h->layers.size(), amax_words = nl * 2 * B * 4 + (nl + 1) * 2 * B;
  if (h->opt.attention != 0 && !h->opt.mfma_f32) {
    WS(am, unsigned, "sg.amax", amax_words * 4);
    w.amax = am;
    w.amax_x = am + nl * 2 * B * 4;
  }
  unsigned* const amax = w.amax;
  SgPlan P;
  if (plan_superglue(h, w, P)) return -1;

  // descriptors -> rows; first keypoint-encoder layer (superglue_test.py:245-250): both sides, one launch
  // (with the per-pair counts: rows n[b] .. Np-1 of x and of the encoder's first layer are ZEROS whatever the caller's tensors hold
  // there.  Every later kernel is row-wise or masks by the counts, so a padding row stays finite for the whole forward -- which the
  // bf16x3 and fp32 attention kernels rely on: they mask the SCORES of keys past the count and still multiply those keys' V rows by
  // the zero weights (0 x NaN would reach every query row); only the fp16-plane form zeroes the K / V fragments itself.
  // tests/test_gpu_padding.py fills the caller's padding with NaN / Inf / 3e38 on every form.)
  {
    SgPrologueArgs pa{};
    pa.d = d;
    for (int sidx = 0; sidx < 2; ++sidx) {
      const SgSide& q = sd[sidx];
      const int Np = sidx ? N1p : N0p;
      pa.desc[sidx] = q.desc; pa.sb[sidx] = (long)q.sb; pa.sc[sidx] = (long)q.sc; pa.sn[sidx] = (long)q.sn;
      pa.xrow[sidx] = x + (sidx ? off1 : 0) * d;
      Kenc0Args& k = pa.k[sidx];
      k.kpts = q.kpts; k.scores = q.scores; k.B = B; k.N = q.N; k.Np = Np; k.n = q.n;
      k.cx = (float)q.W / 2.0f; k.cy = (float)q.H / 2.0f;
      k.scaling = (float)std::max(q.W, q.H) * 0.7f;
      k.w = h->kenc0_w; k.bias = h->kenc0_b; k.C1 = h->kenc_c1;
      k.out = ta + (sidx ? off1 : 0) * h->kenc_c1;
    }
    RUN("sg_prologue", launch_sg_prologue(pa, s));
  }
  {
    float* cur = ta;
    float* nxt = tb;
    int curw = h->kenc_c1;
    for (size_t i = 0; i < h->kenc.size(); ++i) {
      const GemmW& g = h->kenc[i];
      const bool last = i + 1 == h->kenc.size();
      if (last) {
        if (gemm(h, s, "kenc", g, gemm_args(g, cur, curw, g.K, nullptr, 0, 0, x, d, x, d, R, false))) return -1;   // desc + kenc(...)
      } else {
        if (gemm(h, s, "kenc", g, gemm_args(g, cur, curw, g.K, nullptr, 0, 0, nullptr, 0, nxt, g.N, R, true))) return -1;
        std::swap(cur, nxt);
        curw = g.N;
      }
    }
  }
  if (h->debug) {
    WS(tk, float, "tap.kenc", (size_t)R * d * f);
    HIP_OK(h, hipMemcpyAsync(tk, x, (size_t)R * d * f, hipMemcpyDeviceToDevice, s));
    tap(h, "kenc", tk, {R, d});
  }
  // attentional GNN (superglue_test.py:122-138)
  if (amax) HIP_OK(h, hipMemsetAsync(amax, 0, amax_words * 4, s));
  auto rows_amax = [&](size_t l) -> int {      // max |x| of the rows about to be projected
    RUN("rows_amax", launch_rows_amax_any(x, d, B, N0p, N1p, sd[0].n, sd[1].n, N0, N1, w.amax_x + (size_t)2 * B * l, s));
    return 0;
  };
  auto linear = [&](Site st, size_t l, GemmForm f) { return gemm(h, s, kSiteName[st], f, lin_w(h, st, l), lin(h, w, st, l, f, P.epilogue_max)); };
  for (size_t l = 0; l < nl; ++l) {
    const SgLayerPlan& p = P.layers[l];
    if (p.rows_amax == 1 && rows_amax(l)) return -1;
    if (p.project && linear(kQkv, l, p.qkv)) return -1;
    const AttnArgs a = attn_args(h, w, l, p.f16x2);
    if (p.qkv_amax) RUN("qkv_amax", launch_qkv_amax(a, amax + 8 * B * l, s));
    RUN("attention", launch_attention(a, s));
    if (p.rows_amax == 2 && rows_amax(l)) return -1;
    switch (p.tail) {
      case TailForm::LayerSmall: RUN("gnn_layer", launch_gnn_layer_small(small_args(h, w, l), s)); break;
      case TailForm::TailH2: RUN("gnn_tail", launch_gnn_tail_h2(tail_args(h, w, l, p.tail, p.f16x2), s)); break;
      case TailForm::TailX3: RUN("gnn_tail", launch_gnn_tail_x3(tail_args(h, w, l, p.tail, p.f16x2), s)); break;
      case TailForm::Unfused: if (linear(kMlp1, l, p.mlp1) || linear(kMlp2, l, p.mlp2)) return -1;
    }
    if (h->debug) {
      std::string nm = "gnn" + std::to_string(l);
      WS(tg, float, "tap." + nm, (size_t)R * d * f);
      HIP_OK(h, hipMemcpyAsync(tg, x, (size_t)R * d * f, hipMemcpyDeviceToDevice, s));
      tap(h, nm.c_str(), tg, {R, d});
    }
  }
  if (P.rows_amax_final && rows_amax(nl)) return -1;
  if (P.final_proj && linear(kFinal, nl, P.final_form)) return -1;
  ScoreArgs sc{mdesc, mdesc + off1 * d, S, B, N0p, N1p, d, (float)(1.0 / std::sqrt((double)d))};
  RUN("score_gemm", launch_score_gemm(sc, s));
  float* part = nullptr;
  if (const int Rs = sinkhorn_slab_rows(N1p)) {
    WS(pt, float, "sg.part", (size_t)B * (N0p / Rs + 1) * (N1p + 1) * 2 * f);
    part = pt;
  }
  SinkhornArgs sk{S, u, v, B, N0p, N1p, sd[0].n, sd[1].n, N0, N1, h->bin_score, c.sinkhorn_iterations, part, h->opt.sinkhorn_group, h->opt.sinkhorn_prefetch};
  // (slabs per workgroup: the group decides the merge order of the column partials, so under "latency_forms" = off the auto rule is
  // evaluated at a fixed batch -- the potentials then do not depend on B, bit for bit)
  if (h->opt.latency_forms == 0 && sk.group == 0) sk.group = sinkhorn_auto_group(N0p, N1p, kSinkhornOffBatch);
  if (part && h->opt.sinkhorn_merge > 0) {       // "sinkhorn_merge" = fused: the slab kernel merges its own column partials (auto = kernel: measured, sg_misc.hip)
    WS(mc, unsigned, "sg.sk_merge_cnt", ((size_t)B + 1) * sizeof(unsigned));
    sk.merge_cnt = mc;
    tap(h, "sk_merge_cnt", mc, {(int64_t)B + 1});          // (word [B] != 0: a merging workgroup gave up waiting -- never seen; the tests read it)
  }
  if (h->debug && part) {        // developer instrumentation: the slab kernel's workgroup lives (all zeros unless sg_misc.hip was built with -DSK_TRACE)
    const int Rs = sinkhorn_slab_rows(N1p), ng = N0p / Rs + 1;
    WS(trc, unsigned long long, "sg.sk_trace", (size_t)B * ng * 8 * sizeof(unsigned long long));
    HIP_OK(h, hipMemsetAsync(trc, 0, (size_t)B * ng * 8 * sizeof(unsigned long long), s));
    sk.trace = trc;
    tap(h, "sk_trace", trc, {(int64_t)B * ng, 16});
  }
  RUN("sinkhorn", launch_sinkhorn(sk, s));
  MatchArgs ma{S, u, v, B, N0p, N1p, sd[0].n, sd[1].n, N0, N1, h->bin_score, c.match_threshold,
               max0, idx0, max1, idx1, m0, m1, ms0, ms1};
  RUN("matches", launch_matches(ma, s));
  tap(h, "x", x, {R, d});
  if (nl) {
    tap(h, "qkv", qkv, {R, 3 * d});                                         // the LAST layer's q|k|v ...
    if (amax) tap(h, "amax", amax + 8 * (size_t)B * (nl - 1), {2 * B, 4});  // ... and its maxima (bit patterns; fetched as floats)
  } else {
    // no GNN layers: nothing wrote sg.qkv in this forward and the table has no layer to point at (nl - 1 would wrap): withdrawn, like
    // "ha_mask" in imx_api.cpp, so that imx_debug_fetch refuses them instead of handing out an earlier forward's or reading wild
    h->taps.erase("qkv");
    h->taps.erase("amax");
  }
  tap(h, "mdesc", mdesc, {R, d});
  tap(h, "scores_in", S, {B, N0p, N1p});
  tap(h, "u", u, {B, N0p + 1});
  tap(h, "v", v, {B, N1p + 1});
  tap(h, "max0", max0, {B, N0p});
  tap(h, "max1", max1, {B, N1p});
  h->sg_last.B = B; h->sg_last.N0 = N0; h->sg_last.N1 = N1; h->sg_last.N0p = N0p; h->sg_last.N1p = N1p;
  h->sg_last.S = S; h->sg_last.u = u; h->sg_last.v = v; h->sg_last.alpha = h->bin_score;      // (readable once sg_keep_counts has run)
  return 0;
}

}  // namespace imx::host
