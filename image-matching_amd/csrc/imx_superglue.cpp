// imx_superglue.cpp -- the SuperGlue launch sequence of libimx.so (sg_forward), with the form planner of its fp16-plane chain, and
// gemm(): the one place a linear layer / 1x1 convolution picks its kernel form (also SuperPoint's convPb / convDb).
#include "imx_host.h"

#include <cmath>

namespace imx::host {

// `ex` (optional; the GNN's linear layers): see GemmExtra in imx_host.h.  ex->done says whether the q|k|v maxima ex->a.amax asks for
// were written from the epilogue (else the caller runs launch_qkv_amax)
int gemm(imx_handle_t h, hipStream_t s, const char* name, const GemmW& W, const float* a0, int lda0, int K0, const float* a1,
         int lda1, int K1, const float* res, int ldr, float* out, int ldo, int M, bool relu, GemmExtra* ex) {
  if (K0 + K1 != W.K) return fail(h, "internal: gemm '%s' K mismatch (%d+%d vs %d)", name, K0, K1, W.K);
  auto with_operands = [&](GemmArgs t) {      // t: the optional fields (all zero for a plain launch)
    t.a0 = a0; t.lda0 = lda0; t.K0 = K0; t.a1 = a1; t.lda1 = lda1; t.K1 = K1; t.w = W.w; t.bias = W.b; t.res = res; t.ldr = ldr;
    t.out = out; t.ldo = ldo; t.M = M; t.N = W.N; t.Npad = W.Npad; t.relu = relu ? 1 : 0;
    return t;
  };
  GemmArgs g = with_operands(GemmArgs{});
  if (ex) { ex->done = false; ex->h2 = false; }
  // Four forms, each with its reason:
  //   gemm_small  M <= 4096 rows (one or two pairs): the latency form ("latency_forms": auto / off / on);
  //   gemm_h2     the GNN's plain linear layers in the throughput path: three fp16 plane products, operands scaled by their actual
  //               (side, pair) maxima ("linear" = auto / f16x2; the caller decides it for the whole chain: want_h2);
  //   gemm_x3     the throughput form of everything else: fp32 products as six bf16 term products on the bf16 matrix pipe;
  //   gemm_tiled  fp32 MFMA: the "mfma" = "f32" A/B reference of the parity tests and the fallback for shapes gemm_x3 rejects.
  // Measured per layer inside the C3 step (64 pairs, gemm_x3 vs the fp32-MFMA forms of round 2): mlp.0 1.85 vs 2.57 ms, mlp.3
  // 1.11 vs 1.45, convPb 0.23 vs 0.51, convDb 0.25 vs 0.35, q|k|v 2.06 vs 2.08.
  const Options& o = h->opt;
  const bool small = gemm_small_supported(g) && (o.latency_forms >= 0 ? o.latency_forms != 0 : M <= 4096);
  const bool x3 = !small && !o.mfma_f32 && W.wx3 && gemm_x3_supported(g);
  if (ex && ex->want_h2) {
    GemmArgs gh = with_operands(ex->a);
    gh.w_inv = W.wh2_inv;
    if (small || o.mfma_f32 || !gemm_h2_weights_ok(W) || !gemm_h2_supported(gh))
      return fail(h, "internal: gemm '%s' was planned on fp16 planes but cannot run there", name);
    ex->done = ex->a.amax != nullptr;
    ex->h2 = true;
    if (h->debug) {        // developer instrumentation: chunk stamps of the first 64 workgroups (all zeros unless gemm_h2.hip was built with -DGH2_TRACE); the LAST launch's stay
      WS(trc, unsigned long long, (std::string("sg.gh2_trace_") + name).c_str(), (size_t)64 * 128 * sizeof(unsigned long long));
      HIP_OK(h, hipMemsetAsync(trc, 0, (size_t)64 * 128 * sizeof(unsigned long long), s));
      gh.trace = trc;
      tap(h, (std::string("gh2_trace_") + name).c_str(), trc, {64, 256});
    }
    RUN(name, launch_gemm_h2(gh, W.wh2, s));
    return 0;
  }
  if (ex && ex->a.amax && x3) {
    const GemmArgs ga = with_operands(ex->a);
    if (gemm_x3_amax_supported(ga)) { g = ga; ex->done = true; }
  }
  RUN(name, small ? launch_gemm_small(g, s) : x3 ? launch_gemm_x3(g, W.wx3, s) : launch_gemm(g, s));
  return 0;
}

// ----------------------------------------------------------------------------- SuperGlue
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
  for (int i = 0; i < c.kenc_n; ++i) maxw = std::max(maxw, c.kenc_channels[i]);
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
        if (gemm(h, s, "kenc", g, cur, curw, g.K, nullptr, 0, 0, x, d, x, d, R, false)) return -1;   // desc + kenc(...)
      } else {
        if (gemm(h, s, "kenc", g, cur, curw, g.K, nullptr, 0, 0, nullptr, 0, nxt, g.N, R, true)) return -1;
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
  // Latency form (one or two pairs; "latency_forms"): the three products after the attention -- mlp.0', mlp.3 + residual and the
  // NEXT layer's q|k|v (final_proj after the last layer) -- are ONE launch per layer (gnn_small.hip; same arithmetic, bit for bit,
  // as the three gemm_small launches it replaces).
  const bool small_form = h->opt.latency_forms >= 0 ? h->opt.latency_forms != 0 : R <= 4096;
  bool have_next = false, have_mdesc = false, have_amax = false;
  // "attention" = f16x2: the two-plane fp16 form of the throughput attention scales q, k, v by powers of two taken from their maxima
  // over the valid rows of every (side, pair) -- [2 B][4] words per layer, zeroed once per forward; written by the fused layer tail that produces the layer's
  // q|k|v (gnn_tail_x3's epilogue), else by qkv_amax (layer 0, whose q|k|v is a plain GEMM; the unfused A/B forms)
  // (the same buffer carries, behind the q / k / v tables, one word per (layer, side, pair) for max |x|: gnn_tail.hip's FmtH2 bounds)
  unsigned* amax = nullptr;
  unsigned* amax_x = nullptr;
  if (h->opt.attention != 0 && !h->opt.mfma_f32) {
    const size_t nl = h->layers.size(), words = nl * 2 * B * 4 + (nl + 1) * 2 * B;
    WS(am, unsigned, "sg.amax", words * 4);
    HIP_OK(h, hipMemsetAsync(am, 0, words * 4, s));
    amax = am;
    amax_x = am + nl * 2 * B * 4;
  }
  long x_max_layer = -1;       // amax_x + 2 B x_max_layer holds max |x| of the CURRENT x (-1: not computed)
  // ("qkv_amax" = "kernel": the maxima of a projected q|k|v by the separate pass even where the projection's epilogue can write them --
  // the A/B switch of tests/test_gpu_superglue.py; the two must agree bit for bit)
  const bool amax_by_kernel = h->opt.qkv_amax != 0;
  // "linear" = auto / f16x2 (round 6): the plain linear layers of the GNN -- every layer's q|k|v, mlp.0' and mlp.3 where the tail is
  // not fused (descriptor_dim 256: C5), layer 0's q|k|v and final_proj otherwise -- as three fp16 plane products (gemm_h2.hip), each
  // operand scaled by its ACTUAL (side, pair) maximum: max |x| from rows_amax (layer 0) or the producing mlp.3's epilogue, max |v|
  // (which bounds the attention output) from the q|k|v epilogue, max |hidden| from mlp.0's.  Decided for the whole chain: the
  // two-plane attention's tables exist and its kernel runs, the throughput forms apply, every matrix passes the spread guard.
  bool lin_h2 = amax && !small_form && h->opt.linear != 0 && N0p % 128 == 0 && N1p % 128 == 0 && R == B * (N0p + N1p) && linear_chain_h2_ok(h);
  {
    AttnArgs a{};
    a.B = B; a.N0p = N0p; a.N1p = N1p; a.d = d; a.heads = HEADS; a.mfma_f32 = h->opt.mfma_f32; a.latency_forms = h->opt.latency_forms;
    lin_h2 = lin_h2 && attention_takes_x3(a);
  }
  const size_t nl_ = h->layers.size();
  auto extra = [&](unsigned* amax_out) {       // the (side, pair) row structure of this forward, and where a q|k|v epilogue should leave its maxima
    GemmExtra e;
    e.a.amax = amax_out; e.a.an0 = sd[0].n; e.a.an1 = sd[1].n; e.a.aB = B; e.a.aN0p = N0p; e.a.aN1p = N1p; e.a.aN0 = N0; e.a.aN1 = N1;
    e.a.sa0_stride = e.a.sa1_stride = e.a.amax_row_stride = 1;
    return e;
  };
  auto x_max_now = [&](size_t l) -> int {      // max |x| of the rows about to be projected, unless the kernel that produced x left it
    if (x_max_layer != (long)l) RUN("rows_amax", launch_rows_amax_any(x, d, B, N0p, N1p, sd[0].n, sd[1].n, N0, N1, amax_x + (size_t)2 * B * l, s));
    x_max_layer = (long)l;
    return 0;
  };
  for (size_t l = 0; l < h->layers.size(); ++l) {
    const GnnLayer& L = h->layers[l];
    if (!have_next) {
      // (the maxima of this q|k|v, if the two-plane attention will want them, out of the projection's epilogue where it can)
      GemmExtra gam = extra(amax && !amax_by_kernel ? amax + 8 * B * l : nullptr);
      if (lin_h2) {
        if (x_max_now(l)) return -1;
        gam.want_h2 = true; gam.a.sa0 = amax_x + (size_t)2 * B * l;
      }
      if (gemm(h, s, "qkv_proj", L.qkv, x, d, d, nullptr, 0, 0, nullptr, 0, qkv, 3 * d, R, false, &gam)) return -1;
      have_amax = gam.done;
    }
    have_next = false;
    AttnArgs a{};
    a.qkv = qkv; a.out = att; a.B = B; a.N0p = N0p; a.N1p = N1p; a.d = d; a.heads = HEADS;
    a.n0 = sd[0].n; a.n1 = sd[1].n; a.N0 = N0; a.N1 = N1; a.cross = c.gnn_layer_is_cross[l];
    a.mfma_f32 = h->opt.mfma_f32; a.latency_forms = h->opt.latency_forms; a.qblocks = h->opt.attention_qblocks;
    const bool f16x2 = amax && attention_takes_x3(a) && (attn_f16x2_ok(L) || h->opt.attention == 1);   // ("attention" = f16x2 forces it: the guard's A/B)
    if (f16x2) a.amax = amax + 8 * B * l;
    // (the maxima also scale gnn_mlp1's [x | att] on the fp16 planes where lin_h2 holds -- max |v| bounds att -- so they are written for
    // every layer then, also where the guard runs this layer's attention on bf16x3)
    if ((f16x2 || lin_h2) && !have_amax) RUN("qkv_amax", launch_qkv_amax(a, amax + 8 * B * l, s));
    have_amax = false;
    RUN("attention", launch_attention(a, s));
    const bool last = l + 1 == h->layers.size();
    const GemmW& nx = last ? h->final_proj : h->layers[l + 1].qkv;
    GnnSmallArgs ga{x, att, L.mlp1.wf, L.mlp1.b, L.mlp2.wf, L.mlp2.b, nx.wf, nx.b, last ? mdesc : qkv, R, d, nx.N};
    // Throughput form: the same three products in one launch on the bf16 pipe (gnn_tail.hip, FmtX3): "gnn_tail" = auto takes it whenever the
    // latency forms do not apply (M > 4096 rows; measured against three gemm_x3 launches: 40 vs 50 us at 8224 rows, 65 vs 86 at 32768,
    // 256 vs 300 at 131072) -- so results do not depend on the batch size under "latency_forms" = off.
    GnnTailArgs ta{x, att, L.tail_stream, L.mlp1.b, L.mlp2.b, nx.b, last ? mdesc : qkv, R, d, nx.N};
    if (f16x2 && !last) {              // the next layer's attention takes the same form (same shapes): its maxima come out of this tail
      ta.amax = amax + 8 * B * (l + 1);
      ta.n0 = sd[0].n; ta.n1 = sd[1].n; ta.B = B; ta.N0p = N0p; ta.N1p = N1p; ta.N0 = N0; ta.N1 = N1;
    }
    const bool tail_ok = !small_form && !h->opt.mfma_f32 && L.tail_stream && nx.Npad == nx.N && gnn_tail_x3_supported(ta);
    const bool tail = tail_ok && h->opt.gnn_tail != 0;
    // "gnn_tail" = auto / fused: the same launch as three fp16 plane products (gnn_tail.hip, FmtH2) where the two-plane attention runs (its
    // v maxima bound att) -- the maxima of x come from the previous layer's tail, for layer 0 from rows_amax
    bool tail_h2 = false;
    // ("auto": only where the bounds that scale the operands are tight enough for both fp16 planes -- L.h2c.loose_*, computed from the
    // weights at imx_finalize_weights; "fused" forces the fp16 form, "bf16x3" the other)
    const bool h2_safe = tail_h2_safe(L);
    if (tail && f16x2 && h->opt.gnn_tail != 2 && L.tail_stream_h2 && (h2_safe || h->opt.gnn_tail == 1)) {
      ta.stream_h2 = L.tail_stream_h2;
      ta.w1_inv = L.h2c.w1_inv; ta.w2_inv = L.h2c.w2_inv; ta.w3_inv = L.h2c.w3_inv;
      ta.l1_1 = L.h2c.l1_1; ta.l1_2 = L.h2c.l1_2; ta.bmax_1 = L.bmax_1; ta.bmax_2 = L.bmax_2;
      ta.amax_x_in = amax_x + (size_t)2 * B * l; ta.amax_v = amax + 8 * B * l; ta.amax_x_out = last ? nullptr : amax_x + (size_t)2 * B * (l + 1);
      ta.cross = c.gnn_layer_is_cross[l];
      ta.n0 = sd[0].n; ta.n1 = sd[1].n; ta.B = B; ta.N0p = N0p; ta.N1p = N1p; ta.N0 = N0; ta.N1 = N1;
      tail_h2 = gnn_tail_h2_supported(ta);
      if (tail_h2 && x_max_now(l)) return -1;
    }
    if (small_form && h->opt.latency_forms != 2 && L.mlp1.Npad == 2 * d && L.mlp2.Npad == d && nx.Npad == nx.N && gnn_layer_small_supported(ga)) {
      RUN("gnn_layer", launch_gnn_layer_small(ga, s));
      have_next = !last;
      have_mdesc = last;
      x_max_layer = -1;
    } else if (tail) {
      RUN("gnn_tail", tail_h2 ? launch_gnn_tail_h2(ta, s) : launch_gnn_tail_x3(ta, s));
      have_next = !last;
      have_mdesc = last;
      have_amax = ta.amax != nullptr;
      x_max_layer = tail_h2 && !last ? (long)l + 1 : -1;     // (the tail's epilogue leaves max |x'| for the next layer)
    } else {
      GemmExtra g1 = extra(nullptr), g2 = g1;
      if (lin_h2) {                      // (x's maximum: this layer's q|k|v projection had it; v's: the attention's table)
        if (x_max_now(l)) return -1;
        g1.want_h2 = true; g1.a.sa0 = amax_x + (size_t)2 * B * l;
        g1.a.sa1 = amax + 8 * B * l; g1.a.sa1_stride = 4; g1.a.sa1_off = 2; g1.a.sa1_cross = c.gnn_layer_is_cross[l] ? 1 : 0;
        g1.a.amax_row = amax + 8 * B * l; g1.a.amax_row_stride = 4; g1.a.amax_row_off = 3;         // max |hidden|: the table's fourth word
        g2.want_h2 = true; g2.a.sa0 = amax + 8 * B * l; g2.a.sa0_stride = 4; g2.a.sa0_off = 3;
        g2.a.amax_row = amax_x + (size_t)2 * B * (l + 1);                                            // max |x'|: the next projection's scale
      }
      if (gemm(h, s, "gnn_mlp1", L.mlp1, x, d, d, att, d, d, nullptr, 0, hid, 2 * d, R, true, &g1)) return -1;   // merge folded in
      if (gemm(h, s, "gnn_mlp2", L.mlp2, hid, 2 * d, 2 * d, nullptr, 0, 0, x, d, x, d, R, false, &g2)) return -1;
      x_max_layer = lin_h2 ? (long)l + 1 : -1;
    }
    if (h->debug) {
      std::string nm = "gnn" + std::to_string(l);
      WS(tg, float, "tap." + nm, (size_t)R * d * f);
      HIP_OK(h, hipMemcpyAsync(tg, x, (size_t)R * d * f, hipMemcpyDeviceToDevice, s));
      tap(h, nm.c_str(), tg, {R, d});
    }
  }
  if (!have_mdesc) {
    GemmExtra gf = extra(nullptr);
    if (lin_h2) {
      if (x_max_now(nl_)) return -1;
      gf.want_h2 = true; gf.a.sa0 = amax_x + (size_t)2 * B * nl_;
    }
    if (gemm(h, s, "final_proj", h->final_proj, x, d, d, nullptr, 0, 0, nullptr, 0, mdesc, d, R, false, &gf)) return -1;
  }
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
  tap(h, "qkv", qkv, {R, 3 * d});                                           // the LAST layer's q|k|v ...
  if (amax) tap(h, "amax", amax + 8 * (size_t)B * (h->layers.size() - 1), {2 * B, 4});      // ... and its maxima (bit patterns; fetched as floats)
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
