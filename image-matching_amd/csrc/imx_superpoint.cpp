// imx_superpoint.cpp -- the SuperPoint launch sequence of libimx.so: the shared encoder and both heads (sp_detect), keypoint selection,
// and descriptor sampling (sp_describe).
#include "imx_host.h"

namespace imx::host {

// ----------------------------------------------------------------------------- SuperPoint
int sp_detect(imx_handle_t h, const float* img0, const float* img1, int split, int B, int H, int W, int32_t* counts_out,
              hipStream_t s, bool dense_only, int32_t* counts_lo, int32_t* counts_hi, bool det_only) {
  if (!h->finalized[IMX_NET_SUPERPOINT]) return fail(h, "SuperPoint weights not finalized");
  h->nms_lazy.pending = false;       // (the maps it points at are about to be overwritten; set again at the end of a detect that ran the bit form)
  if (B <= 0 || H < 8 || W < 8) return fail(h, "bad image batch shape B=%d H=%d W=%d", B, H, W);
  const imx_config_t& c = h->cfg;
  const int H2 = H / 2, W2 = W / 2, H4 = H2 / 2, W4 = W2 / 2, Hc = H4 / 2, Wc = W4 / 2, H8 = Hc * 8, W8 = Wc * 8;
  const int d = c.descriptor_dim;
  const size_t f = sizeof(float);
  WS(a1, float, "sp.a1", (size_t)B * H2 * W2 * 64 * f);
  // (a2a / a3a / a4a may be written tile-swizzled -- whole 8 x 16-pixel tiles, conv3x3_wino24p.hip: sized for the padded tile grid)
  auto padded = [](int hh, int ww) { return (size_t)((hh + 7) / 8 * 8) * ((ww + 15) / 16 * 16); };
  WS(a2a, float, "sp.a2a", (size_t)B * padded(H2, W2) * 64 * f);
  WS(a2, float, "sp.a2", (size_t)B * H4 * W4 * 64 * f);
  WS(a3a, float, "sp.a3a", (size_t)B * padded(H4, W4) * 128 * f);
  WS(a3, float, "sp.a3", (size_t)B * Hc * Wc * 128 * f);
  WS(a4a, float, "sp.a4a", (size_t)B * padded(Hc, Wc) * 128 * f);
  WS(x4, float, "sp.x4", (size_t)B * Hc * Wc * 128 * f);
  WS(hd, float, "sp.heads", (size_t)B * Hc * Wc * 512 * f);
  WS(semi, float, "sp.semi", (size_t)B * Hc * Wc * 65 * f);
  // (the descriptor map is not needed by a detector-only forward, the score / NMS maps by neither dense form: at 480 x 640, N = 100
  // that is ~490 MB a homographic-adaptation call never asks for)
  float* dense = nullptr;
  if (!det_only) {
    WS(dense_, float, "sp.dense", (size_t)B * Hc * Wc * d * f);
    dense = dense_;
  }

  // Activations between the Winograd layers are channel-blocked (B, C/8, H, W, 8) -- dense patch loads for the next layer
  // (conv3x3_wino24.hip); the last 3x3 layer writes NHWC rows for the 1x1-conv GEMMs.  IMX_CONV=direct (or a layer the Winograd
  // kernels reject) keeps NHWC everywhere: the direct kernel reads nothing else.
  bool blocked = !h->opt.conv_direct, h_shapes = true;
  {
    const int hs[7] = {H2, H2, H4, H4, Hc, Hc, Hc}, ws_[7] = {W2, W2, W4, W4, Wc, Wc, Wc};
    for (int i = 1; i < 8 && blocked; ++i) {
      ConvArgs t{};
      t.H = hs[i - 1]; t.W = ws_[i - 1]; t.Cin = h->conv[i].cin; t.Cout = h->conv[i].cout; t.wu24 = h->conv[i].wu24;
      blocked = conv3x3_wino24_supported(t);
      // the fp16-plane kernel's OWN predicate, in the same pre-pass (the chain used to be enabled on the fp32 kernel's
      // predicate and a layer the fp16 kernel then rejected was a hard error; now the whole chain falls back to the fp32 kernels)
      t.wuh = h->conv[i].wuh; t.u_scale_inv = h->conv[i].su_inv; t.amax_in = reinterpret_cast<const unsigned*>(h);      // (any non-null pointer: shape check only)
      h_shapes = h_shapes && blocked && conv3x3_wino24h_supported(t);
    }
  }
  // "conv" = "wino": the layers after the first run their Winograd products on the fp16 matrix pipe (conv3x3_wino24h.hip).  Each needs an
  // upper bound of |input| per image: one zeroed word per (layer, image), written by the PRODUCING layer's epilogue through atomicMax --
  // the fused first layer starts the chain, so without it (conv = direct, shapes the Winograd kernels reject) the fp32 forms run
  unsigned* amax = nullptr;
  // ... and weights whose transformed values fit ONE power-of-two scale per layer: a layer whose typical output channel sits more than
  // 2^14 below the largest |U| (a checkpoint with one runaway channel) would push that channel's weights under 2^-3 x 2^13 / 2^14 and
  // lose the low plane -- the whole chain then runs the fp32-MFMA Winograd kernels ("conv" reports it through imx_timing_form)
  const bool all_h = conv_chain_h_ok(h);      // (every 3x3 layer, and conv1a's plain output channels)
  // The maxima live in 256 slots per layer (the kernels' LDS tables): a batch of more than 256 images runs its 3x3 layers in slices of
  // 256 images, each with its own tables, so that an image's scales -- and with them its low-order bits -- never depend on which other
  // images share the call (tests/test_gpu_superpoint.py: image b of a 260-image batch equals the same image alone).
  constexpr int kSlice = 256;
  const int nslice = (B + kSlice - 1) / kSlice;
  if (blocked && all_h && h_shapes && h->opt.conv_f16 && !h->opt.mfma_f32) {
    WS(am, unsigned, "sp.amax", (size_t)nslice * 8 * 256 * 4);          // one word per (slice, layer, image slot b % 256)
    HIP_OK(h, hipMemsetAsync(am, 0, (size_t)nslice * 8 * 256 * 4, s));
    amax = am;
  }
  int layer = 0;
  // conv2a -> conv2b, conv3a -> conv3b, conv4a -> conv4b: the tensor between them is tile-swizzled (ConvArgs::out_blocked / in_blocked
  // = 2) when BOTH layers run the pair kernel on this slice -- its stores are then 1 KB contiguous per instruction
  // (conv3x3_wino24p.hip).  "conv_swizzle" = "off": never (the A/B switch of tools and tests; the results are bit-identical either way).
  const bool swz_on = h->opt.conv_swizzle != 0;
  auto swz_pair = [&](int li_prod, int hh, int ww, int nb) -> bool {
    if (!amax || !swz_on || h->opt.conv_f16 != 1 || (li_prod != 1 && li_prod != 3 && li_prod != 5)) return false;
    for (int k = 0; k < 2; ++k) {
      const ConvW& cw = h->conv[li_prod + k];
      ConvArgs t{};
      t.B = nb; t.H = hh; t.W = ww; t.Cin = cw.cin; t.Cout = cw.cout; t.pool = (k == 1 && li_prod != 5) ? 1 : 0; t.relu = 1;
      t.wu24 = cw.wu24; t.wuh = cw.wuh; t.u_scale_inv = cw.su_inv; t.amax_in = amax;
      if (!conv3x3_wino24p_preferred(t)) return false;
    }
    return true;
  };
  auto conv = [&](const char* name, const ConvW& w, const float* in, float* out, int hh, int ww, bool pool, bool first, bool last = false) -> int {
    const int li = layer++;
    for (int sl = 0; sl < (amax ? nslice : 1); ++sl) {
    ConvArgs a{};
    const int b0 = amax ? sl * kSlice : 0, nb = amax ? std::min(kSlice, B - b0) : B;
    const bool in_z = !first && swz_pair(li - 1, hh, ww, nb), out_z = !first && !pool && !last && swz_pair(li, hh, ww, nb);
    const size_t ztile = (size_t)((hh + 7) / 8) * ((ww + 15) / 16) * 2048;       // floats per image and 16-channel block of a swizzled tensor
    // (a slice's images are packed with their layout's own size; the SLICES of a tensor that may be swizzled are spaced by the padded
    // size whatever each slice's layout is -- a short last slice can fall back to the blocked layout, and its region must not start
    // inside the region of the slice before it)
    const bool in_cand = li == 2 || li == 4 || li == 6, out_cand = li == 1 || li == 3 || li == 5;
    const size_t in_img = in_cand ? ztile * (w.cin / 16) : (size_t)hh * ww * (first ? 1 : w.cin);
    const size_t out_img = out_cand ? ztile * (w.cout / 16) : (size_t)(pool ? hh / 2 : hh) * (pool ? ww / 2 : ww) * w.cout;
    if (amax) {
      unsigned* am = amax + (size_t)sl * 8 * 256;
      a.amax_out = last ? nullptr : am + (size_t)li * 256;
      a.amax_in = li > 0 ? am + (size_t)(li - 1) * 256 : nullptr;
      a.wuh = w.wuh; a.u_scale_inv = w.su_inv;
      a.c1a_l1 = h->c1a_l1; a.c1a_bmax = h->c1a_bmax;
    }
    a.in_blocked = in_z ? 2 : (blocked && !first) ? 1 : 0;
    a.out_blocked = out_z ? 2 : (blocked && !last) ? 1 : 0;
    if (first) {                       // images below `split` come from img0, the others from img1: the slice's view of that
      if (b0 >= split) { a.in = img1 + (size_t)(b0 - split) * in_img; a.in2 = nullptr; a.split = nb; }
      else { a.in = in + (size_t)b0 * in_img; a.in2 = img1; a.split = split - b0; }
    } else {
      a.in = in + (size_t)b0 * in_img; a.in2 = nullptr; a.split = 0;
    }
    a.w = w.w; a.wu24 = w.wu24; a.bias = w.b; a.w1 = h->w1; a.b1 = h->b1; a.out = out + (size_t)b0 * out_img;
    a.B = nb; a.H = hh; a.W = ww; a.Cin = w.cin; a.Cout = w.cout; a.relu = 1; a.pool = pool ? 1 : 0; a.first = first ? 1 : 0;
    const bool fused1 = a.first && a.pool && !h->opt.conv_direct;
    const bool wino = !a.first && !h->opt.conv_direct && conv3x3_wino24_supported(a);
    const bool winoh = wino && amax && conv3x3_wino24h_supported(a);
    if (amax && !fused1 && !winoh) return fail(h, "%s: the fp16-plane Winograd chain needs every layer to take part (internal)", name);
    const bool fused1h = fused1 && amax && conv1ab_wino24h_supported(a);
    // the fp16-plane layers: tile pairs with the positions split over two waves where that fills the chip (conv3x3_wino24p.hip: a U
    // fragment serves two tiles), one tile per workgroup otherwise ("conv" = "wino_h": always) -- the same arithmetic, bit for bit
    const bool winop = winoh && h->opt.conv_f16 == 1 && conv3x3_wino24p_preferred(a);
    const bool fused1p = fused1h && h->opt.conv_f16 == 1 && conv1ab_wino24p_preferred(a);
    if ((in_z || out_z) && !winop) return fail(h, "%s: a tile-swizzled tensor needs the pair kernel on both sides (internal)", name);
    RUN(name, fused1p ? launch_conv1ab_wino24p(a, s) : fused1h ? launch_conv1ab_wino24h(a, s) : fused1 ? launch_conv1ab_wino24(a, s) : winop ? launch_conv3x3_wino24p(a, s) : winoh ? launch_conv3x3_wino24h(a, s) :
              wino ? launch_conv3x3_wino24(a, s) : launch_conv3x3(a, s));
    }
    return 0;
  };
  if (conv("conv1ab_pool", h->conv[0], img0, a1, H, W, true, true)) return -1;
  if (conv("conv2a", h->conv[1], a1, a2a, H2, W2, false, false)) return -1;
  if (conv("conv2b_pool", h->conv[2], a2a, a2, H2, W2, true, false)) return -1;
  if (conv("conv3a", h->conv[3], a2, a3a, H4, W4, false, false)) return -1;
  if (conv("conv3b_pool", h->conv[4], a3a, a3, H4, W4, true, false)) return -1;
  if (conv("conv4a", h->conv[5], a3, a4a, Hc, Wc, false, false)) return -1;
  if (conv("conv4b", h->conv[6], a4a, x4, Hc, Wc, false, false)) return -1;
  // det_only (imx_homography_adapt: only `semi` is consumed): the descriptor head is not run.  convPa | convDa share one launch whose
  // Winograd weights are laid out by 64-channel output block, convPa's four blocks first, so a Cout = 256 view of the same buffers IS
  // convPa alone; the direct form's [9][Cin][Cout] weights have no such prefix, so there (and where the Winograd kernels reject the
  // narrower shape) the shared launch stays and only convDb is skipped.
  ConvW heads = h->conv[7];
  int hd_ld = 512;
  if (det_only && blocked) {
    ConvArgs t{};
    t.B = std::min(B, kSlice); t.H = Hc; t.W = Wc; t.Cin = heads.cin; t.Cout = 256; t.wu24 = heads.wu24;
    bool ok = conv3x3_wino24_supported(t);
    if (ok && amax) { t.wuh = heads.wuh; t.u_scale_inv = heads.su_inv; t.amax_in = amax; ok = conv3x3_wino24h_supported(t); }
    if (ok) { heads.cout = 256; hd_ld = 256; }
  }
  if (conv(hd_ld == 256 ? "convPa" : "convPaDa", heads, x4, hd, Hc, Wc, false, false, true)) return -1;
  const int rows = B * Hc * Wc;
  if (gemm(h, s, "convPb", h->pb, hd, hd_ld, 256, nullptr, 0, 0, nullptr, 0, semi, 65, rows, false)) return -1;
  if (!det_only && gemm(h, s, "convDb", h->db, hd + 256, 512, 256, nullptr, 0, 0, nullptr, 0, dense, d, rows, false)) return -1;
  h->det_Hc = Hc; h->det_Wc = Wc;
  if (dense_only) { h->det_B = 0; h->nms_lazy.pending = false; return 0; }     // network only (imx_superpoint_dense)
  WS(smap, float, "sp.score_map", (size_t)B * H8 * W8 * f);
  WS(nms, float, "sp.nms", (size_t)B * H8 * W8 * f);
  RUN("softmax_shuffle", launch_softmax_shuffle(semi, 65, smap, B, Hc, Wc, s));
  WS(nms_scratch, unsigned, "sp.nms_scratch", nms_scratch_bytes(B, H8, W8, c.nms_radius));
  // Round 6: NMS + threshold + remove_borders leave the detector as candidate BIT rows (20 words per 640-pixel row) and the keypoint kernels
  // count / scatter from those -- the dense where(max_mask, scores, 0) map (a 157-MB write and two reads at C3) is only materialised for
  // the debug tap, for "keypoints" = dense, and where the bit form does not apply (radius > 4 or 0, a negative threshold: there the
  // suppressed zeros pass `> threshold`)
  const bool kp_bits = nms_candidate_bits_supported(c.nms_radius, c.keypoint_threshold) && h->opt.keypoints != 0;
  if (kp_bits) RUN("nms", launch_nms_candidate_bits(smap, B, H8, W8, c.nms_radius, c.keypoint_threshold, c.remove_borders, s, nms_scratch));
  else RUN("nms", launch_nms(smap, nms, B, H8, W8, c.nms_radius, s, nms_scratch));

  const int Ksel = c.max_keypoints >= 0 ? (c.max_keypoints > 0 ? c.max_keypoints : 1) : H8 * W8;
  KeypointArgs k{};
  k.nms = kp_bits ? nullptr : nms; k.cand_bits = kp_bits ? nms_scratch : nullptr; k.scores = smap; k.B = B; k.H = H8; k.W = W8; k.threshold = c.keypoint_threshold; k.border = c.remove_borders;
  k.max_keypoints = c.max_keypoints; k.Ksel = Ksel;
  WS(row_count, int, "kp.row_count", (size_t)B * H8 * 4);
  WS(row_off, int, "kp.row_off", (size_t)B * H8 * 4);
  WS(cand_count, int, "kp.cand_count", (size_t)B * 4);
  WS(cand_idx, int, "kp.cand_idx", (size_t)B * H8 * W8 * 4);
  WS(cand_score, float, "kp.cand_score", (size_t)B * H8 * W8 * 4);
  WS(sel_count, int, "kp.sel_count", (size_t)B * 4);
  WS(sel_idx, int, "kp.sel_idx", (size_t)B * Ksel * 4);
  WS(sel_score, float, "kp.sel_score", (size_t)B * Ksel * 4);
  k.row_count = row_count; k.row_off = row_off; k.cand_count = cand_count; k.cand_idx = cand_idx; k.cand_score = cand_score;
  k.sel_count = sel_count; k.sel_idx = sel_idx; k.sel_score = sel_score;
  k.counts_out[0] = counts_out; k.counts_out[1] = counts_lo; k.counts_out[2] = counts_hi; k.counts_split = split;   // written by kp_topk itself
  if (c.max_keypoints > 16384) {      // beyond the LDS sort of kp_topk: its sort slots live in HBM (slow, but nothing is refused)
    size_t P = 1;
    while (P < (size_t)c.max_keypoints) P <<= 1;
    WS(slots, unsigned long long, "kp.sort_slots", (size_t)B * P * 8);
    k.sort_scratch = slots;
  }
  RUN("keypoints", launch_keypoints(k, s));

  h->det_B = B; h->det_H = H; h->det_W = W; h->det_Hc = Hc; h->det_Wc = Wc; h->det_Ksel = Ksel;
  tap(h, "a1", a1, {B, H2, W2, 64}, blocked);
  tap(h, "a2", a2, {B, H4, W4, 64}, blocked);
  tap(h, "a3", a3, {B, Hc, Wc, 128}, blocked);
  tap(h, "x4", x4, {B, Hc, Wc, 128}, blocked);
  tap(h, "semi", semi, {B, Hc, Wc, 65});
  tap(h, "desc_raw", dense, {B, Hc, Wc, d});
  tap(h, "score_map", smap, {B, H8, W8});
  // the "nms" tap: the dense map is materialised only if somebody fetches it (after the keypoints: the pass overwrites the bit rows)
  h->nms_lazy.smap = smap; h->nms_lazy.nms = nms; h->nms_lazy.scratch = nms_scratch; h->nms_lazy.B = B; h->nms_lazy.H = H8; h->nms_lazy.W = W8;
  h->nms_lazy.radius = c.nms_radius; h->nms_lazy.pending = kp_bits;
  tap(h, "nms", nms, {B, H8, W8});
  return 0;
}

int sp_describe(imx_handle_t h, int b0, int B, int Kcap, float* kpts, float* scores, float* desc, hipStream_t s,
                int split, float* kpts2, float* scores2, float* desc2) {
  if (h->det_B <= 0 || b0 + B > h->det_B) return fail(h, "describe: no matching imx_superpoint_detect (B=%d, detect B=%d)", B, h->det_B);
  DescribeArgs a{};
  a.dense = static_cast<const float*>(h->bufs["sp.dense"].p);
  a.ld = h->cfg.descriptor_dim; a.d = h->cfg.descriptor_dim; a.Hc = h->det_Hc; a.Wc = h->det_Wc; a.W8 = h->det_Wc * 8;
  a.sel_count = static_cast<const int*>(h->bufs["kp.sel_count"].p);
  a.sel_idx = static_cast<const int*>(h->bufs["kp.sel_idx"].p);
  a.sel_score = static_cast<const float*>(h->bufs["kp.sel_score"].p);
  a.Ksel = h->det_Ksel; a.b0 = b0; a.B = B; a.Kcap = Kcap; a.kpts = kpts; a.scores = scores; a.desc = desc;
  a.split = split >= 0 ? split : B; a.kpts2 = kpts2; a.scores2 = scores2; a.desc2 = desc2;
  a.align_corners = h->cfg.align_corners; a.dense_eps = h->cfg.sp_variant == IMX_SP_VARIANT_OFFICIAL ? 1 : 0;
  RUN("describe", launch_describe(a, s));
  return 0;
}

}  // namespace imx::host
