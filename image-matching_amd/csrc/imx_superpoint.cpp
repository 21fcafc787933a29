// imx_superpoint.cpp -- the SuperPoint side of libimx.so: plan_superpoint(), the ONE place the forms and activation layouts of the
// eight 3x3 convolutions are chosen; sp_detect(), which launches the shared encoder and both heads from that
// plan, then keypoint selection; and descriptor sampling (sp_describe).
#include "imx_host.h"

namespace imx::host {

namespace {

// The eight 3x3 launches: the input is (H >> level) x (W >> level); `swz` marks an output that may be written tile-swizzled (conv2a ->
// conv2b, conv3a -> conv3b, conv4a -> conv4b: whole 8 x 16-pixel tiles, conv3x3_wino24p.hip).  Layer i reads act[i], writes act[i + 1].
struct SpLayer { const char* name; int level; bool pool, first, last, swz; };
constexpr int kSpN = 8;
constexpr SpLayer kSpLayers[kSpN] = {{"conv1ab_pool", 0, true, true, false, false}, {"conv2a", 1, false, false, false, true},
                                  {"conv2b_pool", 1, true, false, false, false}, {"conv3a", 2, false, false, false, true},
                                  {"conv3b_pool", 2, true, false, false, false}, {"conv4a", 3, false, false, false, true},
                                  {"conv4b", 3, false, false, false, false},     {"convPaDa", 3, false, false, true, false}};
// The maxima of the fp16-plane chain live in 256 slots per layer (the kernels' LDS tables): a batch of more than 256 images runs its
// 3x3 layers in slices of 256 images, each with its own tables, so that an image's scales -- and with them its low-order bits -- never
// depend on which other images share the call (tests/test_gpu_superpoint.py: image b of a 260-image batch equals
// the same image alone).
constexpr int kSlice = 256;

struct SpWork {                 // shapes and workspaces of one call
  int B, H, W, split;
  const float *img0, *img1;     // the images below `split`, the others
  float* act[kSpN];             // each layer's output: a1, a2a, a2, a3a, a3, a4a, x4, heads
  unsigned* amax;               // "sp.amax": one word per (slice, layer, image slot b % 256); null: the weights / options rule the chain out
};
enum class ConvForm : unsigned char { Direct, Wino, WinoH, WinoP, C1, C1H, C1P };
constexpr hipError_t (*kConvLaunch[])(const ConvArgs&, hipStream_t) = {launch_conv3x3, launch_conv3x3_wino24, launch_conv3x3_wino24h, launch_conv3x3_wino24p,
                                                                       launch_conv1ab_wino24, launch_conv1ab_wino24h, launch_conv1ab_wino24p};
static_assert(sizeof(kConvLaunch) / sizeof(*kConvLaunch) == (size_t)ConvForm::C1P + 1, "one launcher per ConvForm, in the enum's order");
struct SpStep { ConvForm form; unsigned char in_blocked, out_blocked; };      // (ConvArgs::in_blocked / out_blocked: 0 NHWC, 1 blocked, 2 swizzled)
struct SpPlan {
  // Activations between the Winograd layers are channel-blocked (B, C/8, H, W, 8) -- dense patch loads for the next layer
  // (conv3x3_wino24.hip); the last 3x3 layer writes NHWC rows for the 1x1-conv GEMMs.  "conv" = direct (or a layer the Winograd
  // kernels reject) keeps NHWC everywhere: the direct kernel reads nothing else.
  bool blocked;
  // "conv" = "wino": the Winograd products on the fp16 matrix pipe (conv3x3_wino24h.hip).  Each layer needs an upper bound of |input|
  // per image, written by the PRODUCING layer's epilogue through atomicMax -- the fused first layer starts the chain; and weights whose
  // transformed values fit ONE power-of-two scale per layer (conv_chain_h_ok).  One layer the fp16 kernel rejects, and the whole chain
  // runs the fp32 kernels ("conv" reports it through imx_timing_form).
  bool chain;
  int nslice;
  // det_only (imx_homography_adapt: only `semi` is consumed): 256 = convPa alone.  convPa | convDa share one launch whose Winograd
  // weights are laid out by 64-channel output block, convPa's four first, so a Cout = 256 view of the same buffers IS convPa; the
  // direct form's [9][Cin][Cout] weights have no such prefix: there the shared launch stays and only convDb is skipped.
  int heads_cout;
  // per layer, [0] for the full slices of 256 images, [1] for the last slice (the only one where the chain is off): the fill rules see
  // the slice's image count and nothing else of it, so all full slices take the same forms
  SpStep steps[2][kSpN];
};

// The arguments of layer li on slice sl but for the two layouts: those are the plan's to choose, and no rule below reads them
ConvArgs conv_args(imx_handle_t h, const SpWork& w, const SpPlan& P, int li, int sl) {
  const SpLayer& T = kSpLayers[li];
  const ConvW& cw = h->conv[li];
  const int hh = w.H >> T.level, ww = w.W >> T.level, cout = T.last ? P.heads_cout : cw.cout;
  const int b0 = P.chain ? sl * kSlice : 0, nb = P.chain ? std::min(kSlice, w.B - b0) : w.B;
  // (a slice's images are packed with their layout's own size; the SLICES of a tensor that may be swizzled are spaced by the padded
  // size whatever each slice's layout is -- a short last slice can fall back to the blocked layout, and its region must not start
  // inside the region of the slice before it)
  const size_t ztile = (size_t)((hh + 7) / 8) * ((ww + 15) / 16) * 2048;       // floats per image and 16-channel block of a swizzled tensor
  const size_t in_img = li && kSpLayers[li - 1].swz ? ztile * (cw.cin / 16) : (size_t)hh * ww * (T.first ? 1 : cw.cin);
  const size_t out_img = T.swz ? ztile * (cout / 16) : (size_t)(T.pool ? hh / 2 : hh) * (T.pool ? ww / 2 : ww) * cout;
  ConvArgs a{};
  if (P.chain) {
    unsigned* am = w.amax + (size_t)sl * kSpN * 256;
    a.amax_out = T.last ? nullptr : am + (size_t)li * 256;
    a.amax_in = li > 0 ? am + (size_t)(li - 1) * 256 : nullptr;
    a.wuh = cw.wuh; a.u_scale_inv = cw.su_inv;
    a.c1a_l1 = h->c1a_l1; a.c1a_bmax = h->c1a_bmax;
  }
  a.in = (li ? w.act[li - 1] : w.img0) + (size_t)b0 * in_img;
  if (T.first) {                       // images below `split` come from img0, the others from img1: the slice's view of that
    if (b0 >= w.split) { a.in = w.img1 + (size_t)(b0 - w.split) * in_img; a.split = nb; }
    else { a.in2 = w.img1; a.split = w.split - b0; }
  }
  a.w = cw.w; a.wu24 = cw.wu24; a.bias = cw.b; a.w1 = h->w1; a.b1 = h->b1; a.out = w.act[li] + (size_t)b0 * out_img;
  a.B = nb; a.H = hh; a.W = ww; a.Cin = cw.cin; a.Cout = cout; a.relu = 1; a.pool = T.pool; a.first = T.first;
  return a;
}

// Each kernel predicate once, on conv_args(): the shape rules (*_supported) per layer, on the first slice's arguments -- they read the
// layer's sizes, weights and pool flag (the pooled layers have Cin == Cout: their input-side size limit implies the unpooled output-side
// one), not the image count; the fill rules (*_preferred) per layer on a full slice and on the last
// one.  A tensor is swizzled where its producer AND its consumer run the pair kernel on the slice -- its stores are then 1 KB
// contiguous per instruction ("conv_swizzle" = "off": never; bit-identical either way).
void plan_superpoint(imx_handle_t h, const SpWork& w, bool det_only, SpPlan& P) {
  const Options& o = h->opt;
  P.blocked = !o.conv_direct;
  P.chain = P.blocked && w.amax;
  P.nslice = 1;
  P.heads_cout = h->conv[kSpN - 1].cout;
  bool wino[kSpN] = {};
  for (int li = 1; li < kSpN; ++li) {     // the shape rules of the Winograd kernels and of their fp16 form
    const ConvArgs a = conv_args(h, w, P, li, 0);
    wino[li] = P.blocked && conv3x3_wino24_supported(a);
    P.chain = P.chain && wino[li] && conv3x3_wino24h_supported(a);
  }
  for (int li = 1; li < kSpN; ++li) P.blocked = P.blocked && wino[li];
  P.chain = P.chain && P.blocked;
  if (det_only && P.blocked) {
    P.heads_cout = 256;
    const ConvArgs a = conv_args(h, w, P, kSpN - 1, 0);
    if (!conv3x3_wino24_supported(a) || (P.chain && !conv3x3_wino24h_supported(a))) P.heads_cout = h->conv[kSpN - 1].cout;
  }
  if (P.chain) P.nslice = (w.B + kSlice - 1) / kSlice;
  const bool pairs = P.chain && o.conv_f16 == 1;      // tile pairs where that fills the chip ("conv" = "wino_h": never) -- the same arithmetic, bit for bit
  for (int r = P.nslice > 1 ? 0 : 1; r < 2; ++r) {
    SpStep* st = P.steps[r];
    for (int li = 0; li < kSpN; ++li) {
      st[li] = SpStep{};
      const ConvArgs a = conv_args(h, w, P, li, r ? P.nslice - 1 : 0);
      if (li ? !wino[li] : o.conv_direct) st[li].form = ConvForm::Direct;      // (a layer the Winograd kernels reject, alone: the others keep them, on NHWC)
      else if (li) st[li].form = !P.chain ? ConvForm::Wino : pairs && conv3x3_wino24p_preferred(a) ? ConvForm::WinoP : ConvForm::WinoH;
      else st[li].form = !(P.chain && conv1ab_wino24h_supported(a)) ? ConvForm::C1 : pairs && conv1ab_wino24p_preferred(a) ? ConvForm::C1P : ConvForm::C1H;
    }
    for (int li = 0; li < kSpN; ++li) {
      const bool swz = kSpLayers[li].swz && o.conv_swizzle != 0 && st[li].form == ConvForm::WinoP && st[li + 1].form == ConvForm::WinoP;
      st[li].out_blocked = swz ? 2 : (P.blocked && !kSpLayers[li].last) ? 1 : 0;
      if (li + 1 < kSpN) st[li + 1].in_blocked = st[li].out_blocked;
    }
  }
}

}  // namespace

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
  // Round 6: NMS + threshold + remove_borders leave the detector as candidate BIT rows (20 words per 640-pixel row) and the keypoint kernels
  // count / scatter from those -- the dense where(max_mask, scores, 0) map (a 157-MB write and two reads at C3) is only materialised for
  // the debug tap, for "keypoints" = dense, and where the bit form does not apply (radius > 4 or 0, a negative threshold: there the
  // suppressed zeros pass `> threshold`)
  const bool kp_bits = nms_candidate_bits_supported(c.nms_radius, c.keypoint_threshold) && h->opt.keypoints != 0;
  SpWork w{B, H, W, split, img0, img1, {a1, a2a, a2, a3a, a3, a4a, x4, hd}, nullptr};
  const size_t amax_bytes = (size_t)((B + kSlice - 1) / kSlice) * kSpN * 256 * 4;
  // (the table of the fp16-plane chain, 8 KB per slice, wherever options and weights allow the chain: the planner asks the shape rules
  // with it; on shapes those reject it stays unused and is not zeroed)
  if (!h->opt.conv_direct && conv_chain_h_ok(h) && h->opt.conv_f16 && !h->opt.mfma_f32) {      // (every 3x3 layer, and conv1a's plain output channels)
    WS(am, unsigned, "sp.amax", amax_bytes);
    w.amax = am;
  }
  SpPlan P;
  plan_superpoint(h, w, det_only, P);
  if (P.chain) HIP_OK(h, hipMemsetAsync(w.amax, 0, amax_bytes, s));
  for (int li = 0; li < kSpN; ++li) {
    const char* name = kSpLayers[li].last && P.heads_cout == 256 ? "convPa" : kSpLayers[li].name;
    for (int sl = 0; sl < P.nslice; ++sl) {
      const SpStep& st = P.steps[sl + 1 == P.nslice][li];
      ConvArgs a = conv_args(h, w, P, li, sl);
      a.in_blocked = st.in_blocked; a.out_blocked = st.out_blocked;
      RUN(name, kConvLaunch[(int)st.form](a, s));
    }
  }
  const bool blocked = P.blocked;
  const int hd_ld = P.heads_cout;
  const int rows = B * Hc * Wc;
  if (gemm(h, s, "convPb", h->pb, gemm_args(h->pb, hd, hd_ld, 256, nullptr, 0, 0, nullptr, 0, semi, 65, rows, false))) return -1;
  if (!det_only && gemm(h, s, "convDb", h->db, gemm_args(h->db, hd + 256, 512, 256, nullptr, 0, 0, nullptr, 0, dense, d, rows, false))) return -1;
  h->det_Hc = Hc; h->det_Wc = Wc;
  if (dense_only) { h->det_B = 0; h->nms_lazy.pending = false; return 0; }     // network only (imx_superpoint_dense)
  WS(smap, float, "sp.score_map", (size_t)B * H8 * W8 * f);
  WS(nms, float, "sp.nms", (size_t)B * H8 * W8 * f);
  RUN("softmax_shuffle", launch_softmax_shuffle(semi, 65, smap, B, Hc, Wc, s));
  WS(nms_scratch, unsigned, "sp.nms_scratch", nms_scratch_bytes(B, H8, W8, c.nms_radius));
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
