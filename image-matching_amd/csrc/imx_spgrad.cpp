// imx_spgrad.cpp -- a host unit of libimx_train.so (include/imx_train.h), on the handle libimx.so made: the two SuperPoint training
// losses as value-and-gradient calls, imx_detector_loss_grad and imx_desc_loss_sparse_grad.  The values come from the forward's own
// launchers (sptrain.hip, linked once into the library: one definition of the device code), the gradients from spgrad.hip.  Every
// scratch buffer ("spg.*") is written in full, or as far as it is read, by the call that reads it.
#include "imx_host.h"
#include "../../include/imx_train.h"

namespace {
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
}  // namespace

extern "C" {

int imx_detector_loss_grad(imx_handle_t h, const float* semi_dev, const float* labels_dev, const float* mask_dev, int B, int H, int W,
                           const float* gout_dev, float* out_dev, float* grad_semi_dev, void* stream) {
  return on_device(h, "imx_detector_loss_grad", [&]() -> int {
    if (B < 1 || H < 8 || W < 8 || H % 8 || W % 8 || (int64_t)B * (H / 8) * (W / 8) > (1 << 30))
      return fail(h, "imx_detector_loss_grad: bad shape B=%d H=%d W=%d (H, W multiples of 8)", B, H, W);
    if (!semi_dev || !labels_dev || !mask_dev || !out_dev || !grad_semi_dev) return fail(h, "imx_detector_loss_grad: null argument");
    if (!aligned16(labels_dev) || !aligned16(mask_dev)) return fail(h, "imx_detector_loss_grad: labels_dev and mask_dev must be 16-byte aligned");
    hipStream_t s = as_stream(stream);
    const int Hc = H / 8, Wc = W / 8;
    WS(part, double, "spg.det_part", (size_t)2 * detector_loss_blocks(B, Hc, Wc) * sizeof(double));
    RUN("detector_loss", launch_detector_loss(semi_dev, labels_dev, mask_dev, B, Hc, Wc, part, out_dev, s));
    RUN("detector_loss_grad", launch_detector_loss_grad(semi_dev, labels_dev, mask_dev, B, Hc, Wc, out_dev, gout_dev, grad_semi_dev, s));
    return 0;
  });
}

int imx_desc_loss_sparse_grad(imx_handle_t h, const float* desc_a_dev, const float* desc_b_dev, int B, int d, int Hc, int Wc,
                              const float* hcell_dev, const int32_t* choice_dev, const int32_t* nonmatch_b_dev, int M, int R, float lamda_d,
                              float margin, int method, const float* gout_dev, float* out_dev, float* mean_dev, int32_t* pairs_dev,
                              int32_t* flag_dev, float* grad_a_dev, float* grad_b_dev, void* stream) {
  return on_device(h, "imx_desc_loss_sparse_grad", [&]() -> int {
    if (B < 1 || B > 32767 || Hc < 1 || Wc < 1 || (int64_t)Hc * Wc > (1 << 24) || M < 1 || R < 1 || (int64_t)B * M * R > (1ll << 31))
      return fail(h, "imx_desc_loss_sparse_grad: bad shape B=%d Hc=%d Wc=%d M=%d R=%d (B in [1,32767], Hc Wc <= 2^24, B M R <= 2^31)", B, Hc, Wc, M, R);
    if (d < 4 || d % 4 || d > 512) return fail(h, "imx_desc_loss_sparse_grad: descriptor dimension %d must be a multiple of 4 in [4,512]", d);
    if (method != 1 && method != 2) return fail(h, "imx_desc_loss_sparse_grad: method must be 1 ('1d') or 2 ('2d'), got %d", method);
    if (!desc_a_dev || !desc_b_dev || !hcell_dev || !choice_dev || !nonmatch_b_dev || !out_dev || !mean_dev || !grad_a_dev || !grad_b_dev)
      return fail(h, "imx_desc_loss_sparse_grad: null argument");
    const int64_t K = desc_grad_slots(R, method == 2), E = (int64_t)M * K;
    if (E > (1ll << 30)) return fail(h, "imx_desc_loss_sparse_grad: M (R + %d) = %lld entries per image exceed 2^30", (int)(K - R), (long long)E);
    hipStream_t s = as_stream(stream);
    const size_t N = (size_t)Hc * Wc;
    WS(ta, float, "spg.desc_a_t", (size_t)B * N * d * sizeof(float));
    WS(tb, float, "spg.desc_b_t", (size_t)B * N * d * sizeof(float));
    WS(pairs, int, "spg.pairs", (size_t)B * N * 2 * sizeof(int));
    WS(nvalid, int, "spg.nvalid", (size_t)B * sizeof(int));
    WS(partial, float, "spg.partial", (size_t)B * M * 3 * sizeof(float));
    DescGradArgs g{};
    DescLossArgs& a = g.f;
    a.desc_a = desc_a_dev; a.desc_b = desc_b_dev; a.hcell = hcell_dev; a.choice = choice_dev; a.nonmatch = nonmatch_b_dev;
    a.B = B; a.d = d; a.Hc = Hc; a.Wc = Wc; a.M = M; a.R = R; a.lamda_d = lamda_d; a.margin = margin; a.method2d = method == 2;
    a.ta = ta; a.tb = tb; a.pairs = pairs; a.nvalid = nvalid; a.partial = partial;
    a.out = out_dev; a.mean = mean_dev; a.pairs_out = pairs_dev; a.flag = flag_dev;
    RUN("desc_loss_sparse", launch_desc_loss_sparse(a, s));
    g.S = desc_grad_segments(E);
    g.seg = (int)((E + g.S - 1) / g.S);
    WS(xm, float, "spg.xm", (size_t)B * M * d * sizeof(float));
    WS(ym, float, "spg.ym", (size_t)B * M * d * sizeof(float));
    WS(an, float, "spg.an", (size_t)B * M * d * sizeof(float));
    WS(ia, int, "spg.ia", (size_t)B * M * sizeof(int));
    WS(keys, int, "spg.keys", (size_t)B * E * sizeof(int));
    WS(coef, float, "spg.coef", (size_t)B * E * sizeof(float));
    WS(hist, int, "spg.hist", (size_t)B * g.S * 2 * N * sizeof(int));
    WS(offs, int, "spg.offs", (size_t)B * (2 * N + 1) * sizeof(int));
    WS(list, int, "spg.list", (size_t)B * E * sizeof(int));
    WS(gt, float, "spg.grad_t", (size_t)B * 2 * N * d * sizeof(float));
    g.gout = gout_dev; g.grad_a = grad_a_dev; g.grad_b = grad_b_dev;
    g.xm = xm; g.ym = ym; g.an = an; g.ia = ia; g.keys = keys; g.coef = coef; g.hist = hist; g.offs = offs; g.list = list; g.gt = gt;
    RUN("desc_loss_sparse_grad", launch_desc_loss_sparse_grad(g, s));
    return 0;
  });
}

}  // extern "C"
