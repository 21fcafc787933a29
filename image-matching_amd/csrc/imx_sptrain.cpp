// imx_sptrain.cpp -- a host unit of libimx_train.so (include/imx_train.h), on the handle libimx.so made: SuperPoint descriptor training up to the forward value of the objective (superpoint_train_descriptor.py ->
// datasets/ALLSS.py -> superpoint/Train_model_heatmap.py:83-314): the entry points imx_warp_labels, imx_erode_mask,
// imx_detector_loss, imx_desc_pairs and imx_desc_loss_sparse.  Every scratch buffer ("spt.*") is written in full by the call that reads it.
#include "imx_host.h"
#include "../../include/imx_train.h"

namespace {
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
}  // namespace

extern "C" {

int imx_warp_labels(imx_handle_t h, const float* pts_dev, const int32_t* counts_dev, int B, int Kcap, const float* mats_dev, int H, int W,
                    float* labels_dev, float* res_dev, int32_t* flag_dev, void* stream) {
  return on_device(h, "imx_warp_labels", [&]() -> int {
    if (B < 1 || B > 65535 || Kcap < 0 || H < 1 || W < 1 || (int64_t)B * H * W > (1ll << 31))
      return fail(h, "imx_warp_labels: bad shape B=%d Kcap=%d H=%d W=%d (B in [1,65535], B H W <= 2^31)", B, Kcap, H, W);
    if (!labels_dev || (Kcap && !pts_dev)) return fail(h, "imx_warp_labels: null argument");
    hipStream_t s = as_stream(stream);
    WarpLabelsArgs a{};
    a.pts = pts_dev; a.counts = counts_dev; a.mats = mats_dev; a.B = B; a.Kcap = Kcap; a.H = H; a.W = W;
    a.labels = labels_dev; a.res = res_dev; a.flag = flag_dev;
    if (res_dev && mats_dev) {
      WS(owner, int, "spt.owner", (size_t)B * H * W * sizeof(int));
      a.owner = owner;
    }
    RUN("warp_labels", launch_warp_labels(a, s));
    return 0;
  });
}

int imx_erode_mask(imx_handle_t h, const float* mask_dev, float* out_dev, int B, int H, int W, int radius, void* stream) {
  return on_device(h, "imx_erode_mask", [&]() -> int {
    if (B < 1 || B > 65535 || H < 1 || W < 1 || (H + 3) / 4 > 65535) return fail(h, "imx_erode_mask: bad shape B=%d H=%d W=%d (B in [1,65535])", B, H, W);
    if (radius < 0 || radius > kErodeMaxRadius) return fail(h, "imx_erode_mask: radius %d outside [0,%d]", radius, kErodeMaxRadius);
    if (!mask_dev || !out_dev) return fail(h, "imx_erode_mask: null argument");
    hipStream_t s = as_stream(stream);
    if (radius == 0) {
      if (out_dev != mask_dev) HIP_OK(h, hipMemcpyAsync(out_dev, mask_dev, (size_t)B * H * W * sizeof(float), hipMemcpyDeviceToDevice, s));
      return 0;
    }
    if (out_dev == mask_dev) return fail(h, "imx_erode_mask: radius > 0 cannot run in place");
    RUN("erode_mask", launch_erode_mask(mask_dev, out_dev, B, H, W, radius, s));
    return 0;
  });
}

int imx_detector_loss(imx_handle_t h, const float* semi_dev, const float* labels_dev, const float* mask_dev, int B, int H, int W,
                      float* out_dev, void* stream) {
  return on_device(h, "imx_detector_loss", [&]() -> int {
    if (B < 1 || H < 8 || W < 8 || H % 8 || W % 8 || (int64_t)B * (H / 8) * (W / 8) > (1 << 30))
      return fail(h, "imx_detector_loss: bad shape B=%d H=%d W=%d (H, W multiples of 8)", B, H, W);
    if (!semi_dev || !labels_dev || !mask_dev || !out_dev) return fail(h, "imx_detector_loss: null argument");
    if (!aligned16(labels_dev) || !aligned16(mask_dev)) return fail(h, "imx_detector_loss: labels_dev and mask_dev must be 16-byte aligned");
    hipStream_t s = as_stream(stream);
    const int Hc = H / 8, Wc = W / 8;
    WS(part, double, "spt.det_part", (size_t)2 * detector_loss_blocks(B, Hc, Wc) * sizeof(double));
    RUN("detector_loss", launch_detector_loss(semi_dev, labels_dev, mask_dev, B, Hc, Wc, part, out_dev, s));
    return 0;
  });
}

int imx_desc_pairs(imx_handle_t h, const float* hcell_dev, int B, int Hc, int Wc, int32_t* pairs_dev, int32_t* n_valid_dev, void* stream) {
  return on_device(h, "imx_desc_pairs", [&]() -> int {
    if (B < 1 || B > 65535 || Hc < 1 || Wc < 1 || (int64_t)Hc * Wc > (1 << 24)) return fail(h, "imx_desc_pairs: bad shape B=%d Hc=%d Wc=%d", B, Hc, Wc);
    if (!hcell_dev || !pairs_dev || !n_valid_dev) return fail(h, "imx_desc_pairs: null argument");
    hipStream_t s = as_stream(stream);
    DescLossArgs a{};
    a.hcell = hcell_dev; a.B = B; a.Hc = Hc; a.Wc = Wc; a.pairs = pairs_dev; a.nvalid = n_valid_dev;
    RUN("desc_pairs", launch_desc_pairs(a, s));
    return 0;
  });
}

int imx_desc_loss_sparse(imx_handle_t h, const float* desc_a_dev, const float* desc_b_dev, int B, int d, int Hc, int Wc,
                         const float* hcell_dev, const int32_t* choice_dev, const int32_t* nonmatch_b_dev, int M, int R, float lamda_d,
                         float margin, int method, float* out_dev, float* mean_dev, int32_t* pairs_dev, int32_t* flag_dev, void* stream) {
  return on_device(h, "imx_desc_loss_sparse", [&]() -> int {
    if (B < 1 || B > 32767 || Hc < 1 || Wc < 1 || (int64_t)Hc * Wc > (1 << 24) || M < 1 || R < 1 || (int64_t)B * M * R > (1ll << 31))
      return fail(h, "imx_desc_loss_sparse: bad shape B=%d Hc=%d Wc=%d M=%d R=%d (B in [1,32767], Hc Wc <= 2^24, B M R <= 2^31)", B, Hc, Wc, M, R);
    if (d < 4 || d % 4 || d > 512) return fail(h, "imx_desc_loss_sparse: descriptor dimension %d must be a multiple of 4 in [4,512]", d);
    if (method != 1 && method != 2) return fail(h, "imx_desc_loss_sparse: method must be 1 ('1d') or 2 ('2d'), got %d", method);
    if (!desc_a_dev || !desc_b_dev || !hcell_dev || !choice_dev || !nonmatch_b_dev || !out_dev || !mean_dev)
      return fail(h, "imx_desc_loss_sparse: null argument");
    hipStream_t s = as_stream(stream);
    const size_t N = (size_t)Hc * Wc;
    WS(ta, float, "spt.desc_a_t", (size_t)B * N * d * sizeof(float));
    WS(tb, float, "spt.desc_b_t", (size_t)B * N * d * sizeof(float));
    WS(pairs, int, "spt.pairs", (size_t)B * N * 2 * sizeof(int));
    WS(nvalid, int, "spt.nvalid", (size_t)B * sizeof(int));
    WS(partial, float, "spt.partial", (size_t)B * M * 3 * sizeof(float));
    DescLossArgs a{};
    a.desc_a = desc_a_dev; a.desc_b = desc_b_dev; a.hcell = hcell_dev; a.choice = choice_dev; a.nonmatch = nonmatch_b_dev;
    a.B = B; a.d = d; a.Hc = Hc; a.Wc = Wc; a.M = M; a.R = R; a.lamda_d = lamda_d; a.margin = margin; a.method2d = method == 2;
    a.ta = ta; a.tb = tb; a.pairs = pairs; a.nvalid = nvalid; a.partial = partial;
    a.out = out_dev; a.mean = mean_dev; a.pairs_out = pairs_dev; a.flag = flag_dev;
    RUN("desc_loss_sparse", launch_desc_loss_sparse(a, s));
    return 0;
  });
}

}  // extern "C"
