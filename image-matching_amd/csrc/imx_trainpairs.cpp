// imx_trainpairs.cpp -- SuperGlue training pairs (datasets/GlueSparse.py, superglue/models/superglue_train.py:289-299): the entry points
// imx_warp_perspective_u8, imx_gt_matches and imx_match_loss, and the record of the last SuperGlue forward the loss reads.
#include "imx_host.h"

namespace imx::host {

int sg_keep_counts(imx_handle_t h, int B, const int32_t* n0, const int32_t* n1, hipStream_t s) {
  auto& L = h->sg_last;
  L.valid = false;
  if (!L.S || L.B != B) return 0;                 // (a forward with an empty side leaves nothing: the loss will say so)
  const DevBuf& own = h->bufs["mp.counts"];
  const int32_t* keep[2] = {n0, n1};
  if ((n0 && !inside(n0, own)) || (n1 && !inside(n1, own))) {
    WS(cp, int32_t, "sg.loss_counts", (size_t)2 * B * 4);
    for (int k = 0; k < 2; ++k)
      if (keep[k] && !inside(keep[k], own)) {
        HIP_OK(h, hipMemcpyAsync(cp + (size_t)k * B, keep[k], (size_t)B * 4, hipMemcpyDeviceToDevice, s));
        keep[k] = cp + (size_t)k * B;
      }
  }
  L.n0 = keep[0];
  L.n1 = keep[1];
  L.valid = true;
  return 0;
}

}  // namespace imx::host

extern "C" {

int imx_warp_perspective_u8(imx_handle_t h, const uint8_t* src_dev, int64_t src_stride_b, const double* minv_dev, uint8_t* dst_dev,
                            int B, int H, int W, void* stream) {
  return on_device(h, "imx_warp_perspective_u8", [&]() -> int {
    if (B < 1 || B > 65535 || H < 1 || W < 1) return fail(h, "imx_warp_perspective_u8: bad shape B=%d H=%d W=%d (B in [1,65535])", B, H, W);
    if (!src_dev || !minv_dev || !dst_dev) return fail(h, "imx_warp_perspective_u8: null argument");
    if (src_stride_b < (int64_t)H * W && B > 1) return fail(h, "imx_warp_perspective_u8: batch stride %lld below one image", (long long)src_stride_b);
    hipStream_t s = as_stream(stream);
    RUN("warp_perspective", launch_warp_perspective_u8(src_dev, (long)src_stride_b, minv_dev, dst_dev, B, H, W, s));
    return 0;
  });
}

int imx_gt_matches(imx_handle_t h, int B, const float* kpts0_dev, const int32_t* n0_dev, int N0, const float* kpts1_dev,
                   const int32_t* n1_dev, int N1, const double* m_dev, double radius, float* proj_dev, int64_t* gt0_dev,
                   int64_t* gt1_dev, int64_t* all_matches_dev, int32_t* n_matches_dev, int32_t* n_all_dev, void* stream) {
  return on_device(h, "imx_gt_matches", [&]() -> int {
    if (B < 1 || B > 65535 || N0 < 0 || N1 < 0 || (int64_t)N0 + N1 > (1 << 30)) return fail(h, "imx_gt_matches: bad shape B=%d N0=%d N1=%d (B in [1,65535])", B, N0, N1);
    if (!m_dev || !n_matches_dev || !n_all_dev || (N0 && (!kpts0_dev || !gt0_dev)) || (N1 && (!kpts1_dev || !gt1_dev)) || (N0 + N1 && !all_matches_dev))
      return fail(h, "imx_gt_matches: null argument");
    hipStream_t s = as_stream(stream);
    const size_t r0 = (size_t)B * std::max(N0, 1), r1 = (size_t)B * std::max(N1, 1);
    WS(proj, float, "gt.proj", r0 * 2 * sizeof(float));
    WS(nn0, int, "gt.nn0", r0 * sizeof(int));
    WS(nn1, int, "gt.nn1", r1 * sizeof(int));
    WS(d0, double, "gt.d0", r0 * sizeof(double));
    GtArgs a{};
    a.kpts0 = kpts0_dev; a.kpts1 = kpts1_dev; a.n0 = n0_dev; a.n1 = n1_dev; a.m = m_dev; a.radius = radius;
    a.B = B; a.N0 = N0; a.N1 = N1; a.proj = proj; a.proj_out = proj_dev; a.nn0 = nn0; a.nn1 = nn1; a.d0 = d0;
    a.gt0 = reinterpret_cast<long long*>(gt0_dev); a.gt1 = reinterpret_cast<long long*>(gt1_dev);
    a.all_matches = reinterpret_cast<long long*>(all_matches_dev); a.n_matches = n_matches_dev; a.n_all = n_all_dev;
    RUN("gt_matches", launch_gt_matches(a, s));
    return 0;
  });
}

int imx_match_loss(imx_handle_t h, int B, const int64_t* all_matches_dev, const int32_t* n_all_dev, int L, const int64_t* matches0_dev,
                   const int64_t* gt0_dev, float* loss_dev, int32_t* stats_dev, void* stream) {
  return on_device(h, "imx_match_loss", [&]() -> int {
    const auto& p = h->sg_last;
    if (!p.valid)
      return fail(h, "imx_match_loss: no SuperGlue forward to read on this handle (none has run, it had an empty side, or its workspaces "
                     "were grown, released or overwritten since): run imx_superglue_forward or imx_match_pairs first");
    if (B != p.B || L != p.N0 + p.N1)
      return fail(h, "imx_match_loss: B=%d L=%d do not belong to the last SuperGlue forward (B=%d, N0=%d, N1=%d: L must be N0 + N1)", B, L, p.B, p.N0, p.N1);
    if (!all_matches_dev || !n_all_dev || !loss_dev) return fail(h, "imx_match_loss: null argument");
    hipStream_t s = as_stream(stream);
    LossArgs a{};
    a.S = p.S; a.u = p.u; a.v = p.v; a.n0 = p.n0; a.n1 = p.n1; a.B = B; a.N0 = p.N0; a.N1 = p.N1; a.N0p = p.N0p; a.N1p = p.N1p;
    a.alpha = p.alpha;
    a.all_matches = reinterpret_cast<const long long*>(all_matches_dev); a.n_all = n_all_dev; a.L = L;
    a.matches0 = reinterpret_cast<const long long*>(matches0_dev); a.gt0 = reinterpret_cast<const long long*>(gt0_dev);
    a.loss = loss_dev; a.stats = matches0_dev && gt0_dev ? stats_dev : nullptr;
    RUN("match_loss", launch_match_loss(a, s));
    return 0;
  });
}

}  // extern "C"
