// imx_homog.cpp -- the host unit of libimx_homog.so (include/imx_homog.h), on the handle libimx.so made: the argument checks of the
// RANSAC homography fit and of the corner error, and their launches (homog.hip).  Scratch: "homog.scratch" (16 B K0 bytes) only when
// K0 is above the LDS staging limit, written by the call before it is read.
#include "imx_host.h"
#include "homog.h"
#include "../../include/imx_homog.h"

extern "C" {

int imx_estimate_homography(imx_handle_t h, const float* kpts0_dev, const float* kpts1_dev, const int64_t* matches0_dev,
                            const int32_t* counts0_dev, int B, int K0, int K1, double threshold, int hypotheses, int refine_iters, uint32_t seed,
                            double* H_dev, uint8_t* inlier_dev, int32_t* n_inliers_dev, int32_t* best_h_dev, void* stream) {
  return on_device(h, "imx_estimate_homography", [&]() -> int {
    const char* who = "imx_estimate_homography";
    hipStream_t s = as_stream(stream);
    if (B < 1 || B > (1 << 20) || K0 < 1 || K1 < 1 || K0 > (1 << 20) || K1 > (1 << 20))
      return fail(h, "%s: bad shape B=%d K0=%d K1=%d (each in [1,2^20])", who, B, K0, K1);
    if (!(threshold > 0.0) || !(threshold < 1e300)) return fail(h, "%s: threshold must be positive and finite", who);
    if (hypotheses < 1 || hypotheses > (1 << 20)) return fail(h, "%s: hypotheses=%d outside [1,2^20]", who, hypotheses);
    if (refine_iters < 0 || refine_iters > 64) return fail(h, "%s: refine_iters=%d outside [0,64]", who, refine_iters);
    if (!kpts0_dev || !kpts1_dev || !matches0_dev || !H_dev || !inlier_dev || !n_inliers_dev || !best_h_dev) return fail(h, "%s: null argument", who);
    float* scratch = nullptr;
    if (K0 > kHomogLdsSlots) {      // the compacted coordinates no longer fit LDS: they live in HBM (slower; nothing is refused)
      WS(hs, float, "homog.scratch", (size_t)B * 4 * K0 * sizeof(float));
      scratch = hs;
    }
    HomogArgs a{};
    a.kpts0 = kpts0_dev; a.kpts1 = kpts1_dev; a.matches0 = reinterpret_cast<const long long*>(matches0_dev); a.counts0 = counts0_dev;
    a.B = B; a.K0 = K0; a.K1 = K1; a.threshold = threshold; a.hypotheses = hypotheses; a.refine_iters = refine_iters; a.seed = seed;
    a.H = H_dev; a.inlier = inlier_dev; a.n_inliers = n_inliers_dev; a.best_h = best_h_dev; a.scratch = scratch;
    RUN("homog_ransac", launch_homog_ransac(a, s));
    return 0;
  });
}

int imx_homography_corner_error(imx_handle_t h, const double* H_est_dev, const double* H_gt_dev, int B, int width, int height, double* err_dev,
                                void* stream) {
  return on_device(h, "imx_homography_corner_error", [&]() -> int {
    const char* who = "imx_homography_corner_error";
    hipStream_t s = as_stream(stream);
    if (B < 1 || B > (1 << 20) || width < 1 || height < 1) return fail(h, "%s: bad shape B=%d width=%d height=%d", who, B, width, height);
    if (!H_est_dev || !H_gt_dev || !err_dev) return fail(h, "%s: null argument", who);
    RUN("homog_corner_error", launch_homog_corner_error(H_est_dev, H_gt_dev, B, width, height, err_dev, s));
    return 0;
  });
}

}  // extern "C"
