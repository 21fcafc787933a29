// homog.h -- launchers of homog.hip, kernels of libimx_homog.so (include/imx_homog.h): the batched RANSAC homography fit on matched
// keypoints (the cv2.findHomography(..., RANSAC) counterpart of registration.hip's similarity fit) and the corner error of a fit against
// a known warp.  DESIGN.md section 24 has the hash, the degeneracy rule, the launch structure and the resource usage.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace imx {

constexpr int kHomogLdsSlots = 8192;        // matched pairs whose coordinates are staged in LDS (4 floats each: 128 KB); above, in `scratch`

struct HomogArgs {
  const float* kpts0; const float* kpts1;   // (B,K0,2), (B,K1,2)
  const long long* matches0;                // (B,K0): index into kpts1, < 0 or >= K1 = unmatched
  const int* counts0;                       // (B) or null = K0; slots past it are never read
  int B, K0, K1;
  double threshold;                         // pixels, in the destination image
  int hypotheses, refine_iters;
  unsigned seed;
  double* H;                                // (B,9), H[8] = 1; all zeros = no fit
  unsigned char* inlier;                    // (B,K0): the winning hypothesis' mask in keypoint0 index space
  int* n_inliers; int* best_h;              // (B); best_h = -1 = no fit
  float* scratch;                           // (B,4,K0) floats when K0 > kHomogLdsSlots, else unused
};

hipError_t launch_homog_ransac(const HomogArgs& a, hipStream_t s);
// err[b] = mean over the corners (0,0), (W-1,0), (W-1,H-1), (0,H-1) of |proj(H_est, c) - proj(H_gt, c)|; +inf for an all-zero H_est
hipError_t launch_homog_corner_error(const double* H_est, const double* H_gt, int B, int width, int height, double* err, hipStream_t s);

}  // namespace imx
