/* imx_homog.h -- C ABI of libimx_homog.so, a companion of libimx.so (include/imx.h) and its eight other companions (imx_train.h,
 * imx_sgtrain.h, imx_spnet.h, imx_spnorm.h, imx_sppool.h, imx_photo.h, imx_sploop.h, imx_sgloop.h): the batched RANSAC homography fit
 * on matched keypoints -- the cv2.findHomography(mkpts0, mkpts1, cv2.RANSAC, thr) counterpart of imx_estimate_affine_partial -- and the
 * corner error of a fit against a known warp, the measure of the SuperPoint and SuperGlue papers for pairs related by a homography.
 *
 * The ten libraries are built together from one source tree (image-matching_amd/csrc/Makefile) and share the handle: every call
 * below takes an imx_handle_t that libimx.so's imx_create made, reports errors through imx_last_error and timing rows through
 * imx_timing_report, and follows the conventions at the top of imx.h (int return codes, caller-owned `*_dev` pointers, asynchronous
 * on the caller's stream, nothing thrown across the ABI).  They live in a library of their own because the symbol tables of the other
 * nine are pinned to their headers.  Use all libraries from the SAME build (the handle's layout is internal to that build).
 *
 * No call reads device memory on the host, reads the environment, uses a floating-point atomic, a cooperative launch or a workgroup
 * that waits on another.  A null required pointer or a shape outside the bounds returns an error code, sets imx_last_error and
 * launches nothing.
 */
#ifndef IMX_HOMOG_H
#define IMX_HOMOG_H

#include "imx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ====================================================================================================================
 * imx_estimate_homography: RANSAC homography of B pairs, one workgroup per pair, every operation after the load in float64
 * ====================================================================================================================
 *
 *   kpts0 (B,K0,2), kpts1 (B,K1,2) fp32      matches0 (B,K0) int64: index into kpts1; < 0 or >= K1 = unmatched
 *   counts0 (B) int32 or NULL = K0, clamped to [0,K0]: slots of kpts0 / matches0 past it are never read (they may hold NaN)
 *   H (B,9) float64, row-major, H[8] = 1, mapping kpts0 to kpts1       inlier (B,K0) uint8       n_inliers (B), best_h (B) int32
 *
 * Per pair, with n the number of matched slots taken in index order:
 *   1. n < 4: the FAILURE OUTPUT -- H all zeros, inlier all 0, n_inliers 0, best_h -1.
 *   2. Hartley normalisation of both point sets over all n points (centroid to 0, mean distance to sqrt 2); a mean distance that is
 *      0 or not finite: the failure output.
 *   3. Hypothesis h = 0 .. hypotheses-1 draws four distinct indices by an integer hash of (seed, h, n) -- not of the pair's position
 *      in the batch -- and is degenerate if, in either normalised set, twice the area of one of its four triples is below 1e-6 in
 *      magnitude, or if a corresponding triple changes orientation.  Otherwise the exact four-point map, scaled to h33 = 1 in
 *      normalised coordinates.  A matched point is an inlier of h if its projected w is positive (the centroid's side of the horizon)
 *      and its forward reprojection error e in destination pixels satisfies e^2 < threshold^2.
 *   4. The largest inlier count wins, the lowest h among equals; a winning count below 4: the failure output.
 *   5. Refit on the winner's inliers in normalised coordinates: the linear problem (8 unknowns, h33 = 1, two DLT rows per point) by
 *      normal equations, then refine_iters Gauss-Newton steps on the reprojection error, each solve(J^T J, -J^T r).  Every sum runs in
 *      a fixed order.  A singular system: the failure output.
 *   6. Back to pixels, divided by H[8]; |H[8]| < 1e-12 |H|_F: the failure output.
 *   7. inlier is the mask of the WINNING HYPOTHESIS in keypoint0 index space (not of the refit), n_inliers its count, best_h its h.
 *
 * Equal inputs give equal bits between calls, handles, batch compositions, positions in the batch, K0 padding past counts0 and
 * workspace histories.  The compacted coordinates are staged in LDS up to 8192 slots of K0, above that in the handle's workspace
 * ("homog.scratch", 16 B K0 bytes, written by the call before it is read).
 *
 * Bounds: 1 <= B <= 2^20, 1 <= K0, K1 <= 2^20, threshold > 0 and finite, 1 <= hypotheses <= 2^20, 0 <= refine_iters <= 64.
 */
IMX_API int imx_estimate_homography(imx_handle_t h, const float* kpts0_dev, const float* kpts1_dev, const int64_t* matches0_dev,
                                    const int32_t* counts0_dev, int B, int K0, int K1, double threshold, int hypotheses, int refine_iters,
                                    uint32_t seed, double* H_dev, uint8_t* inlier_dev, int32_t* n_inliers_dev, int32_t* best_h_dev,
                                    void* stream);

/* ====================================================================================================================
 * imx_homography_corner_error: the mean distance of the image corners under two homographies, B pairs
 * ====================================================================================================================
 *
 *   H_est (B,9), H_gt (B,9) float64, row-major          err (B) float64
 *
 * err[b] = the mean over the corners (0,0), (width-1,0), (width-1,height-1), (0,height-1) of the distance between the corner's
 * projections by H_est[b] and by H_gt[b], in float64.  +inf for an all-zero H_est (imx_estimate_homography's failure output) and
 * wherever the value is not finite (a corner on a horizon).
 *
 * Bounds: 1 <= B <= 2^20, width, height >= 1.
 */
IMX_API int imx_homography_corner_error(imx_handle_t h, const double* H_est_dev, const double* H_gt_dev, int B, int width, int height,
                                        double* err_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IMX_HOMOG_H */
