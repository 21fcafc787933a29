/* imx_sptrain.h -- C ABI of libimx_sptrain.so, the companion of libimx.so (include/imx.h) for SuperPoint descriptor training.
 *
 * The two libraries are built together from one source tree (image-matching_amd/csrc/Makefile) and share the handle: every call
 * below takes an imx_handle_t that libimx.so's imx_create made, draws its scratch from that handle's workspace, reports errors
 * through imx_last_error and timing rows through imx_timing_report / imx_timing_form, and follows the conventions at the top of
 * imx.h (int return codes, caller-owned `*_dev` pointers, asynchronous on the caller's stream, nothing thrown across the ABI).
 * They live in a library of their own because libimx.so's symbol table is pinned to the 34 entry points of imx.h; use both
 * libraries from the SAME build (the handle's layout is internal to that build).
 */
#ifndef IMX_SPTRAIN_H
#define IMX_SPTRAIN_H

#include "imx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* SuperPoint descriptor training up to the forward VALUE of the objective (superpoint_train_descriptor.py -> datasets/ALLSS.py ->
 * superpoint/Train_model_heatmap.py:83-314); there is no backward pass.  Asynchronous, no host read.  No floating-point atomics: every
 * sum has a fixed order, so equal inputs give equal bits between calls, handles and workspace histories.
 *
 * imx_warp_labels: ALLSS.points_to_2D (datasets/ALLSS.py:129-133) and warpLabels (datasets/data_tools.py:36-54) for B images.
 * pts_dev (B,Kcap,2) float (x, y); counts_dev (B) int32 or NULL = Kcap (rows past the count are never read); mats_dev (B,3,3) fp32 in
 * PIXEL coordinates -- homography_scaling_torch(H) (utils/utils.py:586-589), formed by the caller.  The call zero-fills labels_dev
 * (B,H,W) and res_dev (B,2,H,W; may be NULL), then per point: truncation toward zero (.long()), warp_points in fp32 as
 * fma(m1, y, m0 x) + m2 over fma(m7, y, m6 x) + m8 (torch's CPU matrix product, k ascending), dropped unless 0 <= p <= size - 1 on the unrounded point, rounded
 * half to even; 1.0 goes to the label map and p - round(p) to res_dev[b][0] (x) and res_dev[b][1] (y).  Two points on one pixel: the
 * HIGHER point index writes the residual (a choice: the reference's indexed assignment defines none).  mats_dev NULL = points_to_2D:
 * truncation only, res_dev stays zero, and a point outside the image is written nowhere and sets bit 0 of *flag_dev (int32; the
 * call zeroes it first; may be NULL). */
IMX_API int imx_warp_labels(imx_handle_t h, const float* pts_dev, const int32_t* counts_dev, int B, int Kcap, const float* mats_dev,
                            int H, int W, float* labels_dev, float* res_dev, int32_t* flag_dev, void* stream);
/* The margin of compute_valid_mask (utils/utils.py:449-452): cv2.erode(mask, getStructuringElement(MORPH_ELLIPSE, (2r, 2r))), default
 * anchor (r, r), one iteration, on mask_dev (B,H,W) -> out_dev; radius 0 copies.  Row i of the 2r rows has dy = i - r,
 * dx = (int)rint(r sqrt((r^2 - dy^2) / r^2)) in double and ones in columns [max(r - dx, 0), min(r + dx + 1, 2r));
 * out(y, x) = min over the set (i, j) of in(y + i - r, x + j - r), pixels outside the image taking no part.  Parity with OpenCV
 * itself is unpinned; the kernel is held to tests/sptrain_ref.py.  radius <= 128; not in place for radius > 0. */
IMX_API int imx_erode_mask(imx_handle_t h, const float* mask_dev, float* out_dev, int B, int H, int W, int radius, void* stream);
/* labels2Dto3D + getMasks + detector_loss(loss_type="softmax") (utils/utils.py:456-468, Train_model_frontend.py:362-377,
 * Train_model_heatmap.py:72-81) in one pass: semi_dev (B,65,H/8,W/8), labels_dev and mask_dev (B,H,W) float (any values, 16-byte
 * aligned), out_dev[2] = {loss, sum of the cell masks}.  Per 8x8 cell: the 64 space-to-depth targets (c = dy 8 + dx),
 * dustbin = 1 - sum set to 0 where < 1, all 65 divided by their sum; cell mask = product of the 64 mask values;
 * sum_c -(t log p + (1 - t) log(1 - p)) with BCELoss's clamps at -100, times the cell mask; loss = total / (sum of masks + 1e-10).
 * -log p_c is min(100, lse - x_c) and 1 - p_c comes from the sum of the OTHER exponentials: the value follows the float64 evaluation
 * of the reference where its own fp32 forward leaves it (logit gaps beyond ~87).  H, W multiples of 8. */
IMX_API int imx_detector_loss(imx_handle_t h, const float* semi_dev, const float* labels_dev, const float* mask_dev, int B, int H, int W,
                              float* out_dev, void* stream);
/* descriptor_loss_sparse / batch_descriptor_loss_sparse (superpoint/loss_functions/sparse_loss.py:98-174, dist='cos') for B images,
 * indices in, losses out (the random draws stay with the caller).  desc_{a,b}_dev (B,d,Hc,Wc) as imx_superpoint_dense writes them;
 * hcell_dev (B,3,3) fp32: scale_homography_torch(H, (Hc,Wc), shift=(-1,-1)), formed by the caller.  Per image: every cell (x, y) in
 * row-major order through warp_points in fp32, round_() half to even, filter_points against (Wc, Hc); the surviving (a, b) flat
 * cell indices compacted in row-major order -- n_valid of them.  choice_dev (B,M) int32 indexes that list; nonmatch_b_dev (B,M,R)
 * int32 are flat cell indices of side b.  match = mean_m max(0, 1 - <a_m, b_m>): method 1 ('1d') at the integer cells, 2 ('2d') both
 * sides by bilinear grid_sample(align_corners=True) at normPts(p) (p / (Wc,Hc) 2 - 1), no renormalisation.
 * non_match = sum_{m,r} v / (count(v != 0) + 1), v = max(0, <a_m, desc_b[nonmatch[m][r]]> - margin), a_m the 1d descriptor always.
 *   out_dev (B,5) = {lamda_d match + non_match, lamda_d match, non_match, num_hard_negatives, n_valid}; mean_dev[3]: the batch means of
 *   the first three; pairs_dev (B,Hc Wc,2) int32 or NULL: the compacted list, -1 past n_valid.
 * n_valid = 0 gives NaN losses for that image (the reference raises inside np.random.choice there) and touches nothing else.  A
 * choice index >= n_valid > 0 sets bit 0 of *flag_dev, a non-match index outside the map bit 1 (the call zeroes the word first; may be
 * NULL); such an entry is not read through and contributes 0.  d a multiple of 4 up to 512. */
IMX_API int imx_desc_loss_sparse(imx_handle_t h, const float* desc_a_dev, const float* desc_b_dev, int B, int d, int Hc, int Wc,
                                 const float* hcell_dev, const int32_t* choice_dev, const int32_t* nonmatch_b_dev, int M, int R,
                                 float lamda_d, float margin, int method, float* out_dev, float* mean_dev, int32_t* pairs_dev,
                                 int32_t* flag_dev, void* stream);

/* The first stage of imx_desc_loss_sparse alone, for the caller's draws (crop_or_pad_choice needs n_valid, create_non_correspondences
 * the matched cells): pairs_dev (B,Hc Wc,2) int32, the compacted (a, b) flat cell indices with -1 past n_valid_dev[b] (B int32).  The
 * same kernel, so the list is the one imx_desc_loss_sparse indexes with choice_dev. */
IMX_API int imx_desc_pairs(imx_handle_t h, const float* hcell_dev, int B, int Hc, int Wc, int32_t* pairs_dev, int32_t* n_valid_dev,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IMX_SPTRAIN_H */
