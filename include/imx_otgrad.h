/* imx_otgrad.h -- C ABI of libimx_otgrad.so, the fourth library on libimx.so's handles (include/imx.h; beside imx_sptrain.h and
 * imx_spgrad.h): the SuperGlue training objective as a value-and-gradient call at the score matrix,
 *
 *   scores -> log_optimal_transport(scores, bin_score, iters) -> mean over all_matches of -log(exp(Z[x][y]))
 *                                                                   (superglue/models/superglue_train.py:134-167 and :267-299)
 *
 * differentiated through the unrolled Sinkhorn loop, as the reference's autograd does (no implicit differentiation at the fixed
 * point).  Built with the other three from one source tree (image-matching_amd/csrc/Makefile); use all from the SAME build.  The call
 * takes an imx_handle_t that libimx.so's imx_create made, draws its scratch from that handle's workspace (names "otg.*":
 * O(B iters (N0 + N1)) floats -- the potentials of every iteration and their cotangents -- plus a few vectors; nothing of matrix
 * size), reports errors through imx_last_error and timing rows through imx_timing_report, and follows the conventions at the top of
 * imx.h.  A library of its own because the symbol tables of the other three are pinned.
 *
 * Asynchronous on the caller's stream, no host read.  No floating-point atomics and no workgroup that waits on another: one plain
 * launch per half-iteration, every sum in a fixed order, so equal inputs give equal bits between calls, handles, batch compositions
 * and workspace histories.  The backward of the einsum and of the network's layers is not here: the caller's framework runs it from
 * grad_scores_dev and grad_bin_dev.
 */
#ifndef IMX_OTGRAD_H
#define IMX_OTGRAD_H

#include "imx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per pair b, with m = n0_dev[b], n = n1_dev[b] (NULL = N0 / N1; clamped to [0,N0] / [0,N1]) and C the (m+1) x (n+1) coupling matrix
 * (scores_dev[b] inside, *bin_score_dev in the last row and column):
 *   u_0 = v_0 = 0;  u_t = log_mu - LSE_j(C + v_{t-1}),  v_t = log_nu - LSE_i(C + u_t)  (t = 1..iters);  Z = C + u_T + v_T - norm
 *   loss_dev[b] = (1 / K) sum over the K = n_all_dev[b] listed (x, y) of -logf(expf(Z[x][y]))      (+inf where the exp underflows)
 *   grad_scores_dev[b] = gout d loss / d scores (B,N0,N1), written in full: 0 on rows past m and columns past n
 *   grad_bin_dev[b]    = gout d loss / d bin_score: the cotangent of C summed over its last row and column
 * all_matches_dev (B,2,L) int64: row 0 the x, row 1 the y of the listings, as imx_gt_matches writes them; x = m / y = n is the dustbin.
 * A listing counts once per appearance; entries past n_all_dev[b] (clamped to [0,L]) are not read; K = 0, m = 0 or n = 0 gives loss 0
 * and zero gradients.  A listed index outside [0,m] x [0,n] sets bit 0 of flag_dev[b] (may be NULL) and contributes nothing (K
 * still counts it).  Rows past m and columns past n of scores_dev are never read.
 * Where a listed entry's exp underflows the value is +inf and the derivative returned is that of -Z[x][y]: finite, the limit of the
 * written form (torch's autograd gives NaN there).
 * gout_dev: B floats on the device, one upstream cotangent per pair; NULL means 1.  grad_scores_dev = NULL: the value only (loss_dev
 * and flag_dev; grad_bin_dev is not written).  0 <= iters <= 4096, 1 <= N0, N1 <= 2^20, 1 <= B <= 65535, 0 <= L. */
IMX_API int imx_ot_match_loss_grad(imx_handle_t h, int B, const float* scores_dev, int N0, int N1, const int32_t* n0_dev,
                                   const int32_t* n1_dev, const float* bin_score_dev, int iters, const int64_t* all_matches_dev,
                                   const int32_t* n_all_dev, int L, const float* gout_dev, float* loss_dev, float* grad_scores_dev,
                                   float* grad_bin_dev, int32_t* flag_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IMX_OTGRAD_H */
