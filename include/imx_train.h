/* imx_train.h -- C ABI of libimx_train.so, the companion of libimx.so (include/imx.h) for training: the SuperPoint descriptor-training
 * stages and the gradients of their losses, the SuperGlue match loss through the unrolled Sinkhorn, and the attention, 1x1 convolutions
 * and BatchNorm + ReLU of SuperGlue's GNN in their training form.  One section per stage below.
 *
 * The two libraries are built together from one source tree (image-matching_amd/csrc/Makefile) and share the handle: every call
 * below takes an imx_handle_t that libimx.so's imx_create made, draws its scratch from that handle's workspace, reports errors
 * through imx_last_error and timing rows through imx_timing_report / imx_timing_form, and follows the conventions at the top of
 * imx.h (int return codes, caller-owned `*_dev` pointers, asynchronous on the caller's stream, nothing thrown across the ABI).
 * They live in a library of their own because libimx.so's symbol table is pinned to the 34 entry points of imx.h; use both
 * libraries from the SAME build (the handle's layout is internal to that build).
 */
#ifndef IMX_TRAIN_H
#define IMX_TRAIN_H

#include "imx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ====================================================================================================================
 * SuperPoint descriptor training: labels, masks and the forward values of the two losses
 * ==================================================================================================================== */

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

/* ====================================================================================================================
 * the gradients of the two SuperPoint training losses
 * ==================================================================================================================== */

/* The gradients of the SuperPoint training objective with respect to what the network emits:
 *
 *   loss = loss_det + loss_det_warp + lambda_loss loss_desc        (superpoint/Train_model_heatmap.py:180-199)
 *
 * Scratch comes from the handle's workspace under the names "spg.*".
 *
 * Both calls are value-and-gradient: they write what the forward entry of the section above writes for the same inputs, bit for bit (the
 * same device code computes it), and the derivative of THAT value.  Asynchronous on the caller's stream, no host read, no
 * floating-point atomics: every sum has a fixed order, so equal inputs give equal bits between calls, handles and workspace
 * histories.  gout_dev: one float on the device, the upstream cotangent; NULL means 1.  The backward of the network's own layers is
 * not here: the caller's framework runs it from these cotangents.
 */

/* imx_detector_loss plus grad_semi_dev (B,65,H/8,W/8) = gout d out_dev[0] / d semi, written in full.  out_dev[2] as imx_detector_loss.
 * The gradient is the derivative of the conditioned form the library evaluates (imx_detector_loss).  Per cell, with softmax p, targets t,
 * cell mask m and D = (sum of cell masks) + 1e-10:
 *     dL/dx_k = (m / D) (q_k - p_k sum_c q_c),     q_c = -t_c + (1 - t_c) p_c / (1 - p_c),
 * p_c / (1 - p_c) formed as e_c / (sum of the OTHER exponentials), never through 1 - p; at the largest logit the products that carry
 * that ratio are multiplied out first (ratio (1 - p) = p), so nothing overflows.  A term whose min(100, .) clamp is active in the value
 * is a constant and contributes nothing.  Where no probability rounds to 1 or underflows (logit gaps below about 36 in float64) this
 * is the derivative of the reference's written form BCELoss(softmax(x)).  Beyond that range torch's own BCE backward ignores the clamp
 * and divides by max(p (1 - p), 1e-12); the two differ by O(1) at logit scale 30, and the library follows its own value.
 * D is read from out_dev[1] (a float; exact for 0/1 masks up to 2^24 cells). */
IMX_API int imx_detector_loss_grad(imx_handle_t h, const float* semi_dev, const float* labels_dev, const float* mask_dev, int B, int H,
                                   int W, const float* gout_dev, float* out_dev, float* grad_semi_dev, void* stream);

/* imx_desc_loss_sparse plus grad_a_dev and grad_b_dev (B,d,Hc,Wc), channel-major like the inputs, written in full:
 * gout d mean_dev[0] / d desc_{a,b}.  out_dev, mean_dev, pairs_dev and flag_dev as imx_desc_loss_sparse writes them.  Per image, with
 * w_m = gout lamda_d / (M B) and w_n = gout / ((num_hard_negatives + 1) B) (the count is a constant of the derivative):
 *   match m, where 1 - <a_m, b_m> >= 0 (inclusive: clamp(min=0) passes the gradient at 0): -w_m b_m at a's position, -w_m a_m at b's;
 *     method 2 spreads both over the four bilinear taps with the forward's weights, taps outside the map dropped;
 *   non-match (m, r), where <a_m, nb_r> - margin > 0 (strict): w_n nb_r at a's cell of match m, w_n a_m at cell nonmatch[m][r] of b,
 *     a_m the 1d descriptor always.
 * An image with n_valid = 0 gets zero gradients and sets bit 2 of *flag_dev (its forward values stay NaN); flagged choice or
 * non-match entries contribute nothing.  Sums into one cell run in ascending (m, slot) order -- a's slots of a match: its match taps
 * (nw, ne, sw, se), then the sum over r of its active non-match rows (formed per match in a fixed order); b's: its match taps, then
 * r ascending -- one fused multiply-add per entry and channel.  d a multiple of 4 up to 512; M (R + 9) <= 2^30. */
IMX_API int imx_desc_loss_sparse_grad(imx_handle_t h, const float* desc_a_dev, const float* desc_b_dev, int B, int d, int Hc, int Wc,
                                      const float* hcell_dev, const int32_t* choice_dev, const int32_t* nonmatch_b_dev, int M, int R,
                                      float lamda_d, float margin, int method, const float* gout_dev, float* out_dev, float* mean_dev,
                                      int32_t* pairs_dev, int32_t* flag_dev, float* grad_a_dev, float* grad_b_dev, void* stream);

/* ====================================================================================================================
 * the SuperGlue match loss through the unrolled Sinkhorn, value and gradient
 * ==================================================================================================================== */

/* The SuperGlue training objective as a value-and-gradient call at the score matrix,
 *
 *   scores -> log_optimal_transport(scores, bin_score, iters) -> mean over all_matches of -log(exp(Z[x][y]))
 *                                                                   (superglue/models/superglue_train.py:134-167 and :267-299)
 *
 * differentiated through the unrolled Sinkhorn loop, as the reference's autograd does (no implicit differentiation at the fixed
 * point).  The call draws its scratch from the handle's workspace (names "otg.*": O(B iters (N0 + N1)) floats -- the potentials of
 * every iteration and their cotangents -- plus a few vectors; nothing of matrix size).
 *
 * Asynchronous on the caller's stream, no host read.  No floating-point atomics and no workgroup that waits on another: one plain
 * launch per half-iteration, every sum in a fixed order, so equal inputs give equal bits between calls, handles, batch compositions
 * and workspace histories.  The backward of the einsum and of the network's layers is not here: the caller's framework runs it from
 * grad_scores_dev and grad_bin_dev.
 */

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

/* ====================================================================================================================
 * the attention of SuperGlue's GNN, training form
 * ==================================================================================================================== */

/* The attention of SuperGlue's GNN (superglue/models/superglue_train.py:82-86: einsum, softmax, einsum)
 * in its training form -- a forward that keeps the row log-sum-exp instead of the probabilities, and the backward that recomputes them.
 * Per (pair b, head h), with D the head dimension and scale = 1 / sqrt(D) (the reference's dim ** .5, dim = query.shape[1]):
 *
 *   forward    S = scale Q^T K (n_q x n_k),  P = softmax_rows(S),  O = P V,  lse_i = log sum_j exp(S_ij)
 *   backward   delta_i = sum_c dO_ic O_ic,  P = exp(S - lse) (recomputed, never stored),
 *              dV = P^T dO,  dP = dO V^T,  dS = P o (dP - delta) scale,  dQ = dS K,  dK = dS^T Q
 *
 * Layout: the reference's own tensors, read and written in place: (B, D, H, n) contiguous fp32, element (b, c, h, n) at
 * ((b D + c) H + h) n_frame + n, which is what conv1d(...).view(B, dim, heads, -1) yields (no copy, no permute); q, out, dout and dq
 * over a frame of N queries, k, v, dk and dv over a frame of M keys.  lse is (B, H, N).  No alignment beyond 4 bytes is assumed.
 *
 * Ragged batches: n_q = nq_dev[b], n_k = nk_dev[b] are read on the device (NULL = N / M; clamped to [0,N] / [0,M]).  Queries past n_q and
 * keys past n_k are never read and may hold anything, NaN included.  out, lse, dq, dk and dv are written in full, with 0 there; n_q = 0 or
 * n_k = 0 gives zeros everywhere for that pair.
 *
 * Arithmetic: every product on the fp32 matrix pipe (v_mfma_f32_32x32x2_f32), fp32 accumulation; a tile's 32 terms accumulate from
 * zero and are then added to the running sum (two levels).  No floating-point atomics, no workgroup that waits on another, no
 * cooperative launch: the order of every sum is fixed at compile time and depends on the pair's own counts only, so equal inputs give
 * equal bits between calls, handles, batch compositions, paddings and workspace histories.
 *
 * The calls draw their scratch from the handle's workspace ("mha.delta": B H N floats, written by the backward call that reads it;
 * nothing of size N M).  Asynchronous on the caller's stream, no host read.
 *
 * Not here: the q / k / v projections, the merge, the MLP and their backward (the caller's framework runs them), dropout, masks other
 * than the counts, the 16-bit plane forms of the inference path, a second derivative.
 */

/* q (B,D,H,N), k and v (B,D,H,M) -> out (B,D,H,N), lse (B,H,N).  lse_dev may be NULL (value only).
 * 1 <= B H <= 65535, 1 <= N, M <= 2^20, D in {16, 32, 64}: anything else, or a null q / k / v / out, returns an error code, sets
 * imx_last_error and launches nothing. */
IMX_API int imx_mha_forward_train(imx_handle_t h, int B, int H, int D, int N, int M,
                                  const float* q_dev, const float* k_dev, const float* v_dev,
                                  const int32_t* nq_dev, const int32_t* nk_dev,
                                  float* out_dev, float* lse_dev, void* stream);

/* the same q, k, v, the forward's out and lse, dout (B,D,H,N) -> dq (B,D,H,N), dk, dv (B,D,H,M).
 * Any of dq_dev / dk_dev / dv_dev may be NULL: that gradient is not formed (dq NULL skips the per-query kernel, dk and dv both NULL the
 * per-key kernel); the others keep their bits.  The same bounds and error rules; q, k, v, out, lse and dout are required. */
IMX_API int imx_mha_backward(imx_handle_t h, int B, int H, int D, int N, int M,
                             const float* q_dev, const float* k_dev, const float* v_dev,
                             const float* out_dev, const float* lse_dev, const float* dout_dev,
                             const int32_t* nq_dev, const int32_t* nk_dev,
                             float* dq_dev, float* dk_dev, float* dv_dev, void* stream);

/* ====================================================================================================================
 * the 1x1 convolutions of SuperGlue, training form
 * ==================================================================================================================== */

/* nn.Conv1d(kernel_size=1) of SuperGlue's GNN, keypoint encoder and final projection
 * (superglue/models/superglue_train.py:52, 96, 97, 111) in its training form -- the forward on torch.cat([x0, x1], 1) without forming the
 * concatenation, and the gradients at both inputs, the weight and the bias.  With xcat the concatenation over channels, Cin = C0 + C1:
 *
 *   forward    y[b,o,n]  = bias[o] + sum_c w[o,c] xcat[b,c,n]
 *   backward   dx[b,c,n] = sum_o w[o,c] dy[b,o,n]   (dx0 = channels [0, C0), dx1 = channels [C0, Cin))
 *              dw[o,c]   = sum_b sum_n dy[b,o,n] xcat[b,c,n],   db[o] = sum_b sum_n dy[b,o,n]
 *
 * Layout: the reference's own tensors, read and written in place: x0 (B,C0,N), x1 (B,C1,N), y and dy (B,Cout,N), contiguous fp32 over a
 * frame of N columns; w (Cout, Cin) row-major, the bytes of conv.weight (Cout, Cin, 1); bias and db (Cout); dw the shape of w.  dw and db
 * are overwritten, not accumulated.  No alignment beyond 4 bytes is assumed.  Outputs must not alias inputs.
 *
 * Ragged batches: n_dev[b] is read on the device (NULL = N; clamped to [0, N]).  Columns past the count are never read in x0, x1 and
 * dy and may hold anything, NaN included; y, dx0 and dx1 are written in full, with 0 there; such columns add nothing to dw and db, and a
 * pair of count 0 adds nothing at all.
 *
 * Arithmetic: every product on the fp32 matrix pipe (v_mfma_f32_32x32x2_f32), fp32 accumulation in two levels: the summation index is
 * cut into blocks of 128, a block accumulates as one MFMA chain from a zero accumulator and is then added to the running sum, blocks
 * ascending.  y: the concatenated input channel 0 .. Cin-1, then the bias (a block may straddle x0 and x1: any split of the same
 * channels gives the same bits).  dx: the output channel.  dw, db: the columns of a pair in slabs of 256 (two blocks each), each slab
 * from zero; a pair's slabs ascending into the pair's sum, then the pairs ascending; blocks and slabs past a pair's count and pairs of
 * count 0 are skipped, not added as zeros.  No floating-point atomics, no workgroup that waits on another, no cooperative launch: the
 * order of every sum is fixed at compile time and depends on the counts only, so equal inputs give equal bits between calls, handles,
 * frames, and workspace histories.  bias_dev = NULL gives the bits of a zero bias (the running sum is never -0).
 *
 * Scratch, from the handle's workspace: "lin.part",
 *     B * ceil(N / 256) * Cout * (C0 + C1 + 1) floats
 * (one partial dw and db per pair and slab), drawn by a backward call that forms dw or db; every element that call reads it has written
 * before.  At B = 8, Cout = Cin = 512, N = 2048 that is 8 * 8 * 512 * 513 * 4 bytes = 64.1 MiB, beside 32 MiB each of xcat, dy and dx.
 * Asynchronous on the caller's stream, no host read.
 *
 * Not here: BatchNorm, ReLU, the score einsum, the optimiser step (the caller's framework runs them), kernel sizes other than 1, groups,
 * the 16-bit plane forms of the inference path, a second derivative.
 */

/* x0 (B,C0,N), x1 (B,C1,N), w (Cout,C0+C1), bias (Cout) -> y (B,Cout,N).  bias_dev may be NULL; x1_dev is NULL exactly when C1 = 0.
 * 1 <= B <= 65535, 1 <= Cout <= 1024, C0 >= 1, C1 >= 0, C0 + C1 <= 1024, 1 <= N <= 2^20: anything else, or a null x0 / w / y, returns an
 * error code, sets imx_last_error and launches nothing. */
IMX_API int imx_conv1x1_forward_train(imx_handle_t h, int B, int Cout, int C0, int C1, int N,
                                      const float* x0_dev, const float* x1_dev, const float* w_dev, const float* bias_dev,
                                      const int32_t* n_dev, float* y_dev, void* stream);

/* the same x0, x1, w and dy (B,Cout,N) -> dx0 (B,C0,N), dx1 (B,C1,N), dw (Cout,C0+C1), db (Cout).
 * Any of dx0_dev / dx1_dev / dw_dev / db_dev may be NULL: that gradient is not formed (dx0 and dx1 both NULL skips the input-gradient
 * kernel, dw and db both NULL the weight-gradient kernels); the others keep their bits.  The same bounds and error rules; x0, w and dy
 * are required, and dx1_dev with C1 = 0 is an error. */
IMX_API int imx_conv1x1_backward(imx_handle_t h, int B, int Cout, int C0, int C1, int N,
                                 const float* x0_dev, const float* x1_dev, const float* w_dev, const float* dy_dev,
                                 const int32_t* n_dev, float* dx0_dev, float* dx1_dev, float* dw_dev, float* db_dev, void* stream);

/* ====================================================================================================================
 * BatchNorm1d + ReLU of SuperGlue's MLPs, training form
 * ==================================================================================================================== */

/* nn.BatchNorm1d followed by nn.ReLU, as they stand inside every MLP of
 * SuperGlue's keypoint encoder and GNN (superglue/models/superglue_train.py:46-57), in their training form -- one launch forward, one
 * backward.  Per channel c, over the valid columns of every pair, M of them in all:
 *
 *   forward    mean = sum x / M,  var = sum (x - mean)^2 / M (biased),  rstd = 1 / sqrt(var + eps)
 *              xhat = (x - mean) rstd,  z = fma(xhat, gamma, beta),  y = max(z, 0)
 *              running_mean = (1 - momentum) running_mean + momentum mean,  running_var likewise with var M / (M - 1)
 *   backward   g = dy where z > 0, else 0;  dbeta = sum g,  dgamma = sum g xhat
 *              dx = gamma rstd (g - dbeta / M - xhat dgamma / M)
 *
 * With use_batch_stats = 0 (a module in .eval()) mean is running_mean and rstd = 1 / sqrt(running_var + eps), nothing is updated, and
 * dx = gamma rstd g; dgamma and dbeta as above.  The backward takes x, mean and rstd, not y: it recomputes z by the forward's own
 * expression, so its mask equals y > 0 bit for bit.  Kept between the two calls: x and the 2 C floats of mean and rstd.
 *
 * Layout: the reference's own tensors, read and written in place: x, y, dy, dx (B,C,N) contiguous fp32 over a frame of N columns;
 * gamma, beta, mean, rstd, dgamma, dbeta, running_mean, running_var (C).  dgamma and dbeta are overwritten, not accumulated.  No
 * alignment beyond 4 bytes is assumed.  Outputs must not alias inputs (the running statistics are updated in place).  The host rejects
 * only the exact cases y = x and dx = x or dy; an output that overlaps an input in part, or mean / rstd on top of the running
 * statistics, is the caller's to avoid and is not detected.
 *
 * Ragged batches: n_dev[b] is read on the device (NULL = N; clamped to [0, N]).  Columns past the count are never read in x and dy and
 * may hold anything, NaN included; y and dx are written in full, with 0 there; such columns add nothing to any sum, and a pair of count
 * 0 adds nothing at all: results have the same bits with or without it.  The statistics of a ragged batch are, BY DEFINITION, those of
 * the reference's BatchNorm on the valid columns of all pairs concatenated along N into one tensor (1, C, M): that is what a layer on a
 * padded batch of pairs with different keypoint counts means here.
 *
 * Edge cases.  M = 0: y, dx, dgamma, dbeta, mean and rstd are 0, the running statistics and num_batches_tracked untouched.  M = 1 in
 * training mode, where PyTorch raises: with n_dev = NULL and B N = 1 the call returns an error; with counts it cannot be seen on the
 * host, and -- a stated departure -- the call computes with var = 0 and leaves running_var untouched (running_mean is updated).
 *
 * Arithmetic: fp32.  One workgroup of 256 threads per channel holds all of the channel's sums: thread t adds the valid columns t,
 * t + 256, ... of pair 0 in ascending order, then those of pair 1, and so on, into one accumulator; a fixed butterfly adds the 64 lanes
 * of a wave, and the four waves are added in ascending order.  The mean is formed around the channel's first valid value and the
 * variance in a second pass around the mean (a constant channel gives mean = its value, var = 0 and z = beta exactly).  No
 * floating-point atomics, no partial sums in memory, no workgroup that waits on another: the order of every sum is fixed at compile
 * time and depends on the counts only, so equal inputs give equal bits between calls, handles and frames.  When the frame has at most
 * 16 (pair, 256-column) slots per thread, B ceil(N / 256) <= 16, the channel stays in registers between the passes; otherwise the passes
 * read x again.  Both forms give the same bits.
 *
 * No scratch is drawn from the handle's workspace.  Asynchronous on the caller's stream, no host read.
 *
 * Not here: the score einsum, the residual adds, the optimiser step (the caller's framework runs them), BatchNorm without ReLU,
 * affine = False, momentum = None (the cumulative average), a second derivative.
 */

/* x (B,C,N), gamma, beta (C) -> y (B,C,N), mean, rstd (C).  use_batch_stats = 1: batch statistics; running_mean_dev, running_var_dev
 * and num_batches_tracked_dev (one int64, + 1 by one thread) may each be NULL and are otherwise updated in place by the same launch.
 * use_batch_stats = 0: running_mean_dev and running_var_dev are required and only read, num_batches_tracked_dev is ignored.
 * 1 <= B <= 65535, 1 <= C <= 1024, 1 <= N <= 2^20, eps > 0, 0 <= momentum <= 1: anything else, a null x / gamma / beta / y / mean /
 * rstd, y aliasing x, or B N = 1 with n_dev = NULL in training mode, returns an error code, sets imx_last_error and launches nothing. */
IMX_API int imx_bn_relu_forward_train(imx_handle_t h, int B, int C, int N, int use_batch_stats, float eps, float momentum,
                                      const float* x_dev, const float* gamma_dev, const float* beta_dev, const int32_t* n_dev,
                                      float* running_mean_dev, float* running_var_dev, int64_t* num_batches_tracked_dev,
                                      float* y_dev, float* mean_dev, float* rstd_dev, void* stream);

/* the same x, gamma, beta, the forward's mean and rstd, and dy (B,C,N) -> dx (B,C,N), dgamma, dbeta (C).  Any of dx_dev / dgamma_dev /
 * dbeta_dev may be NULL: that gradient is not written; the others keep their bits (all three NULL launches nothing).  The same bounds
 * and error rules; x, gamma, beta, mean, rstd and dy are required, and dx must not alias x or dy. */
IMX_API int imx_bn_relu_backward(imx_handle_t h, int B, int C, int N, int use_batch_stats,
                                 const float* x_dev, const float* gamma_dev, const float* beta_dev, const float* mean_dev,
                                 const float* rstd_dev, const float* dy_dev, const int32_t* n_dev,
                                 float* dx_dev, float* dgamma_dev, float* dbeta_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IMX_TRAIN_H */
