/* imx_sgloop.h -- C ABI of libimx_sgloop.so, a companion of libimx.so (include/imx.h), libimx_train.so (include/imx_train.h),
 * libimx_sgtrain.so (include/imx_sgtrain.h), libimx_spnet.so (include/imx_spnet.h), libimx_spnorm.so (include/imx_spnorm.h),
 * libimx_sppool.so (include/imx_sppool.h), libimx_photo.so (include/imx_photo.h) and libimx_sploop.so (include/imx_sploop.h) for
 * SuperGlue's training LOOP: the matches and matching scores that the reference's training forward returns with the loss on every step
 * (superglue/models/superglue_train.py:276-286), taken from the loss's OWN Sinkhorn -- no second one.
 *
 * The nine libraries are built together from one source tree (image-matching_amd/csrc/Makefile) and share the handle: every call
 * below takes an imx_handle_t that libimx.so's imx_create made, reports errors through imx_last_error and timing rows through
 * imx_timing_report / imx_timing_form, and follows the conventions at the top of imx.h (int return codes, caller-owned `*_dev`
 * pointers, asynchronous on the caller's stream, nothing thrown across the ABI).  They live in a library of their own because the
 * symbol tables of the other eight are pinned to their headers.  Use all libraries from the SAME build (the handle's layout is
 * internal to that build).
 *
 * No call reads device memory on the host, reads the environment, uses a floating-point atomic, a cooperative launch or a workgroup
 * that waits on another.  A null required pointer or a shape outside the bounds returns an error code, sets imx_last_error and
 * launches nothing.
 */
#ifndef IMX_SGLOOP_H
#define IMX_SGLOOP_H

#include "imx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ====================================================================================================================
 * imx_assignment_matches: the extraction of superglue_train.py:276-286 for B pairs, from scores and potentials
 * ====================================================================================================================
 *
 *   scores (B,N0,N1) fp32             n0 / n1 (B) int32 or NULL = N0 / N1, clamped to [0,N0] / [0,N1] as imx_ot_match_loss_grad does
 *   u (B,N0+1), v (B,N1+1) fp32       the final potentials of the log-domain Sinkhorn, or NULL = zeros (the last element of each row,
 *                                     the dustbin's, is never read)
 *   matches0 (B,N0), matches1 (B,N1)  int64, -1 = no match          mscores0 (B,N0), mscores1 (B,N1) fp32
 *   gt0 (B,N0) int64 and stats (B,3) int32: both or neither
 *
 * Per pair b with m = n0[b], n = n1[b], for i < m and j < n, in fp32 with every operation rounded on its own:
 *
 *   Z[i][j] = ((scores[i][j] + u[i]) + v[j]) - norm,     norm = -logf((float)(m + n))
 *
 * the expression and the normaliser that imx_ot_match_loss_grad's loss reads (one device function serves both), so a matching score
 * below is the expf of the very bits the loss takes the logarithm of.  Z is never stored; the dustbin row and column take no part, as
 * in the reference's Z[:, :-1, :-1].  Then
 *
 *   j*(i) = the column of the maximum of row i, i*(j) = the row of the maximum of column j; among EQUAL fp32 values the lowest index
 *           wins, on both sides (the first-occurrence rule of numpy.argmax)
 *   mscores0[i] = expf(Z[i][j*(i)]) where i*(j*(i)) == i (mutual), else 0         mscores1[j] = mscores0[i*(j)] where mutual, else 0
 *   matches0[i] = j*(i) where mutual and mscores0[i] > threshold (strict), else -1; matches1[j] likewise from mscores0[i*(j)]
 *   past the counts: matches -1, scores 0.   m = 0 or n = 0: everything -1 / 0, the three counts 0
 *   stats[b] = [gt0 >= 0, matches0 > -1, matches0 == gt0 >= 0] counted over i < m -- the three counts of imx_match_loss (imx.h)
 *
 * Rows past m and columns past n of scores, and gt0 past m, are never read and may hold anything.  A NaN INSIDE the valid block is
 * outside the contract: it is never chosen as a maximum, every index written stays in [-1, n) / [-1, m) and nothing faults.
 *
 * Three plain launches (row maxima, column maxima, one workgroup per pair for the rest); the matrix is read twice and never written;
 * 3 B (N0 + N1) words of the handle's workspace ("sgl.*"), each written by the call before it is read.  Equal inputs give equal bits
 * whatever the batch, the frame, the handle or the workspace held before.
 *
 * Bounds: 1 <= B <= 65535, 1 <= N0, N1 <= 2^20, threshold not NaN.
 */
IMX_API int imx_assignment_matches(imx_handle_t h, int B, const float* scores_dev, int N0, int N1, const int32_t* n0_dev, const int32_t* n1_dev,
                                   const float* u_dev, const float* v_dev, float threshold, const int64_t* gt0_dev, int64_t* matches0_dev,
                                   int64_t* matches1_dev, float* mscores0_dev, float* mscores1_dev, int32_t* stats_dev, void* stream);

/* ====================================================================================================================
 * imx_ot_match_loss_grad_matches: imx_ot_match_loss_grad (imx_train.h) and the matches of its own final potentials, one call
 * ====================================================================================================================
 *
 * The arguments up to flag_dev are imx_ot_match_loss_grad's, with its meanings and bounds; those from threshold on are
 * imx_assignment_matches'; the stream is last as everywhere.  The call runs imx_ot_match_loss_grad's launch sequence on the same kernels (one shared definition of the
 * sequence, the same kernel source compiled into this library), then the three launches above on u_T and v_T where they lie in the
 * workspace: loss, grad_scores, grad_bin and flag equal imx_ot_match_loss_grad's bit for bit, and the matches are those
 * imx_assignment_matches returns for the potentials of `iters` iterations (iters = 0: zeros).  One Sinkhorn, nothing of matrix size
 * stored beyond grad_scores.
 */
IMX_API int imx_ot_match_loss_grad_matches(imx_handle_t h, int B, const float* scores_dev, int N0, int N1, const int32_t* n0_dev,
                                           const int32_t* n1_dev, const float* bin_score_dev, int iters, const int64_t* all_matches_dev,
                                           const int32_t* n_all_dev, int L, const float* gout_dev, float* loss_dev, float* grad_scores_dev,
                                           float* grad_bin_dev, int32_t* flag_dev, float threshold, const int64_t* gt0_dev,
                                           int64_t* matches0_dev, int64_t* matches1_dev, float* mscores0_dev, float* mscores1_dev,
                                           int32_t* stats_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IMX_SGLOOP_H */
