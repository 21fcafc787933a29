/* imx_sgtrain.h -- C ABI of libimx_sgtrain.so, a companion of libimx.so (include/imx.h) and libimx_train.so (include/imx_train.h) for
 * SuperGlue's training step: the score product between the two images' projected descriptors, forward and backward.  With it every
 * matrix product of the reference's training forward (superglue/models/superglue_train.py:174-307) is in the libraries.
 *
 * The three libraries are built together from one source tree (image-matching_amd/csrc/Makefile) and share the handle: every call
 * below takes an imx_handle_t that libimx.so's imx_create made, reports errors through imx_last_error and timing rows through
 * imx_timing_report / imx_timing_form, and follows the conventions at the top of imx.h (int return codes, caller-owned `*_dev`
 * pointers, asynchronous on the caller's stream, nothing thrown across the ABI).  They live in a library of their own because the
 * symbol tables of the other two are pinned: libimx.so's to the 34 entry points of imx.h, libimx_train.so's to the 14 of imx_train.h
 * -- the reason libimx_train.so was split from libimx.so in the first place.  Folding this library into libimx_train.so is a
 * refactoring of its own.  Use all libraries from the SAME build (the handle's layout is internal to that build).
 */
#ifndef IMX_SGTRAIN_H
#define IMX_SGTRAIN_H

#include "imx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ====================================================================================================================
 * the score product of SuperGlue, training form
 * ==================================================================================================================== */

/* scores = torch.einsum('bdn,bdm->bnm', mdesc0, mdesc1) / descriptor_dim ** .5 (superglue/models/superglue_train.py:267-268) in its
 * training form, forward and the gradients at both inputs.  Per pair b, with A = a[b] (D, N0), Bm = b[b] (D, N1), n0 = n0_dev[b] and
 * n1 = n1_dev[b]:
 *
 *   forward    S[n][m]   = scale sum_d A[d][n] Bm[d][m]          (B, N0, N1)
 *   backward   dA[d][n]  = scale sum_m dS[n][m] Bm[d][m]         (B, D, N0)
 *              dBm[d][m] = scale sum_n dS[n][m] A[d][n]          (B, D, N1)
 *
 * Layout: the reference's own tensors, read and written in place: a (B,D,N0), b (B,D,N1), scores and dscores (B,N0,N1), da the shape
 * of a, db the shape of b, contiguous fp32.  No alignment beyond 4 bytes is assumed.  Outputs must not alias inputs or each other: an
 * output whose byte range meets an input's is rejected.
 *
 * Ragged batches: n0_dev[b] and n1_dev[b] are read on the device (NULL = N0 / N1; clamped to [0,N0] / [0,N1]).  Columns of a past n0,
 * columns of b past n1 and dscores outside [0,n0) x [0,n1) are never read and may hold anything, NaN included.  scores, da and db are
 * written in full, with 0 past the counts; n0 = 0 or n1 = 0 gives zeros everywhere for that pair.  A 64 x 64 tile that lies wholly
 * past a count writes its zeros before any load.
 *
 * Arithmetic: every product on the fp32 matrix pipe (v_mfma_f32_32x32x2_f32), fp32 accumulation in two levels: the summation index
 * is cut into blocks of 128, a block accumulates as one MFMA chain from a zero accumulator (index ascending) and is then added to the
 * running sum, blocks ascending, the running sum starting at +0; the finished sum is multiplied by scale once.  scores: the channel
 * 0 .. D-1.  da: the column 0 .. n1-1 of the pair.  db: the row 0 .. n0-1 of the pair.  Blocks past a count are skipped, not added as
 * zeros.  One workgroup forms the whole sum of its 64 x 64 output tile: the summation index is NOT split between workgroups, there are
 * no partial sums in memory, no floating-point atomics, no workgroup that waits on another and no cooperative launch.  The order of
 * every sum is fixed at compile time and depends on the pair's own counts only, so equal inputs give equal bits between calls,
 * handles, frames (N0, N1), batch compositions and workspace histories, and a gradient's bits do not depend on whether the other is
 * formed.
 *
 * No scratch is drawn from the handle's workspace.  Asynchronous on the caller's stream, no host read.
 *
 * Not here: the optimal-transport layer and the match loss (imx_train.h: imx_ot_match_loss_grad), the final projection that produces a
 * and b (imx_train.h: imx_conv1x1_forward_train), the residual adds, the optimiser step (the caller's framework runs them), a batch
 * matrix product of any other layout, the 16-bit plane forms of the inference path, a second derivative.
 */

/* a (B,D,N0), b (B,D,N1) -> scores (B,N0,N1).
 * 1 <= B <= 65535, 1 <= D <= 1024, 1 <= N0, N1 <= 2^20, B ceil(N0 / 64) ceil(N1 / 64) <= 2^31 - 1, scale finite: anything else, a null
 * a / b / scores, or scores overlapping a or b, returns an error code, sets imx_last_error and launches nothing. */
IMX_API int imx_score_product_forward_train(imx_handle_t h, int B, int D, int N0, int N1,
                                            const float* a_dev, const float* b_dev,
                                            const int32_t* n0_dev, const int32_t* n1_dev,
                                            float scale, float* scores_dev, void* stream);

/* the same a, b and scale, and dscores (B,N0,N1) -> da (B,D,N0), db (B,D,N1).
 * da_dev / db_dev may each be NULL: that gradient is not formed and its kernel is skipped (both NULL launches nothing); the other keeps
 * its bits.  The same bounds and error rules; a, b and dscores are required, and da / db must overlap neither an input nor each
 * other. */
IMX_API int imx_score_product_backward(imx_handle_t h, int B, int D, int N0, int N1,
                                       const float* a_dev, const float* b_dev, const float* dscores_dev,
                                       const int32_t* n0_dev, const int32_t* n1_dev, float scale,
                                       float* da_dev, float* db_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IMX_SGTRAIN_H */
