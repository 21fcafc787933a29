/* imx_spnorm.h -- C ABI of libimx_spnorm.so, a companion of libimx.so (include/imx.h), libimx_train.so (include/imx_train.h),
 * libimx_sgtrain.so (include/imx_sgtrain.h) and libimx_spnet.so (include/imx_spnet.h) for SuperPoint's training step: nn.BatchNorm2d,
 * optionally followed by nn.ReLU, forward and backward on NCHW maps (superpoint/models/unet_parts.py:10-25 with ReLU;
 * superpoint/models/superpoint_train.py:48, 51 without).
 *
 * The five libraries are built together from one source tree (image-matching_amd/csrc/Makefile) and share the handle: every call
 * below takes an imx_handle_t that libimx.so's imx_create made, reports errors through imx_last_error and timing rows through
 * imx_timing_report / imx_timing_form, and follows the conventions at the top of imx.h (int return codes, caller-owned `*_dev`
 * pointers, asynchronous on the caller's stream, nothing thrown across the ABI).  They live in a library of their own because the
 * symbol tables of the other four are pinned to their headers.  Use all libraries from the SAME build (the handle's layout is
 * internal to that build).
 */
#ifndef IMX_SPNORM_H
#define IMX_SPNORM_H

#include "imx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ====================================================================================================================
 * nn.BatchNorm2d [+ nn.ReLU], training form
 * ==================================================================================================================== */

/* A map is its flat run of HW = H W pixels; M = B HW values per channel.  fp32, NCHW contiguous, read and written in place.
 *
 *   forward    mean = sum x / M,  var = sum (x - mean)^2 / M (biased),  rstd = 1 / sqrtf(var + eps)       (use_batch_stats = 1)
 *              mean = running_mean,  rstd = 1 / sqrtf(running_var + eps)                                  (use_batch_stats = 0)
 *              xhat = (x - mean) rstd,  z = fma(xhat, gamma, beta),  y = relu ? (z > 0 ? z : 0) : z
 *              use_batch_stats = 1:  running_mean = (1 - momentum) running_mean + momentum mean,
 *                                    running_var  = (1 - momentum) running_var  + momentum var M / (M - 1),  num_batches_tracked += 1
 *   backward   g = relu ? (z > 0 ? dy : 0) : dy  (a select, never a product; z recomputed from x, mean, rstd by the forward's expression,
 *              so the mask equals y > 0 bit for bit),  dbeta = sum g,  dgamma = sum g xhat,
 *              dx = gamma rstd ((g - dbeta / M) - xhat dgamma / M)   (use_batch_stats = 1),   dx = gamma rstd g   (use_batch_stats = 0)
 *
 * Structure: a map is cut into slabs of 4096 consecutive pixels, one workgroup each, so the grid is ceil(HW / 4096) C B workgroups.
 * The training forward is three launches (slab statistics, a per-channel combine, the normalisation), the evaluation forward one; the
 * backward is up to three (slab sums, a per-channel combine, dx).  A slab's mean is formed around its first pixel and its M2 around
 * that mean, from registers; the combine joins (count, mean, M2) pairwise in float64, the slabs of an image ascending, then the images
 * ascending, and the backward's sums are added in float64 in the same order and rounded once.  No floating-point atomics, no workgroup
 * that waits on another, no cooperative launch.  The order of every sum is fixed at compile time and depends on (B, C, HW) only, so
 * equal inputs give equal bits between calls, handles, workspace histories and pointer alignments, a gradient's bits do not depend on
 * which others are formed, and in evaluation mode y and dx of an image do not depend on its batch.  A constant channel gives
 * mean = its value, var = 0 and z = beta exactly.
 *
 * Scratch: 2 B C ceil(HW / 4096) floats ("bn2d.part") from the handle's workspace, written by the call that reads them; the evaluation
 * forward and an evaluation backward that forms dx alone draw none.  Asynchronous on the caller's stream, no host read.
 *
 * Bounds: 1 <= B <= 65535, 1 <= C <= 1024, 1 <= HW <= 2^24, B HW <= 2^31 - 1, eps > 0, 0 <= momentum <= 1; in training mode B HW > 1.
 * Outputs (the running statistics and num_batches_tracked among them) must not share a byte with an input or another output.  Anything
 * else returns an error code, sets imx_last_error and launches nothing.
 *
 * Not here: max-pooling, the descriptor normalisation, momentum = None, affine = False, a second derivative.
 */

/* x (B,C,HW), gamma, beta (C) -> y (B,C,HW), mean, rstd (C).  use_batch_stats = 1: running_mean_dev, running_var_dev (C) and
 * num_batches_tracked_dev (one int64) are updated in place; each may be NULL.  use_batch_stats = 0: both running statistics are
 * required and nothing is updated; mean and rstd receive what was used. */
IMX_API int imx_bn2d_forward_train(imx_handle_t h, int B, int C, int HW, int relu, int use_batch_stats, float eps, float momentum,
                                   const float* x_dev, const float* gamma_dev, const float* beta_dev,
                                   float* running_mean_dev, float* running_var_dev, int64_t* num_batches_tracked_dev,
                                   float* y_dev, float* mean_dev, float* rstd_dev, void* stream);

/* the same x, gamma, beta, the forward's mean and rstd, and dy (B,C,HW) -> dx (B,C,HW), dgamma, dbeta (C), overwritten in full (not
 * accumulated).  dx_dev / dgamma_dev / dbeta_dev may each be NULL: the others keep their bits; all three NULL launch nothing. */
IMX_API int imx_bn2d_backward(imx_handle_t h, int B, int C, int HW, int relu, int use_batch_stats,
                              const float* x_dev, const float* gamma_dev, const float* beta_dev,
                              const float* mean_dev, const float* rstd_dev, const float* dy_dev,
                              float* dx_dev, float* dgamma_dev, float* dbeta_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IMX_SPNORM_H */
