/* imx_bngrad.h -- C ABI of libimx_bngrad.so, the seventh library on libimx.so's handles (include/imx.h; beside imx_sptrain.h,
 * imx_spgrad.h, imx_otgrad.h, imx_mhagrad.h and imx_lingrad.h): nn.BatchNorm1d followed by nn.ReLU, as they stand inside every MLP of
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
 * Built with the other six from one source tree (image-matching_amd/csrc/Makefile); use all from the SAME build.  The calls take an
 * imx_handle_t that libimx.so's imx_create made, report errors through imx_last_error and timing rows through imx_timing_report, and
 * follow the conventions at the top of imx.h.  No scratch is drawn from the handle's workspace.  A library of its own because the
 * symbol tables of the other six are pinned.  Asynchronous on the caller's stream, no host read.
 *
 * Not here: the score einsum, the residual adds, the optimiser step (the caller's framework runs them), BatchNorm without ReLU,
 * affine = False, momentum = None (the cumulative average), a second derivative.
 */
#ifndef IMX_BNGRAD_H
#define IMX_BNGRAD_H

#include "imx.h"

#ifdef __cplusplus
extern "C" {
#endif

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
#endif /* IMX_BNGRAD_H */
