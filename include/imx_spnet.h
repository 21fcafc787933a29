/* imx_spnet.h -- C ABI of libimx_spnet.so, a companion of libimx.so (include/imx.h), libimx_train.so (include/imx_train.h) and
 * libimx_sgtrain.so (include/imx_sgtrain.h) for SuperPoint's training step: the 3x3 convolutions of the network itself
 * (superpoint/models/unet_parts.py:10-25), forward and backward.
 *
 * The four libraries are built together from one source tree (image-matching_amd/csrc/Makefile) and share the handle: every call
 * below takes an imx_handle_t that libimx.so's imx_create made, reports errors through imx_last_error and timing rows through
 * imx_timing_report / imx_timing_form, and follows the conventions at the top of imx.h (int return codes, caller-owned `*_dev`
 * pointers, asynchronous on the caller's stream, nothing thrown across the ABI).  They live in a library of their own because the
 * symbol tables of the other three are pinned to their headers.  Use all libraries from the SAME build (the handle's layout is
 * internal to that build).
 */
#ifndef IMX_SPNET_H
#define IMX_SPNET_H

#include "imx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ====================================================================================================================
 * nn.Conv2d(Cin, Cout, 3, padding=1), training form
 * ==================================================================================================================== */

/* Stride 1, no dilation, no groups, fp32.  With x = 0 and dy = 0 outside the image:
 *
 *   forward    y [b][o][i][j] = bias[o] + sum_c sum_{u,v in 0..2} w[o][c][u][v] x[b][c][i+u-1][j+v-1]
 *   backward   dx[b][c][i][j] = sum_o sum_{u,v} w[o][c][u][v] dy[b][o][i-u+1][j-v+1]
 *              dw[o][c][u][v] = sum_b sum_{i,j} dy[b][o][i][j] x[b][c][i+u-1][j+v-1]
 *              db[o]          = sum_b sum_{i,j} dy[b][o][i][j]
 *
 * Layout: the reference's own tensors, read and written in place: x and dx (B,Cin,H,W), w and dw (Cout,Cin,3,3), bias and db (Cout),
 * y and dy (B,Cout,H,W), NCHW, contiguous fp32.  No alignment beyond 4 bytes is assumed, no channels-last copy and no packed weights
 * are made.  Outputs must not alias inputs or each other: an output whose byte range meets an input's or another output's is rejected.
 *
 * Arithmetic: every product on the fp32 matrix pipe (v_mfma_f32_32x32x2_f32), fp32 accumulation in two levels: MFMA chains from a zero
 * accumulator that are added to a running sum, which starts at +0.  y and dx: the summation channels in chunks of 8 (pairs of channels
 * ascending, the nine taps of a pair in row-major order; dx walks the flipped taps), chains of two chunks (72 MFMA steps -- not the
 * 64-step blocks of 128 of imx_train.h's 1x1 convolutions: 128 is no whole number of channels times nine taps); y adds the bias
 * last, and bias = NULL gives the bits of a zero bias.  dw and db: an image is cut into slabs of 16 rows; one workgroup sums a
 * slab's pixels in row-major order in chains of 128 pixels (64 MFMA steps) and writes a partial to scratch; a second kernel adds an
 * image's slabs ascending from +0, then the images ascending from +0, one thread per element.  db is the product with a column of ones.
 * No floating-point atomics, no workgroup that waits on another, no cooperative launch.  The order of every sum is fixed at compile
 * time and depends on (B, Cin, Cout, H, W) only, so equal inputs give equal bits between calls, handles and workspace histories, a
 * gradient's bits do not depend on which others are formed, and y and dx of an image do not depend on its batch.
 *
 * Scratch: the backward draws B ceil(H / 16) Cout (9 Cin + 1) floats ("conv3.part") from the handle's workspace when dw or db is
 * wanted; the forward draws none.  Asynchronous on the caller's stream, no host read.
 *
 * Not here: BatchNorm and ReLU (imx_train.h: imx_bn_relu_forward_train on the (B, C, H W) view), max-pooling, stride, dilation, groups,
 * other kernel sizes, the Winograd and 16-bit plane forms of the inference path, a second derivative.
 */

/* x (B,Cin,H,W), w (Cout,Cin,3,3), bias (Cout) or NULL -> y (B,Cout,H,W).
 * 1 <= B <= 65535, 1 <= Cin, Cout <= 1024, 1 <= H, W <= 4096, and no launch of either call may need more than 2^31 - 1 workgroups
 * (B ceil(H / 8) ceil(W / 32) ceil(max(Cin, Cout) / 64) for y and dx): anything else, a null x / w / y, or y overlapping an input,
 * returns an error code, sets imx_last_error and launches nothing. */
IMX_API int imx_conv3x3_forward_train(imx_handle_t h, int B, int Cout, int Cin, int H, int W,
                                      const float* x_dev, const float* w_dev, const float* bias_dev,
                                      float* y_dev, void* stream);

/* the same x and w, and dy (B,Cout,H,W) -> dx (B,Cin,H,W), dw (Cout,Cin,3,3), db (Cout), overwritten in full (not accumulated).
 * dx_dev / dw_dev / db_dev may each be NULL: dx = NULL skips the input-gradient kernel, dw and db both NULL skip the other two (all
 * three NULL launch nothing); the others keep their bits.  The same bounds and error rules; x, w and dy are required. */
IMX_API int imx_conv3x3_backward(imx_handle_t h, int B, int Cout, int Cin, int H, int W,
                                 const float* x_dev, const float* w_dev, const float* dy_dev,
                                 float* dx_dev, float* dw_dev, float* db_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IMX_SPNET_H */
