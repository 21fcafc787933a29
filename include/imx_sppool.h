/* imx_sppool.h -- C ABI of libimx_sppool.so, a companion of libimx.so (include/imx.h), libimx_train.so (include/imx_train.h),
 * libimx_sgtrain.so (include/imx_sgtrain.h), libimx_spnet.so (include/imx_spnet.h) and libimx_spnorm.so (include/imx_spnorm.h) for
 * SuperPoint's training step: nn.MaxPool2d(2) (superpoint/models/unet_parts.py:41) and the descriptor normalisation desc / ||desc||_2
 * (superpoint/models/superpoint_train.py:53-54), forward and backward on NCHW maps.
 *
 * The six libraries are built together from one source tree (image-matching_amd/csrc/Makefile) and share the handle: every call
 * below takes an imx_handle_t that libimx.so's imx_create made, reports errors through imx_last_error and timing rows through
 * imx_timing_report / imx_timing_form, and follows the conventions at the top of imx.h (int return codes, caller-owned `*_dev`
 * pointers, asynchronous on the caller's stream, nothing thrown across the ABI).  They live in a library of their own because the
 * symbol tables of the other five are pinned to their headers.  Use all libraries from the SAME build (the handle's layout is
 * internal to that build).
 *
 * Everything is fp32, NCHW contiguous, read and written in place.  No call reads on the host, draws on the handle's workspace, uses a
 * floating-point atomic, a cooperative launch or a workgroup that waits on another.  An output that shares a byte with an input or with
 * another output, a null required pointer or a shape outside the bounds returns an error code, sets imx_last_error and launches nothing.
 * Each launch reports its form through imx_timing_form: "x4" (16-byte loads and stores) or "x1" (dwords); the two give the same bits.
 */
#ifndef IMX_SPPOOL_H
#define IMX_SPPOOL_H

#include "imx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ====================================================================================================================
 * nn.MaxPool2d(2): kernel 2, stride 2, no padding, floor
 * ====================================================================================================================
 *
 *   forward    x (B,C,H,W) -> y (B,C,H/2,W/2), idx (B,C,H/2,W/2) bytes.  A window is scanned (0,0), (0,1), (1,0), (1,1) from its first
 *              element; a later one is taken when v > best || isnan(v).  That is PyTorch's rule: the first maximum wins a tie, -0 before
 *              +0 stays -0, a NaN wins and the last NaN keeps the index.  idx = 2 row + col of the taken element, 0..3.
 *   backward   dx (B,C,H,W) = dy at the recorded element of each window, +0 at every other element, the trailing row and column that an
 *              odd H or W leaves outside every window included.  Written in full, not accumulated; a select, never a product; neither x
 *              nor y is read.  An index byte outside 0..3 routes nothing.
 *
 * Pure streams: per input value the forward reads 4 bytes and writes 1 + 1/4 (a quarter as many outputs, 4 + 1 bytes each); the backward
 * reads 1 + 1/4 and writes 4.  The 16-byte form is taken when W % 8 == 0, x / dx and y / dy are
 * 16-byte aligned and idx is 4-byte aligned; otherwise dwords and bytes.  Nothing past a map's last element is touched.
 *
 * Bounds: 1 <= B <= 65535, 1 <= C <= 1024, 2 <= H, W <= 4096.
 */

/* idx_dev may be NULL (evaluation): y has the same bits. */
IMX_API int imx_maxpool2_forward_train(imx_handle_t h, int B, int C, int H, int W, const float* x_dev, float* y_dev, uint8_t* idx_dev,
                                       void* stream);

IMX_API int imx_maxpool2_backward(imx_handle_t h, int B, int C, int H, int W, const uint8_t* idx_dev, const float* dy_dev, float* dx_dev,
                                  void* stream);

/* ====================================================================================================================
 * desc / ||desc||_2 over the channels
 * ====================================================================================================================
 *
 *   forward    x (B,C,HW) -> norm (B,HW) = sqrtf(sum_c x^2), y (B,C,HW) = x / norm: a true division, no epsilon.  A pixel whose vector is
 *              zero gets NaN in all its channels (and in its dx); no other pixel is affected.
 *   backward   s = sum_c y_c dy_c,  dx_c = (dy_c - y_c s) / norm.
 *
 * Lanes run along pixels (channels are HW apart); a workgroup is 64 lanes x 4 waves, wave g adds the channels g, g + 4, ... ascending
 * with one fma each from +0, and the four partial sums are added in wave order.  The order is fixed at compile time and depends on C
 * alone, so a pixel's bits do not depend on B, on the other pixels, on the pointers or on an earlier call.  The inputs are read twice
 * (the sum, then the quotient); whether the second sweep comes from cache depends on C and was not measured.  The 16-byte form (a lane holds four consecutive pixels) is taken when
 * HW % 4 == 0, every pointer is 16-byte aligned and B HW >= 2^16.
 *
 * Bounds: B >= 1, 1 <= C <= 1024, 1 <= HW <= 2^24, B HW <= 2^31 - 1.
 */

IMX_API int imx_l2norm_forward_train(imx_handle_t h, int B, int C, int HW, const float* x_dev, float* y_dev, float* norm_dev, void* stream);

IMX_API int imx_l2norm_backward(imx_handle_t h, int B, int C, int HW, const float* y_dev, const float* norm_dev, const float* dy_dev,
                                float* dx_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IMX_SPPOOL_H */
