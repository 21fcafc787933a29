/* imx_lingrad.h -- C ABI of libimx_lingrad.so, the sixth library on libimx.so's handles (include/imx.h; beside imx_sptrain.h,
 * imx_spgrad.h, imx_otgrad.h and imx_mhagrad.h): nn.Conv1d(kernel_size=1) of SuperGlue's GNN, keypoint encoder and final projection
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
 * Built with the other five from one source tree (image-matching_amd/csrc/Makefile); use all from the SAME build.  The calls take an
 * imx_handle_t that libimx.so's imx_create made, report errors through imx_last_error and timing rows through imx_timing_report, and
 * follow the conventions at the top of imx.h.  Scratch, from the handle's workspace: "lin.part",
 *     B * ceil(N / 256) * Cout * (C0 + C1 + 1) floats
 * (one partial dw and db per pair and slab), drawn by a backward call that forms dw or db; every element that call reads it has written
 * before.  At B = 8, Cout = Cin = 512, N = 2048 that is 8 * 8 * 512 * 513 * 4 bytes = 64.1 MiB, beside 32 MiB each of xcat, dy and dx.
 * A library of its own because the symbol tables of the other five are pinned.  Asynchronous on the caller's stream, no host read.
 *
 * Not here: BatchNorm, ReLU, the score einsum, the optimiser step (the caller's framework runs them), kernel sizes other than 1, groups,
 * the 16-bit plane forms of the inference path, a second derivative.
 */
#ifndef IMX_LINGRAD_H
#define IMX_LINGRAD_H

#include "imx.h"

#ifdef __cplusplus
extern "C" {
#endif

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

#ifdef __cplusplus
}
#endif
#endif /* IMX_LINGRAD_H */
