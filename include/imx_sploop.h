/* imx_sploop.h -- C ABI of libimx_sploop.so, a companion of libimx.so (include/imx.h), libimx_train.so (include/imx_train.h),
 * libimx_sgtrain.so (include/imx_sgtrain.h), libimx_spnet.so (include/imx_spnet.h), libimx_spnorm.so (include/imx_spnorm.h),
 * libimx_sppool.so (include/imx_sppool.h) and libimx_photo.so (include/imx_photo.h) for SuperPoint's training LOOP: the soft labels of
 * the shipped configuration's `gaussian_label` (imx_warp_labels_bi: datasets/data_tools.py:9-34 get_labels_bi, then the 8-bit
 * quantisation of utils/photometric.py:72-77) and the optimiser step (imx_adam_flat: torch.optim.Adam on one flat arena, one launch).
 *
 * The eight libraries are built together from one source tree (image-matching_amd/csrc/Makefile) and share the handle: every call
 * below takes an imx_handle_t that libimx.so's imx_create made, reports errors through imx_last_error and timing rows through
 * imx_timing_report / imx_timing_form, and follows the conventions at the top of imx.h (int return codes, caller-owned `*_dev`
 * pointers, asynchronous on the caller's stream, nothing thrown across the ABI).  They live in a library of their own because the
 * symbol tables of the other seven are pinned to their headers.  Use all libraries from the SAME build (the handle's layout is
 * internal to that build).
 *
 * No call reads device memory on the host, reads the environment, uses a floating-point atomic, a cooperative launch or a workgroup
 * that waits on another.  A null required pointer or a shape outside the bounds returns an error code, sets imx_last_error and
 * launches nothing.
 */
#ifndef IMX_SPLOOP_H
#define IMX_SPLOOP_H

#include "imx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ====================================================================================================================
 * imx_warp_labels_bi: get_labels_bi as warpLabels(..., bilinear=True) calls it, for B images
 * ====================================================================================================================
 *
 *   pts (B,Kcap,2) fp32 (x, y)        counts (B) int32 or NULL = Kcap, clamped to 0..Kcap; rows past the count are never read
 *   mats (B,3,3) fp32, PIXEL space    out (B,H,W) fp32, written in full (zero where no entry lands)
 *   flag (1) int32 or NULL            levels 0 or 255
 *
 * Per point i < count, float32, no contraction except where written:
 *   1. (x, y) = trunc(pts)                                          .long()
 *   2. (u, v, w) = rows of mats[b] @ (x, y, 1), each row fma(m2, 1, fma(m1, y, m0 x)); p = (u / w, v / w): the expression of
 *      imx_warp_labels (imx_train.h), the same device function.  NO filter on p.
 *   3. a non-finite p is dropped and sets bit 1 of *flag.
 *   4. q = trunc(p) toward zero per coordinate, r = p - q, e = 1 - r (rounded), and the four entries in the reference's concatenation
 *      order k = 0..3:
 *        k = 0  (qx,     qy    )  ex * ey
 *        k = 1  (qx,     qy + 1)  ex * ry
 *        k = 2  (qx + 1, qy    )  rx * ey
 *        k = 3  (qx + 1, qy + 1)  rx * ry          one rounded product each
 *   5. an entry is kept iff 0 <= cx <= W - 1 and 0 <= cy <= H - 1 (filter_points), compared in float32 as the reference does.
 *   6. several kept entries on one pixel: the one with the highest order index k * count + i writes.  That is the reference's
 *      sequence under sequential assignment (torch defines no order for an indexed assignment with repeated indices; like
 *      imx_warp_labels this library picks the sequential one).  Resolved with an integer atomicMax on an int32 map in the handle's
 *      workspace ("spl.owner", written in full by every call) and a second pass that recomputes the winner's weight: the result does
 *      not depend on scheduling, on an earlier call, on B or on the image's place in the batch.
 *   7. levels = 0: the weight itself.  levels = 255: trunc(w * 255.0f) clamped to [0, 255], then / 255.0f -- the
 *      (img * 255).astype(np.uint8) ... astype(np.float32) / 255 of ImgAugTransform.__call__.
 *
 * A weight outside [0, 1] arises only for a warped coordinate in (-1, 0), where trunc gives 0 and r is negative; the reference's cast
 * to uint8 is undefined there.  The clamp of step 7 is this project's choice; a kept entry with such a weight sets bit 0 of *flag
 * (for either value of levels; with levels = 0 the raw weight is written).  *flag is zeroed by the call before anything sets a bit.
 *
 * Bounds: 1 <= B <= 65535, 0 <= Kcap < 2^29, H, W >= 1, B H W <= 2^31.
 */
IMX_API int imx_warp_labels_bi(imx_handle_t h, const float* pts_dev, const int32_t* counts_dev, int B, int Kcap, const float* mats_dev, int H,
                               int W, int levels, float* out_dev, int32_t* flag_dev, void* stream);

/* ====================================================================================================================
 * imx_adam_flat: one step of torch.optim.Adam (amsgrad=False, maximize=False) on n contiguous floats, ONE launch
 * ====================================================================================================================
 *
 *   p, g, m, v (n) fp32: parameters, gradients, exp_avg, exp_avg_sq; distinct, non-overlapping
 *
 * Per element, float32, every operation rounded on its own (no contraction), in exactly this order:
 *   g1 = weight_decay != 0 ? g + weight_decay * p : g
 *   m  = m + (1 - beta1) * (g1 - m)                    t1 = g1 - m;  t2 = c1 * t1;  m = m + t2            c1 = (float)(1 - beta1)
 *   v  = beta2 * v + (1 - beta2) * g1 * g1             a = beta2 * v;  b = c2 * g1;  c = b * g1;  v = a + c   c2 = (float)(1 - beta2)
 *   p  = p - step_size * m / (sqrt(v) * inv_sqrt_bc2 + eps)
 *                                                      s = sqrtf(v) (correctly rounded);  d = s * inv_sqrt_bc2;  d = d + eps;
 *                                                      q = m / d (correctly rounded);  q = step_size * q;  p = p - q
 * step_size = lr / (1 - beta1^t) and inv_sqrt_bc2 = 1 / sqrt(1 - beta2^t) are formed by the caller on the host in double.  The six scalars
 * are passed by value as doubles and each is rounded to float32 once, in the library (c1 and c2 from the double differences); nothing is
 * read from the device on the host.  0 <= beta1, beta2 < 1, eps >= 0, everything finite, 0 <= n <= 2^38.  zero_grad != 0 stores +0 to g after reading it.
 *
 * 16-byte loads and stores where the four pointers are 16-byte aligned ("x4"), dwords otherwise ("x1"); the tail of the x4 form is
 * dwords.  Both do the same operations per element, so the choice does not reach the bits.  Any n >= 0 (n = 0 launches nothing);
 * offsets are 64-bit.  Nothing is drawn from the handle's workspace.
 */
IMX_API int imx_adam_flat(imx_handle_t h, float* p_dev, float* g_dev, float* m_dev, float* v_dev, int64_t n, double step_size, double beta1,
                          double beta2, double inv_sqrt_bc2, double eps, double weight_decay, int zero_grad, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IMX_SPLOOP_H */
