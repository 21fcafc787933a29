/* imx_photo.h -- C ABI of libimx_photo.so, a companion of libimx.so (include/imx.h), libimx_train.so (include/imx_train.h),
 * libimx_sgtrain.so (include/imx_sgtrain.h), libimx_spnet.so (include/imx_spnet.h), libimx_spnorm.so (include/imx_spnorm.h) and
 * libimx_sppool.so (include/imx_sppool.h) for SuperPoint's training data: the photometric augmentation the reference applies to the image
 * and to the warped image of every training pair (datasets/ALLSS.py:116-128, utils/photometric.py) -- brightness, contrast, Gaussian
 * noise, impulse noise and motion blur in the reference's fixed order (imx_photo_pixels), then the additive shade (imx_photo_shade).
 *
 * The seven libraries are built together from one source tree (image-matching_amd/csrc/Makefile) and share the handle: every call
 * below takes an imx_handle_t that libimx.so's imx_create made, reports errors through imx_last_error and timing rows through
 * imx_timing_report / imx_timing_form, and follows the conventions at the top of imx.h (int return codes, caller-owned `*_dev`
 * pointers, asynchronous on the caller's stream, nothing thrown across the ABI).  They live in a library of their own because the
 * symbol tables of the other six are pinned to their headers.  Use all libraries from the SAME build (the handle's layout is
 * internal to that build).
 *
 * Every random PARAMETER is an input the caller drew, one entry per image; every per-PIXEL draw comes from Philox4x32-10 inside the
 * kernel, counter (pixel index low, pixel index high, 0, 0) with pixel index = y W + x, key = the image's own.  An image's result depends
 * on its own parameters and key alone: not on B, on its place in the batch, on the other images or on an earlier call.  No call reads
 * device memory on the host, uses a floating-point atomic, a cooperative launch or a workgroup that waits on another.  A null required
 * pointer, an output that shares a byte with an input, or a shape or host-side parameter outside the bounds returns an error code, sets
 * imx_last_error and launches nothing.  A device-side parameter cannot be checked without a read: whatever it holds, no address outside
 * the images is formed (a count is clamped to its capacity, a table index is a byte).
 *
 * Bounds of both calls: 1 <= B <= 65535, 2 <= H, W <= 4096.  Everything is contiguous.
 */
#ifndef IMX_PHOTO_H
#define IMX_PHOTO_H

#include "imx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ====================================================================================================================
 * imx_photo_pixels: iaa.Add, iaa.LinearContrast, iaa.AdditiveGaussianNoise, iaa.ImpulseNoise, iaa.MotionBlur(3)
 * ====================================================================================================================
 *
 *   img (B,H,W) fp32 in [0,1]          lut (B,256) bytes               noise_scale (B) fp32           thresh (B) uint32
 *   table (256) bytes, shared           blur_kernel (B,9) fp32          blur_on (B) int32              key (B,2) uint32
 *   out (B,H,W) bytes
 *
 * Per pixel, in this order (float32, no contraction):
 *   1. q = trunc(clamp(x * 255, 0, 255))                       the reference's (img * 255).astype(uint8); a NaN gives 0
 *   2. a = lut[b][q]                                           brightness and contrast, composed into one table by the caller
 *   3. a = clamp(a + rne(noise_scale[b] * z), 0, 255)          z = sqrtf(-2 logf(u1)) * cospif(2 u2),
 *                                                              u1 = ((r0 >> 8) + 1) 2^-24, u2 = (r1 >> 8) 2^-24, both exact
 *   4. where (r2 >> 8) < thresh[b]:  a = table[r3 >> 24]       thresh = ceil(p 2^24) replaces a pixel with probability p
 *   5. where blur_on[b] != 0: the result of step 4 correlated with blur_kernel[b] under BORDER_REFLECT_101 -- taps in row-major
 *      order, one product and one add per tap from +0 -- then rne, saturated to 0..255
 * (r0, r1, r2, r3) = Philox4x32-10 as above; rne is round to nearest, ties to even.
 *
 * The 16-byte form ("x4": one float4 load and one dword store per four pixels) is taken when W % 4 == 0, img is 16-byte and out 4-byte
 * aligned; otherwise dwords and bytes ("x1").  The two give the same bits.  Nothing is drawn from the handle's workspace.
 */
IMX_API int imx_photo_pixels(imx_handle_t h, int B, int H, int W, const float* img_dev, const uint8_t* lut_dev, const float* noise_scale_dev,
                             const uint32_t* thresh_dev, const uint8_t* table_dev, const float* blur_kernel_dev, const int32_t* blur_on_dev,
                             const uint32_t* key_dev, uint8_t* out_dev, void* stream);

/* ====================================================================================================================
 * imx_photo_shade: customizedTransform.additive_shade
 * ====================================================================================================================
 *
 *   img (B,H,W) bytes                   ellipses (B,E,5) fp32: cx, cy, ax, ay, angle in degrees          n_ellipses (B) int32, clamped to 0..E
 *   taps (B,Kcap) fp32                  ksize (B) int32 ON THE HOST: odd, 3 <= ksize <= min(351, Kcap)   transparency (B) fp32
 *   on (B) int32                        out (B,H,W) fp32
 *
 *   1. mask = 255 where the pixel (x, y) lies in the union of the image's ellipses, 0 elsewhere, decided in double:
 *      ((dx cos + dy sin) / ax)^2 + ((dy cos - dx sin) / ay)^2 <= 1, dx = x - cx, dy = y - cy, (sin, cos) = sincospi(angle / 180).
 *      Analytic: OpenCV's cv2.ellipse fills a polygon approximation (unpinned).
 *   2. m = the mask blurred along x with taps[b][0 .. ksize), then along y, under BORDER_REFLECT_101 with as many bounces as the halo
 *      needs, float32: one fma per tap, taps ascending, from +0.  The order of a pixel's sum depends on ksize alone.
 *   3. out = clamp(v * (1 - transparency[b] * m / 255), 0, 255) / 255,  v = (a / 255) * 255, float32 in this order.
 *   4. on[b] == 0: out = a / 255.
 *
 * ksize is read on the host during the call (it sizes the halo, so it is checked: an even value, one below 3 or above Kcap is an
 * error) and travels to the kernels in their arguments, 64 images per launch of a blur pass.  The mask (B H W bytes) and the row pass
 * (B H W floats) go through the handle's workspace; no result depends on what an earlier call left there.  1 <= E <= 64, 3 <= Kcap <= 351.
 */
IMX_API int imx_photo_shade(imx_handle_t h, int B, int H, int W, int E, int Kcap, const uint8_t* img_dev, const float* ellipses_dev,
                            const int32_t* n_ellipses_dev, const float* taps_dev, const int32_t* ksize_host, const float* transparency_dev,
                            const int32_t* on_dev, float* out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IMX_PHOTO_H */
