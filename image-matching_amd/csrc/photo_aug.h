// photo_aug.h -- launchers of photo_aug.hip, kernels of libimx_photo.so (include/imx_photo.h): the photometric augmentation of SuperPoint's
// training data on (B,H,W) images.  DESIGN.md section 21 has the arithmetic, the launch structure and the summation order.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace imx {

constexpr int kPhotoTileW = 64, kPhotoTileH = 16;   // a workgroup of the pixel kernel: 256 threads, four consecutive pixels of a row each
constexpr int kPhotoThreads = 256;
constexpr int kShadeMaxE = 64;                      // ellipses per image
constexpr int kShadeMaxK = 351;                     // taps per image; the kernels keep them in 352 floats (a multiple of four, zero padded)
constexpr int kShadeTapSlots = 352;
constexpr int kShadeChunk = 64;                     // images per launch of a blur pass: their ksize travels in the kernel arguments
constexpr int kRowOut = 256, kRowRows = 4;          // row pass: 64 lanes x four consecutive outputs along x, four rows per workgroup
constexpr int kColW = 32, kColH = 32;               // column pass: 32 lanes along x, eight groups of four consecutive outputs along y

struct PixelArgs {
  const float* img;          // (B,H,W)
  const uint8_t* lut;        // (B,256)
  const float* noise_scale;  // (B)
  const uint32_t* thresh;    // (B)
  const uint8_t* table;      // (256)
  const float* blur_k;       // (B,9)
  const int32_t* blur_on;    // (B)
  const uint32_t* key;       // (B,2)
  uint8_t* out;              // (B,H,W)
  int B, H, W;
};

struct ShadeArgs {
  const uint8_t* img;        // (B,H,W)
  const float* ell;          // (B,E,5): cx, cy, ax, ay, angle in degrees
  const int32_t* n_ell;      // (B)
  const float* taps;         // (B,Kcap)
  const float* transparency; // (B)
  const int32_t* on;         // (B)
  uint8_t* mask;             // (B,H,W) workspace: 0 / 255
  float* tmp;                // (B,H,W) workspace: the row pass
  float* out;                // (B,H,W)
  int B, H, W, E, Kcap;
  int b0;                    // first image of this launch (the blur passes go 64 images at a time)
  uint16_t ks[kShadeChunk];  // ksize of the images b0 .. b0 + 63, validated on the host: odd, 3 .. min(351, Kcap)
};

inline bool photo_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
// the 16-byte form of the pixel kernel: a thread's four pixels are one float4 load and one dword store.  Both forms do the same
// operations per pixel, so the choice does not reach the bits.
inline bool pixels_x4(int W, const void* img, const void* out) { return W % 4 == 0 && photo_aligned(img, 16) && photo_aligned(out, 4); }

hipError_t launch_photo_pixels(const PixelArgs& a, hipStream_t s);
hipError_t launch_shade_mask(const ShadeArgs& a, hipStream_t s);    // mask, all B images
hipError_t launch_shade_rows(const ShadeArgs& a, int n, hipStream_t s);   // tmp of the images b0 .. b0 + n - 1
hipError_t launch_shade_cols(const ShadeArgs& a, int n, hipStream_t s);   // out of the images b0 .. b0 + n - 1

}  // namespace imx
