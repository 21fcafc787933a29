// photo_aug.hip -- the photometric augmentation of SuperPoint's training data on (B,H,W) images (include/imx_photo.h).
//
//   photo_pixels   grid (ceil(W / 64), ceil(H / 16), B), 256 threads, a thread = four consecutive pixels of a row.  Per pixel: quantise,
//                  the image's table, Gaussian noise (Box-Muller on Philox4x32-10 of (pixel index, image key)), impulse noise.  Where the
//                  image's blur word is set the noisy tile meets in LDS with a one-pixel ring (the ring's pixels are computed a second
//                  time from their own counters: 164 per 1024) and each thread correlates its pixels with the image's 3x3 kernel.  The
//                  neighbours of an image pixel under BORDER_REFLECT_101 are image pixels of the same 3x3 window, so the ring holds
//                  image pixels only.  LDS rather than nine recomputations: a draw costs ten Philox rounds, a logarithm, a root and a
//                  cosine, about 150 VALU operations, against one byte through LDS
//   shade_mask     grid (ceil(H W / 256), 1, B): 255 where the pixel lies in the union of the image's ellipses, in double, one byte each
//   shade_rows     grid (ceil(W / 256), ceil(H / 4), images of the chunk): the Gaussian along x of the mask.  A wave holds one row segment
//                  of 256 outputs + ksize - 1 mask values in LDS; a lane adds its four consecutive outputs tap by tap, ascending, one fma
//                  each from +0, the window sliding through registers (two 16-byte LDS reads per sixteen fma)
//   shade_cols     grid (ceil(W / 32), ceil(H / 32), images of the chunk): the Gaussian along y of the row pass, 32 lanes along x, a thread
//                  four consecutive outputs along y, the same order; then the shading itself
//
// The taps sit in LDS padded with +0 to a multiple of four: a padded step adds +0 x (a finite window value, or +0) to a non-negative sum and
// leaves its bits.  The order of a pixel's sum depends on ksize alone.  BORDER_REFLECT_101 takes as many bounces as the halo needs.
// No floating-point atomics, no workgroup that waits on another.  Loads and stores are predicated: nothing past an image's last element
// is touched, whatever the parameter arrays hold (a count is clamped to its capacity, a table index is a byte).  Contraction is off: every
// fused multiply-add is written as one.  Every offset is 64-bit.
#include "photo_aug.h"

#pragma clang fp contract(off)

namespace imx {

namespace {

// i reflected into [0, n) without repeating the border sample (cv::BORDER_REFLECT_101), any number of bounces; n >= 2
__device__ __forceinline__ int reflect101(int i, int n) {
  const int p = 2 * n - 2;
  int m = i % p;
  if (m < 0) m += p;
  return m < n ? m : p - m;
}

// Philox4x32-10 (Salmon et al., SC'11; Random123) of the counter (c0, c1, 0, 0) under the key (k0, k1)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1, uint32_t (&r)[4]) {
  uint32_t x0 = c0, x1 = c1, x2 = 0u, x3 = 0u;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, x0), lo0 = 0xD2511F53u * x0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, x2), lo1 = 0xCD9E8D57u * x2;
    x0 = hi1 ^ x1 ^ k0;
    x1 = lo1;
    x2 = hi0 ^ x3 ^ k1;
    x3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  r[0] = x0; r[1] = x1; r[2] = x2; r[3] = x3;
}

struct PixelParams {
  float scale;
  uint32_t thresh, k0, k1;
};

// steps 1 to 4 of imx_photo_pixels for the pixel `idx` = y W + x of its image
__device__ __forceinline__ uint32_t noisy_pixel(float x, uint64_t idx, const PixelParams& p, const uint8_t* lut_s, const uint8_t* tab_s) {
  const float xs = fminf(fmaxf(x * 255.f, 0.f), 255.f);      // a NaN pixel quantises to 0
  float a = (float)lut_s[(int)xs];
  uint32_t r[4];
  philox4x32_10((uint32_t)idx, (uint32_t)(idx >> 32), p.k0, p.k1, r);
  const float u1 = (float)((r[0] >> 8) + 1u) * 0x1p-24f;     // (0, 1], exact
  const float u2x2 = (float)(r[1] >> 8) * 0x1p-23f;          // 2 u2 in [0, 2), exact: cos(2 pi u2) = cospif(2 u2)
  const float z = sqrtf(-2.f * logf(u1)) * cospif(u2x2);
  a = fminf(fmaxf(a + rintf(p.scale * z), 0.f), 255.f);
  uint32_t v = (uint32_t)a;
  if ((r[2] >> 8) < p.thresh) v = tab_s[r[3] >> 24];
  return v;
}

constexpr int kTileStride = kPhotoTileW + 4;   // bytes of a tile row in LDS: 64 pixels, the ring, padding to a multiple of four

template <bool X4>
__global__ __launch_bounds__(kPhotoThreads) void photo_pixels_kernel(PixelArgs a) {
  __shared__ uint8_t lut_s[256], tab_s[256];
  __shared__ uint8_t tile[(kPhotoTileH + 2) * kTileStride];
  const int b = blockIdx.z, tid = threadIdx.x, H = a.H, W = a.W;
  lut_s[tid] = a.lut[(size_t)b * 256 + tid];
  tab_s[tid] = a.table[tid];
  __syncthreads();
  const PixelParams p{a.noise_scale[b], a.thresh[b], a.key[2 * (size_t)b], a.key[2 * (size_t)b + 1]};
  const bool blur = a.blur_on[b] != 0;                        // the same for every thread of the workgroup
  const int x0 = (int)blockIdx.x * kPhotoTileW, y0 = (int)blockIdx.y * kPhotoTileH;
  const int r = tid >> 4, c = (tid & 15) * 4;
  const int y = y0 + r, x = x0 + c;
  const size_t plane = (size_t)b * H * W;
  const float* img = a.img + plane;
  uint8_t* out = a.out + plane;
  const bool live = y < H && x < W;
  const size_t at = (size_t)(live ? y : 0) * W + (size_t)(live ? x : 0);
  uint32_t v[4] = {0u, 0u, 0u, 0u};
  if (live) {
    float px[4];
    if constexpr (X4) {
      const float4 q = *reinterpret_cast<const float4*>(img + at);
      px[0] = q.x; px[1] = q.y; px[2] = q.z; px[3] = q.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) px[j] = x + j < W ? img[at + j] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (X4 || x + j < W) v[j] = noisy_pixel(px[j], (uint64_t)at + j, p, lut_s, tab_s);
  }
  if (blur) {
#pragma unroll
    for (int j = 0; j < 4; ++j) tile[(r + 1) * kTileStride + c + 1 + j] = (uint8_t)v[j];
    // the ring: the rows above and below (66 pixels each), then the columns left and right (16 each); image pixels only
    constexpr int kRing = 2 * (kPhotoTileW + 2) + 2 * kPhotoTileH;
    if (tid < kRing) {
      int tr, tc;
      if (tid < 2 * (kPhotoTileW + 2)) {
        tr = tid < kPhotoTileW + 2 ? 0 : kPhotoTileH + 1;
        tc = tid < kPhotoTileW + 2 ? tid : tid - (kPhotoTileW + 2);
      } else {
        const int k = tid - 2 * (kPhotoTileW + 2);
        tr = 1 + (k >> 1);
        tc = (k & 1) ? kPhotoTileW + 1 : 0;
      }
      const int gy = y0 + tr - 1, gx = x0 + tc - 1;
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
        const size_t g = (size_t)gy * W + gx;
        tile[tr * kTileStride + tc] = (uint8_t)noisy_pixel(img[g], (uint64_t)g, p, lut_s, tab_s);
      }
    }
    __syncthreads();
    if (live) {
      float k[9];
#pragma unroll
      for (int t = 0; t < 9; ++t) k[t] = a.blur_k[(size_t)b * 9 + t];
      const int ru = reflect101(y - 1, H) - y0 + 1, rd = reflect101(y + 1, H) - y0 + 1;
      const int rows[3] = {ru, r + 1, rd};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (!X4 && x + j >= W) continue;
        const int cl = reflect101(x + j - 1, W) - x0 + 1, cr = reflect101(x + j + 1, W) - x0 + 1;
        const int cols[3] = {cl, c + j + 1, cr};
        float acc = 0.f;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) {
            const float prod = k[dy * 3 + dx] * (float)tile[rows[dy] * kTileStride + cols[dx]];
            acc = acc + prod;
          }
        v[j] = (uint32_t)fminf(fmaxf(rintf(acc), 0.f), 255.f);
      }
    }
  }
  if (!live) return;
  if constexpr (X4) {
    *reinterpret_cast<uint32_t*>(out + at) = v[0] | v[1] << 8 | v[2] << 16 | v[3] << 24;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x + j < W) out[at + j] = (uint8_t)v[j];
  }
}

// ---------------------------------------------------------------------------------------------------------------- additive shade

__global__ __launch_bounds__(kPhotoThreads) void shade_mask_kernel(ShadeArgs a) {
  __shared__ double es[kShadeMaxE * 6];
  const int b = blockIdx.z, tid = threadIdx.x;
  if (a.on[b] == 0) return;                                   // the same for every thread of the workgroup
  const int n = min(max(a.n_ell[b], 0), a.E);
  if (tid < n) {
    const float* e = a.ell + ((size_t)b * a.E + tid) * 5;
    double sn, cs;
    sincospi((double)e[4] / 180.0, &sn, &cs);
    es[tid * 6 + 0] = (double)e[0];
    es[tid * 6 + 1] = (double)e[1];
    es[tid * 6 + 2] = cs;
    es[tid * 6 + 3] = sn;
    es[tid * 6 + 4] = (double)e[2];
    es[tid * 6 + 5] = (double)e[3];
  }
  __syncthreads();
  const int HW = a.H * a.W, idx = (int)blockIdx.x * kPhotoThreads + tid;
  if (idx >= HW) return;
  const int y = idx / a.W, x = idx - y * a.W;
  bool in = false;
  for (int i = 0; i < n && !in; ++i) {
    const double dx = (double)x - es[i * 6], dy = (double)y - es[i * 6 + 1], cs = es[i * 6 + 2], sn = es[i * 6 + 3];
    const double u = (dx * cs + dy * sn) / es[i * 6 + 4], v = (dy * cs - dx * sn) / es[i * 6 + 5];
    in = u * u + v * v <= 1.0;
  }
  a.mask[(size_t)b * HW + idx] = in ? 255 : 0;
}

// the image's taps into LDS, padded with +0 to kpad = the next multiple of four
__device__ __forceinline__ void load_taps(const ShadeArgs& a, int b, int k, int kpad, float* taps_s, int tid) {
  for (int t = tid; t < kpad; t += kPhotoThreads) taps_s[t] = t < k ? a.taps[(size_t)b * a.Kcap + t] : 0.f;
}

// sixteen steps of four sliding sums: acc[j] += tp[tt] * win[tt + j], tt ascending
__device__ __forceinline__ void slide4(float (&acc)[4], const float4 tp, const float (&w)[8]) {
  const float t[4] = {tp.x, tp.y, tp.z, tp.w};
#pragma unroll
  for (int tt = 0; tt < 4; ++tt)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = __builtin_fmaf(t[tt], w[tt + j], acc[j]);
}

constexpr int kRowWin = kRowOut + kShadeTapSlots;    // floats of a row segment in LDS: index j + t, j < 256, t < kpad

__global__ __launch_bounds__(kPhotoThreads) void shade_rows_kernel(ShadeArgs a) {
  __shared__ __attribute__((aligned(16))) float taps_s[kShadeTapSlots];
  __shared__ __attribute__((aligned(16))) float win[kRowRows * kRowWin];
  const int b = a.b0 + (int)blockIdx.z, tid = threadIdx.x;
  if (a.on[b] == 0) return;                                   // the same for every thread of the workgroup
  const int k = a.ks[blockIdx.z], kpad = (k + 3) & ~3, rad = k >> 1;
  load_taps(a, b, k, kpad, taps_s, tid);
  const int lane = tid & 63, rr = tid >> 6;
  const int y = (int)blockIdx.y * kRowRows + rr, x0 = (int)blockIdx.x * kRowOut;
  const size_t plane = (size_t)b * a.H * a.W;
  float* w_s = win + rr * kRowWin;
  if (y < a.H) {
    const uint8_t* m = a.mask + plane + (size_t)y * a.W;
    for (int i = lane; i < kRowOut + kpad; i += 64) w_s[i] = i < kRowOut + k - 1 ? (float)m[reflect101(x0 + i - rad, a.W)] : 0.f;
  }
  __syncthreads();
  const int x = x0 + 4 * lane;
  if (y >= a.H || x >= a.W) return;
  float acc[4] = {0.f, 0.f, 0.f, 0.f}, w[8];
  const float4 first = *reinterpret_cast<const float4*>(w_s + 4 * lane);
  w[0] = first.x; w[1] = first.y; w[2] = first.z; w[3] = first.w;
  for (int t = 0; t < kpad; t += 4) {
    const float4 next = *reinterpret_cast<const float4*>(w_s + 4 * lane + t + 4);
    w[4] = next.x; w[5] = next.y; w[6] = next.z; w[7] = next.w;
    slide4(acc, *reinterpret_cast<const float4*>(taps_s + t), w);
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = w[4 + j];
  }
  float* o = a.tmp + plane + (size_t)y * a.W + x;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (x + j < a.W) o[j] = acc[j];
}

constexpr int kColWin = kColH + kShadeTapSlots;      // rows of a column tile in LDS: index j + t, j < 32, t < kpad

__global__ __launch_bounds__(kPhotoThreads) void shade_cols_kernel(ShadeArgs a) {
  __shared__ __attribute__((aligned(16))) float taps_s[kShadeTapSlots];
  __shared__ float win[kColWin * kColW];
  const int b = a.b0 + (int)blockIdx.z, tid = threadIdx.x;
  const int lx = tid & (kColW - 1), g = tid / kColW;
  const int x = (int)blockIdx.x * kColW + lx, y0 = (int)blockIdx.y * kColH;
  const size_t plane = (size_t)b * a.H * a.W;
  const uint8_t* img = a.img + plane;
  float* out = a.out + plane;
  if (a.on[b] == 0) {                                         // the same for every thread of the workgroup
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int y = y0 + 4 * g + j;
      if (y < a.H && x < a.W) out[(size_t)y * a.W + x] = (float)img[(size_t)y * a.W + x] / 255.f;
    }
    return;
  }
  const int k = a.ks[blockIdx.z], kpad = (k + 3) & ~3, rad = k >> 1;
  load_taps(a, b, k, kpad, taps_s, tid);
  const float* tmp = a.tmp + plane;
  for (int i = g; i < kColH + kpad; i += kPhotoThreads / kColW)
    win[i * kColW + lx] = (i < kColH + k - 1 && x < a.W) ? tmp[(size_t)reflect101(y0 + i - rad, a.H) * a.W + x] : 0.f;
  __syncthreads();
  if (x >= a.W || y0 + 4 * g >= a.H) return;
  float acc[4] = {0.f, 0.f, 0.f, 0.f}, w[8];
  const float* col = win + (4 * g) * kColW + lx;
#pragma unroll
  for (int j = 0; j < 4; ++j) w[j] = col[j * kColW];
  for (int t = 0; t < kpad; t += 4) {
#pragma unroll
    for (int j = 0; j < 4; ++j) w[4 + j] = col[(t + 4 + j) * kColW];
    slide4(acc, *reinterpret_cast<const float4*>(taps_s + t), w);
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = w[4 + j];
  }
  const float tr = a.transparency[b];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int y = y0 + 4 * g + j;
    if (y >= a.H) break;
    const float v = (float)img[(size_t)y * a.W + x] / 255.f * 255.f;      // img * 255 of the image / 255, as the caller of additive_shade forms it
    const float s = 1.f - tr * acc[j] / 255.f;
    out[(size_t)y * a.W + x] = fminf(fmaxf(v * s, 0.f), 255.f) / 255.f;
  }
}

inline unsigned cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }

}  // namespace

hipError_t launch_photo_pixels(const PixelArgs& a, hipStream_t s) {
  const dim3 grid(cdiv(a.W, kPhotoTileW), cdiv(a.H, kPhotoTileH), a.B);
  if (pixels_x4(a.W, a.img, a.out))
    hipLaunchKernelGGL(photo_pixels_kernel<true>, grid, dim3(kPhotoThreads), 0, s, a);
  else
    hipLaunchKernelGGL(photo_pixels_kernel<false>, grid, dim3(kPhotoThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_shade_mask(const ShadeArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(shade_mask_kernel, dim3(cdiv((long long)a.H * a.W, kPhotoThreads), 1, a.B), dim3(kPhotoThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_shade_rows(const ShadeArgs& a, int n, hipStream_t s) {
  hipLaunchKernelGGL(shade_rows_kernel, dim3(cdiv(a.W, kRowOut), cdiv(a.H, kRowRows), n), dim3(kPhotoThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_shade_cols(const ShadeArgs& a, int n, hipStream_t s) {
  hipLaunchKernelGGL(shade_cols_kernel, dim3(cdiv(a.W, kColW), cdiv(a.H, kColH), n), dim3(kPhotoThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace imx
