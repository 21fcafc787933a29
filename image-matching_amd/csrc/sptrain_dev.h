// sptrain_dev.h -- device helpers that kernels of more than one unit share: the warp of a label point (sptrain.hip, sploop.hip) and, of
// the sparse descriptor loss, what its forward (sptrain.hip) and its gradient (spgrad.hip) share:
// the bilinear taps of the '2d' method, the lane layout of a descriptor row, the row load, the four-tap sample and the dot product.
// One definition, so both sides form the same numbers from the same instructions.
#pragma once
#include <hip/hip_runtime.h>

namespace imx {
namespace {

// One row of warp_points' matrix product H @ (x, y, 1) (utils/utils.py:561-584) as torch's CPU product evaluates it on a processor
// with fused multiply-add: k ascending, the first product rounded, every later term fused into the running sum.  The fixtures
// the reference wrote agree with this order bit for bit (tests/sptrain_ref.py: warp_points).
__device__ __forceinline__ float warp_row(const float* __restrict__ m, float x, float y) {
#pragma clang fp contract(off)
  return fmaf(m[2], 1.0f, fmaf(m[1], y, m[0] * x));
}
// warp_points of the integer point (x, y) under the pixel-space matrix m: imx_warp_labels (sptrain.hip) and imx_warp_labels_bi
// (sploop.hip) both warp by this
__device__ __forceinline__ void warp_point(const float* __restrict__ m, float x, float y, float& wx, float& wy) {
#pragma clang fp contract(off)
  const float u = warp_row(m, x, y), v = warp_row(m + 3, x, y), w = warp_row(m + 6, x, y);
  wx = u / w;
  wy = v / w;
}

// bilinear taps of grid_sample (zero padding, align_corners=True) at normPts(p, size): g = p / size * 2 - 1, then
// ((g + 1) / 2) (size - 1), as torch forms them
struct Tap4 { int x0, y0; float nw, ne, sw, se; bool ok; };
__device__ __forceinline__ Tap4 dl_taps(int cell, int Hc, int Wc) {
#pragma clang fp contract(off)
  const int yi = cell / Wc, xi = cell - yi * Wc;
  const float gx = (float)xi / (float)Wc * 2.0f - 1.0f, gy = (float)yi / (float)Hc * 2.0f - 1.0f;
  const float ix = ((gx + 1.0f) / 2.0f) * (float)(Wc - 1), iy = ((gy + 1.0f) / 2.0f) * (float)(Hc - 1);
  Tap4 t;
  t.ok = ix > -1.0f && ix < (float)Wc && iy > -1.0f && iy < (float)Hc;
  const float fx = floorf(ix), fy = floorf(iy);
  t.x0 = t.ok ? (int)fx : 0; t.y0 = t.ok ? (int)fy : 0;
  const float ex = (fx + 1.0f) - ix, ey = (fy + 1.0f) - iy, dx = ix - fx, dy = iy - fy;
  t.nw = ex * ey; t.ne = dx * ey; t.sw = ex * dy; t.se = dx * dy;
  return t;
}

constexpr int kDlBlocks = 2;       // channel blocks of 4 LPR floats per lane: d <= 512

struct DlLane { int sub, lpr, nvec; };

__device__ __forceinline__ void dl_load(const float* __restrict__ row, const DlLane& L, float4 (&v)[kDlBlocks]) {
#pragma unroll
  for (int k = 0; k < kDlBlocks; ++k) {
    const int j = L.sub + k * L.lpr;
    v[k] = j < L.nvec ? reinterpret_cast<const float4*>(row)[j] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// the four-tap sample of one map at a cell's normPts position, this lane's channels
__device__ __forceinline__ void dl_sample(const float* __restrict__ map, const Tap4& t, int Hc, int Wc, int d, const DlLane& L, float4 (&v)[kDlBlocks]) {
#pragma unroll
  for (int k = 0; k < kDlBlocks; ++k) v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (!t.ok) return;
  const int xs[4] = {t.x0, t.x0 + 1, t.x0, t.x0 + 1}, ys[4] = {t.y0, t.y0, t.y0 + 1, t.y0 + 1};
  const float ws[4] = {t.nw, t.ne, t.sw, t.se};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (xs[q] < 0 || xs[q] >= Wc || ys[q] < 0 || ys[q] >= Hc) continue;
    float4 r[kDlBlocks];
    dl_load(map + ((size_t)ys[q] * Wc + xs[q]) * d, L, r);
#pragma unroll
    for (int k = 0; k < kDlBlocks; ++k) { v[k].x += r[k].x * ws[q]; v[k].y += r[k].y * ws[q]; v[k].z += r[k].z * ws[q]; v[k].w += r[k].w * ws[q]; }
  }
}

// this lane's channels in ascending order, then a fixed butterfly over the lanes of the row's group: every lane of it holds the sum
__device__ __forceinline__ float dl_dot(const float4 (&x)[kDlBlocks], const float4 (&y)[kDlBlocks], const DlLane& L) {
  float s = 0.0f;
#pragma unroll
  for (int k = 0; k < kDlBlocks; ++k) {
    s = fmaf(x[k].x, y[k].x, s); s = fmaf(x[k].y, y[k].y, s); s = fmaf(x[k].z, y[k].z, s); s = fmaf(x[k].w, y[k].w, s);
  }
  for (int o = L.lpr >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o);
  return s;
}

// the lane layout of one wave for descriptor rows of d floats: LPR = min(64, pow2 >= d / 4) lanes per row
__device__ __forceinline__ DlLane dl_lanes(int d, int lane) {
  DlLane L;
  L.nvec = d >> 2;
  L.lpr = 1;
  while (L.lpr < L.nvec && L.lpr < 64) L.lpr <<= 1;
  L.sub = lane & (L.lpr - 1);
  return L;
}

}  // namespace
}  // namespace imx
