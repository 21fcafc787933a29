// sploop.hip -- kernels of libimx_sploop.so (include/imx_sploop.h) for gfx950: what SuperPoint's training LOOP needed beyond the step's
// own layers.
//
//   labels_bi   : get_labels_bi (datasets/data_tools.py:9-34) as warpLabels(..., bilinear=True) calls it, with the 8-bit quantisation
//                 of ImgAugTransform.__call__ (utils/photometric.py:72-77) optional: three launches (fill, claim, write)
//   adam_flat   : one step of torch.optim.Adam on n contiguous floats, one launch
//
// All fp32 with contraction off, so the header's order of operations is the order of the instructions (tests/sploop_ref.py restates
// both).  No floating-point atomics: the only atomics are an integer maximum of order indices and an OR of error bits, whose results
// do not depend on arrival order.  DESIGN.md section 22.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "sploop.h"
#include "sptrain_dev.h"

namespace imx {
namespace {

// ------------------------------------------------------------------------------------------------------------- labels_bi
__global__ __launch_bounds__(256) void lb_fill_kernel(LabelsBiArgs a) {
  const size_t n = (size_t)a.B * a.H * a.W;
  if (blockIdx.x == 0 && threadIdx.x == 0 && a.flag) *a.flag = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    a.out[i] = 0.0f;
    a.owner[i] = -1;
  }
}

// the four entries of point i of image b: pixel offsets within the image (-1 = not kept) and weights; false: the point is dropped
struct Splat { int pix[4]; float w[4]; };
__device__ __forceinline__ bool lb_entries(const LabelsBiArgs& a, int b, int i, Splat& e, bool report) {
#pragma clang fp contract(off)
  const float* p = a.pts + ((size_t)b * a.Kcap + i) * 2;
  const float x = truncf(p[0]), y = truncf(p[1]);                       // .long()
  float wx, wy;
  warp_point(a.mats + (size_t)b * 9, x, y, wx, wy);
  if (!(fabsf(wx) <= 3.402823466e+38f && fabsf(wy) <= 3.402823466e+38f)) {   // NaN or infinite
    if (report && a.flag) atomicOr(a.flag, 2);
    return false;
  }
  const float qx = truncf(wx), qy = truncf(wy);                         // .long() again, toward zero
  const float rx = wx - qx, ry = wy - qy;
  const float ex = 1.0f - rx, ey = 1.0f - ry;
  const float cx[4] = {qx, qx, qx + 1.0f, qx + 1.0f}, cy[4] = {qy, qy + 1.0f, qy, qy + 1.0f};
  e.w[0] = ex * ey; e.w[1] = ex * ry; e.w[2] = rx * ey; e.w[3] = rx * ry;
  const float xm = (float)(a.W - 1), ym = (float)(a.H - 1);
  bool odd = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool keep = cx[k] >= 0.0f && cx[k] <= xm && cy[k] >= 0.0f && cy[k] <= ym;      // filter_points
    e.pix[k] = keep ? (int)cy[k] * a.W + (int)cx[k] : -1;
    odd = odd || (keep && !(e.w[k] >= 0.0f && e.w[k] <= 1.0f));
  }
  if (odd && report && a.flag) atomicOr(a.flag, 1);
  return true;
}

template <int PASS>
__global__ __launch_bounds__(256) void lb_points_kernel(LabelsBiArgs a) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  const int n = a.counts ? min(max(a.counts[b], 0), a.Kcap) : a.Kcap;
  if (i >= n) return;                                                  // rows past the count are never read
  Splat e;
  if (!lb_entries(a, b, i, e, PASS == 0)) return;
  const size_t base = (size_t)b * a.H * a.W;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (e.pix[k] < 0) continue;
    const int key = k * n + i;                                         // the entry's place in the reference's concatenation
    if (PASS == 0) {
      atomicMax(a.owner + base + e.pix[k], key);
    } else if (a.owner[base + e.pix[k]] == key) {
      float w = e.w[k];
      if (a.levels == 255) {
        float q = truncf(w * 255.0f);                                  // (img * 255).astype(np.uint8)
        q = q > 0.0f ? (q > 255.0f ? 255.0f : q) : 0.0f;               // the clamp: only for a weight outside [0,1] (flag bit 0); -0 -> +0, as a byte has no sign
        w = q / 255.0f;                                                // .astype(np.float32) / 255
      }
      a.out[base + e.pix[k]] = w;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------- adam_flat
__device__ __forceinline__ void adam_one(const AdamArgs& a, float& p, float g, float& m, float& v) {
#pragma clang fp contract(off)
  if (a.weight_decay != 0.0f) {
    const float wp = a.weight_decay * p;
    g = g + wp;
  }
  const float t1 = g - m;
  const float t2 = a.c1 * t1;
  m = m + t2;
  const float va = a.beta2 * v;
  const float vb = a.c2 * g;
  const float vc = vb * g;
  v = va + vc;
  float d = sqrtf(v) * a.inv_sqrt_bc2;                               // (default flags: sqrtf and / are correctly rounded)
  d = d + a.eps;
  float q = m / d;
  q = a.step_size * q;
  p = p - q;
}

__device__ __forceinline__ void adam_scalar(const AdamArgs& a, int64_t i) {
  float p = a.p[i], m = a.m[i], v = a.v[i];
  const float g = a.g[i];
  adam_one(a, p, g, m, v);
  a.p[i] = p; a.m[i] = m; a.v[i] = v;
  if (a.zero_grad) a.g[i] = 0.0f;
}

// X4: a thread takes the float4 at index t; the n % 4 tail elements go to the first threads of the grid as dwords
template <bool X4>
__global__ __launch_bounds__(kAdamThreads) void adam_flat_kernel(AdamArgs a) {
  const int64_t t = (int64_t)blockIdx.x * kAdamThreads + threadIdx.x;
  if (X4) {
    const int64_t n4 = a.n >> 2;
    if (t < n4) {
      float4 p = reinterpret_cast<float4*>(a.p)[t], m = reinterpret_cast<float4*>(a.m)[t], v = reinterpret_cast<float4*>(a.v)[t];
      const float4 g = reinterpret_cast<const float4*>(a.g)[t];
      adam_one(a, p.x, g.x, m.x, v.x);
      adam_one(a, p.y, g.y, m.y, v.y);
      adam_one(a, p.z, g.z, m.z, v.z);
      adam_one(a, p.w, g.w, m.w, v.w);
      reinterpret_cast<float4*>(a.p)[t] = p;
      reinterpret_cast<float4*>(a.m)[t] = m;
      reinterpret_cast<float4*>(a.v)[t] = v;
      if (a.zero_grad) reinterpret_cast<float4*>(a.g)[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const int64_t tail = (n4 << 2) + t;
    if (t < 4 && tail < a.n) adam_scalar(a, tail);
  } else if (t < a.n) {
    adam_scalar(a, t);
  }
}

}  // namespace

hipError_t launch_labels_bi(const LabelsBiArgs& a, hipStream_t s) {
  const size_t n = (size_t)a.B * a.H * a.W;
  const int fill_blocks = (int)std::min<size_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(lb_fill_kernel, dim3(fill_blocks), dim3(256), 0, s, a);
  if (a.Kcap > 0) {
    const dim3 grid((a.Kcap + 255) / 256, a.B);
    hipLaunchKernelGGL(lb_points_kernel<0>, grid, dim3(256), 0, s, a);
    hipLaunchKernelGGL(lb_points_kernel<1>, grid, dim3(256), 0, s, a);
  }
  return hipGetLastError();
}

hipError_t launch_adam_flat(const AdamArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  if (adam_x4(a)) {
    const int64_t items = std::max<int64_t>(a.n >> 2, std::min<int64_t>(a.n, 4));        // the float4s, or the threads the tail needs
    hipLaunchKernelGGL(adam_flat_kernel<true>, dim3((unsigned)((items + kAdamThreads - 1) / kAdamThreads)), dim3(kAdamThreads), 0, s, a);
  } else {
    hipLaunchKernelGGL(adam_flat_kernel<false>, dim3((unsigned)((a.n + kAdamThreads - 1) / kAdamThreads)), dim3(kAdamThreads), 0, s, a);
  }
  return hipGetLastError();
}

}  // namespace imx
