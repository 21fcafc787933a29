// sppool_train.hip -- nn.MaxPool2d(2) and the descriptor normalisation of SuperPoint's training step on NCHW maps, forward and backward
// (include/imx_sppool.h).
//
//   maxpool2_fwd   grid (ceil(items / 256), C, B), an item = one output (dword form) or four outputs of one row (16-byte form).  A window
//                  is scanned (0,0), (0,1), (1,0), (1,1) from its first element, a later one taken when v > best || isnan(v): PyTorch's
//                  rule (the first maximum wins a tie, -0 before +0 stays, a NaN wins and the last NaN keeps the index).  y, and
//                  idx = 2 row + col as one byte where asked for
//   maxpool2_bwd   grid (ceil(items / 256), C, B), an item = one window position of the ceil(H/2) x ceil(W/2) cover of the map: dx = dy at
//                  the recorded element, +0 at the three others and in the trailing row / column an odd H / W leaves outside every window.
//                  A select, never a product; neither x nor y is read
//   l2norm_fwd     grid (B ceil(HW / pixels per workgroup)), 256 threads = 64 lanes along pixels x 4 waves along channels.  Wave g adds
//                  fma(x, x, acc) over the channels g, g + 4, ... ascending from +0; the four partial sums meet in LDS as
//                  ((s0 + s1) + s2) + s3; norm = sqrtf(that), y = x / norm (a true division) in a second sweep over the same channels
//   l2norm_bwd     the same structure: s = sum_c y_c dy_c in the same order, dx_c = (dy_c - y_c s) / norm
//
// The order of each channel sum is a function of C alone, so a pixel's bits depend on nothing but its own vector.  The normalisation reads
// its inputs twice: a workgroup's slice (64 or 256 pixels x C values, 64 KiB to 1 MiB) does not fit the registers for C up to 1024 without
// one kernel per channel count.  Where the second sweep is served from was not measured: at the training shape (C = 256, about 37 resident
// workgroups x 64 KiB per XCD) the slices fit L2; at C = 1024 in the 16-byte form they do not.  No floating-point atomics,
// no workgroup that waits on another, no workspace.  Loads and stores are predicated: nothing past a map's last element is touched.
// Contraction is off: every fused multiply-add is written as one.  Every offset is 64-bit.
#include "sppool_train.h"

#pragma clang fp contract(off)

namespace imx {

namespace {

// one step of the scan: element (code) of the window against the best so far
__device__ __forceinline__ void take(float v, int code, float& best, int& at) {
  if (v > best || v != v) {
    best = v;
    at = code;
  }
}
__device__ __forceinline__ void window(float v00, float v01, float v10, float v11, float& best, int& at) {
  best = v00;
  at = 0;
  take(v01, 1, best, at);
  take(v10, 2, best, at);
  take(v11, 3, best, at);
}

__device__ __forceinline__ size_t plane_of(const PoolArgs& a) { return (size_t)blockIdx.z * a.C + blockIdx.y; }

template <bool X4>
__global__ __launch_bounds__(kPoolThreads) void maxpool2_fwd_kernel(PoolArgs a) {
  const int Ho = a.H >> 1, Wo = a.W >> 1;
  const size_t plane = plane_of(a);
  const float* x = a.x + plane * ((size_t)a.H * a.W);
  const size_t out = plane * ((size_t)Ho * Wo);
  const int item = (int)blockIdx.x * kPoolThreads + (int)threadIdx.x;
  if constexpr (X4) {
    const int Wq = Wo >> 2;
    if (item >= Ho * Wq) return;
    const int r = item / Wq, q = item - r * Wq;
    const float* p = x + (size_t)(2 * r) * a.W + 8 * q;
    const float4 t0 = *reinterpret_cast<const float4*>(p), t1 = *reinterpret_cast<const float4*>(p + 4);
    const float4 u0 = *reinterpret_cast<const float4*>(p + a.W), u1 = *reinterpret_cast<const float4*>(p + a.W + 4);
    float b0, b1, b2, b3;
    int i0, i1, i2, i3;
    window(t0.x, t0.y, u0.x, u0.y, b0, i0);
    window(t0.z, t0.w, u0.z, u0.w, b1, i1);
    window(t1.x, t1.y, u1.x, u1.y, b2, i2);
    window(t1.z, t1.w, u1.z, u1.w, b3, i3);
    const size_t o = out + (size_t)r * Wo + 4 * q;
    *reinterpret_cast<float4*>(a.y + o) = make_float4(b0, b1, b2, b3);
    if (a.idx) *reinterpret_cast<uint32_t*>(a.idx + o) = (uint32_t)i0 | (uint32_t)i1 << 8 | (uint32_t)i2 << 16 | (uint32_t)i3 << 24;
  } else {
    if (item >= Ho * Wo) return;
    const int r = item / Wo, c = item - r * Wo;
    const float* p = x + (size_t)(2 * r) * a.W + 2 * c;
    float best;
    int at;
    window(p[0], p[1], p[a.W], p[a.W + 1], best, at);
    const size_t o = out + (size_t)r * Wo + c;
    a.y[o] = best;
    if (a.idx) a.idx[o] = (uint8_t)at;
  }
}

template <bool X4>
__global__ __launch_bounds__(kPoolThreads) void maxpool2_bwd_kernel(PoolArgs a) {
  const int Ho = a.H >> 1, Wo = a.W >> 1, R = (a.H + 1) >> 1;
  const size_t plane = plane_of(a);
  float* dx = a.dx + plane * ((size_t)a.H * a.W);
  const size_t in = plane * ((size_t)Ho * Wo);
  const int item = (int)blockIdx.x * kPoolThreads + (int)threadIdx.x;
  if constexpr (X4) {                                    // W % 8 == 0: no trailing column
    const int Wq = Wo >> 2;
    if (item >= R * Wq) return;
    const int r = item / Wq, q = item - r * Wq;
    float* p = dx + (size_t)(2 * r) * a.W + 8 * q;
    if (r >= Ho) {                                       // the trailing row of an odd H
      const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4*>(p) = z;
      *reinterpret_cast<float4*>(p + 4) = z;
      return;
    }
    const size_t o = in + (size_t)r * Wo + 4 * q;
    const float4 g = *reinterpret_cast<const float4*>(a.dy + o);
    const uint32_t w = *reinterpret_cast<const uint32_t*>(a.idx_in + o);
    const uint32_t i0 = w & 255u, i1 = (w >> 8) & 255u, i2 = (w >> 16) & 255u, i3 = w >> 24;
    *reinterpret_cast<float4*>(p) = make_float4(i0 == 0 ? g.x : 0.f, i0 == 1 ? g.x : 0.f, i1 == 0 ? g.y : 0.f, i1 == 1 ? g.y : 0.f);
    *reinterpret_cast<float4*>(p + 4) = make_float4(i2 == 0 ? g.z : 0.f, i2 == 1 ? g.z : 0.f, i3 == 0 ? g.w : 0.f, i3 == 1 ? g.w : 0.f);
    *reinterpret_cast<float4*>(p + a.W) = make_float4(i0 == 2 ? g.x : 0.f, i0 == 3 ? g.x : 0.f, i1 == 2 ? g.y : 0.f, i1 == 3 ? g.y : 0.f);
    *reinterpret_cast<float4*>(p + a.W + 4) = make_float4(i2 == 2 ? g.z : 0.f, i2 == 3 ? g.z : 0.f, i3 == 2 ? g.w : 0.f, i3 == 3 ? g.w : 0.f);
  } else {
    const int Cw = (a.W + 1) >> 1;
    if (item >= R * Cw) return;
    const int r = item / Cw, c = item - r * Cw;
    const bool inside = r < Ho && c < Wo;                // a window; otherwise a piece of the trailing row / column
    float g = 0.f;
    uint32_t at = 255u;
    if (inside) {
      const size_t o = in + (size_t)r * Wo + c;
      g = a.dy[o];
      at = a.idx_in[o];
    }
    float* p = dx + (size_t)(2 * r) * a.W + 2 * c;
    const bool right = 2 * c + 1 < a.W, below = 2 * r + 1 < a.H;
    p[0] = at == 0 ? g : 0.f;
    if (right) p[1] = at == 1 ? g : 0.f;
    if (below) {
      p[a.W] = at == 2 ? g : 0.f;
      if (right) p[a.W + 1] = at == 3 ? g : 0.f;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- desc / ||desc||_2

// a lane's V consecutive pixels of channel c: p points at the lane's first pixel of channel 0; pixels from `valid` on are not touched
template <int V>
__device__ __forceinline__ void load_px(const float* __restrict__ p, size_t chan, int valid, float (&v)[V]) {
  if constexpr (V == 4) {
    const float4 w = *reinterpret_cast<const float4*>(p + chan);      // valid is 4 in this form: HW % 4 == 0
    v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
  } else {
    v[0] = valid > 0 ? p[chan] : 0.f;
  }
}
template <int V>
__device__ __forceinline__ void store_px(float* __restrict__ p, size_t chan, int valid, const float (&v)[V]) {
  if constexpr (V == 4) {
    *reinterpret_cast<float4*>(p + chan) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    if (valid > 0) p[chan] = v[0];
  }
}

// the workgroup's place: image b, first pixel of the lane, how many of its V pixels exist (0 = none: the lane only keeps the barriers)
struct L2Place {
  size_t base;       // offset of (b, channel 0, first pixel) in (B,C,HW)
  size_t npos;       // offset of (b, first pixel) in (B,HW)
  int valid;
};
template <int V>
__device__ __forceinline__ L2Place l2_place(const L2Args& a, int lane) {
  const unsigned per = ((unsigned)a.HW + kL2Lanes * V - 1) / (kL2Lanes * V);      // workgroups of an image
  const unsigned b = blockIdx.x / per, chunk = blockIdx.x - b * per;
  const int first = ((int)chunk * kL2Lanes + lane) * V;
  const int left = a.HW - first;
  return L2Place{(size_t)b * a.C * (size_t)a.HW + (size_t)(left > 0 ? first : 0), (size_t)b * a.HW + (size_t)(left > 0 ? first : 0),
                 left >= V ? V : (left > 0 ? left : 0)};
}

// the four waves' partial sums of the lane's pixels, added in wave order; red: kL2Groups x kL2Lanes x V floats
template <int V>
__device__ __forceinline__ void join_groups(float (&acc)[V], float* red, int g, int lane) {
#pragma unroll
  for (int j = 0; j < V; ++j) red[(g * kL2Lanes + lane) * V + j] = acc[j];
  __syncthreads();
#pragma unroll
  for (int j = 0; j < V; ++j)
    acc[j] = ((red[lane * V + j] + red[(kL2Lanes + lane) * V + j]) + red[(2 * kL2Lanes + lane) * V + j]) + red[(3 * kL2Lanes + lane) * V + j];
}

template <int V>
__global__ __launch_bounds__(kL2Lanes * kL2Groups) void l2norm_fwd_kernel(L2Args a) {
  __shared__ float red[kL2Groups * kL2Lanes * V];
  const int lane = threadIdx.x & (kL2Lanes - 1), g = threadIdx.x / kL2Lanes;
  const L2Place pl = l2_place<V>(a, lane);
  const float* x = a.x + pl.base;
  float acc[V], v[V];
#pragma unroll
  for (int j = 0; j < V; ++j) acc[j] = 0.f;
  if (pl.valid) {
#pragma unroll 8
    for (int c = g; c < a.C; c += kL2Groups) {
      load_px<V>(x, (size_t)c * a.HW, pl.valid, v);
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] = __builtin_fmaf(v[j], v[j], acc[j]);
    }
  }
  join_groups<V>(acc, red, g, lane);
  if (!pl.valid) return;
#pragma unroll
  for (int j = 0; j < V; ++j) acc[j] = sqrtf(acc[j]);
  if (g == 0) store_px<V>(a.norm + pl.npos, 0, pl.valid, acc);
  float* y = a.y + pl.base;
#pragma unroll 8
  for (int c = g; c < a.C; c += kL2Groups) {
    load_px<V>(x, (size_t)c * a.HW, pl.valid, v);
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = v[j] / acc[j];
    store_px<V>(y, (size_t)c * a.HW, pl.valid, v);
  }
}

template <int V>
__global__ __launch_bounds__(kL2Lanes * kL2Groups) void l2norm_bwd_kernel(L2Args a) {
  __shared__ float red[kL2Groups * kL2Lanes * V];
  const int lane = threadIdx.x & (kL2Lanes - 1), g = threadIdx.x / kL2Lanes;
  const L2Place pl = l2_place<V>(a, lane);
  const float* y = a.y_in + pl.base;
  const float* dy = a.dy + pl.base;
  float acc[V], v[V], d[V];
#pragma unroll
  for (int j = 0; j < V; ++j) acc[j] = 0.f;
  if (pl.valid) {
#pragma unroll 8
    for (int c = g; c < a.C; c += kL2Groups) {
      load_px<V>(y, (size_t)c * a.HW, pl.valid, v);
      load_px<V>(dy, (size_t)c * a.HW, pl.valid, d);
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] = __builtin_fmaf(v[j], d[j], acc[j]);
    }
  }
  join_groups<V>(acc, red, g, lane);
  if (!pl.valid) return;
  float n[V];
  load_px<V>(a.norm_in + pl.npos, 0, pl.valid, n);
  float* dx = a.dx + pl.base;
#pragma unroll 8
  for (int c = g; c < a.C; c += kL2Groups) {
    load_px<V>(y, (size_t)c * a.HW, pl.valid, v);
    load_px<V>(dy, (size_t)c * a.HW, pl.valid, d);
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = (d[j] - v[j] * acc[j]) / n[j];
    store_px<V>(dx, (size_t)c * a.HW, pl.valid, v);
  }
}

inline unsigned blocks_of(long long items) { return (unsigned)((items + kPoolThreads - 1) / kPoolThreads); }
inline unsigned l2_grid(const L2Args& a, int V) { return (unsigned)a.B * (((unsigned)a.HW + kL2Lanes * V - 1) / (kL2Lanes * V)); }

}  // namespace

hipError_t launch_maxpool2_fwd(const PoolArgs& a, hipStream_t s) {
  const long long Ho = a.H / 2, Wo = a.W / 2;
  if (pool_x4(a.W, a.x, a.y, a.idx))
    hipLaunchKernelGGL(maxpool2_fwd_kernel<true>, dim3(blocks_of(Ho * (Wo / 4)), a.C, a.B), dim3(kPoolThreads), 0, s, a);
  else
    hipLaunchKernelGGL(maxpool2_fwd_kernel<false>, dim3(blocks_of(Ho * Wo), a.C, a.B), dim3(kPoolThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_maxpool2_bwd(const PoolArgs& a, hipStream_t s) {
  const long long R = (a.H + 1) / 2, Wo = a.W / 2, Cw = (a.W + 1) / 2;
  if (pool_x4(a.W, a.dx, a.dy, a.idx_in))
    hipLaunchKernelGGL(maxpool2_bwd_kernel<true>, dim3(blocks_of(R * (Wo / 4)), a.C, a.B), dim3(kPoolThreads), 0, s, a);
  else
    hipLaunchKernelGGL(maxpool2_bwd_kernel<false>, dim3(blocks_of(R * Cw), a.C, a.B), dim3(kPoolThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_l2norm_fwd(const L2Args& a, hipStream_t s) {
  if (l2_x4(a.B, a.HW, a.x, a.y, a.norm))
    hipLaunchKernelGGL(l2norm_fwd_kernel<4>, dim3(l2_grid(a, 4)), dim3(kL2Lanes * kL2Groups), 0, s, a);
  else
    hipLaunchKernelGGL(l2norm_fwd_kernel<1>, dim3(l2_grid(a, 1)), dim3(kL2Lanes * kL2Groups), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_l2norm_bwd(const L2Args& a, hipStream_t s) {
  if (l2_x4(a.B, a.HW, a.y_in, a.norm_in, a.dy, a.dx))
    hipLaunchKernelGGL(l2norm_bwd_kernel<4>, dim3(l2_grid(a, 4)), dim3(kL2Lanes * kL2Groups), 0, s, a);
  else
    hipLaunchKernelGGL(l2norm_bwd_kernel<1>, dim3(l2_grid(a, 1)), dim3(kL2Lanes * kL2Groups), 0, s, a);
  return hipGetLastError();
}

}  // namespace imx
