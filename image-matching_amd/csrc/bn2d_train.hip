// bn2d_train.hip -- nn.BatchNorm2d, optionally followed by nn.ReLU, in its training form on NCHW maps (include/imx_spnorm.h; DESIGN.md
// section 19), the work split over pixels.  A map is its flat run of HW pixels; a slab is kBn2dSlab = 4096 consecutive pixels of one
// (image, channel), one workgroup of 256 threads.  With M = B HW:
//
//   forward    mean = sum x / M,  var = sum (x - mean)^2 / M,  rstd = 1 / sqrt(var + eps)            (training; evaluation: the running ones)
//              xhat = (x - mean) rstd,  z = fma(xhat, gamma, beta),  y = relu ? (z > 0 ? z : 0) : z
//   backward   g = relu ? (z > 0 ? dy : 0) : dy (z recomputed by the same expression),  dbeta = sum g,  dgamma = sum g xhat,
//              dx = gamma rstd (g - dbeta / M - xhat dgamma / M)                                      (evaluation: dx = gamma rstd g)
//
//   bn2d_stats         grid (slabs, C, B): the slab is loaded once into 16 registers per thread; mean_slab = pivot + sum (x - pivot) / n
//                      around the slab's first pixel, M2_slab = sum (x - mean_slab)^2 from the registers; (mean_slab, M2_slab) to part
//   bn2d_finalize      grid C, one wave: the pairwise update  d = mean_b - mean_a, mean = mean_a + d n_b / n, M2 = M2_a + M2_b +
//                      d^2 n_a n_b / n  in float64, over the slabs of an image ascending, then over the images ascending
//   bn2d_apply         grid (slabs, C, B): y
//   bn2d_bwd_sums      grid (slabs, C, B): (sum g, sum g xhat) of the slab to part
//   bn2d_bwd_finalize  grid C, one wave: float64 sums of the slabs of an image ascending, then of the images ascending, rounded once
//   bn2d_bwd_dx        grid (slabs, C, B): dx
//
// Summation order, fixed at compile time and a function of (B, C, HW) only: thread t of a slab holds the quads 1024 k + 4 t + j, k = 0..3,
// j = 0..3, and adds its valid values with k ascending, then j ascending, into one accumulator that starts at +0; a butterfly over the 64
// lanes (xor 32, 16, 8, 4, 2, 1) gives the wave's sum and the four waves are added in ascending order through LDS, as block_sum of
// bn_train.hip does.  A finalize lane combines the slabs of one image ascending, starting from slab 0's partial itself; lane 0 then
// combines the images ascending, starting from image 0's.  No floating-point atomics, no workgroup that waits on another.  A constant
// channel has x - pivot = 0 and d = 0 everywhere, so mean = its value and var = 0 exactly.
//
// Two load forms (bn2d_x4): when every map's run starts on a 16-byte boundary a quad is one 16-byte load or store, otherwise four dwords.
// The values, their registers and every operation on them are the same, so the form does not reach the bits.  Loads and stores are
// predicated: nothing past a map's last pixel is touched.  Contraction is off in this file: every fused multiply-add is written as one,
// which is what makes the mask of the backward equal y > 0 bit for bit.  Every offset is 64-bit.
#include "bn2d_train.h"
#include "train_dev.h"

#pragma clang fp contract(off)

namespace imx {

namespace {

constexpr int kQuads = kBn2dSlab / (4 * kBn2dThreads);      // quads of a thread: 4
constexpr int kVals = 4 * kQuads;                            // values of a thread: 16

// the workgroup's sum of u, on every thread; red: four floats of LDS that nothing else uses before the next barrier
__device__ __forceinline__ float block_sum(float u, float* red, int t) {
  u = wave_sum(u);
  if ((t & 63) == 0) red[t >> 6] = u;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// the one expression of the normalised value and of the pre-activation, shared by the forward and the mask of the backward
__device__ __forceinline__ float xhat_of(float x, float mean, float rstd) { return (x - mean) * rstd; }
__device__ __forceinline__ float z_of(float xh, float gamma, float beta) { return __builtin_fmaf(xh, gamma, beta); }

struct Slab {
  size_t base;      // offset of the slab's first pixel in (B,C,HW)
  int n;            // its pixels: kBn2dSlab, fewer in a map's last slab
};
__device__ __forceinline__ Slab slab_of(const Bn2dArgs& a) {
  const int first = (int)blockIdx.x * kBn2dSlab;
  const int rest = a.HW - first;
  return Slab{((size_t)blockIdx.z * a.C + blockIdx.y) * (size_t)a.HW + (size_t)first, rest < kBn2dSlab ? rest : kBn2dSlab};
}
// slab pixel of value i = 4 k + j of thread t
__device__ __forceinline__ int pixel_of(int t, int i) { return 4 * kBn2dThreads * (i >> 2) + 4 * t + (i & 3); }

// v[4 k + j] = p[1024 k + 4 t + j] where that pixel is below n, else 0.  X4: n % 4 == 0 and p is 16-byte aligned, so a quad is valid or
// invalid as a whole
template <bool X4>
__device__ __forceinline__ void load_slab(const float* __restrict__ p, int n, int t, float (&v)[kVals]) {
#pragma unroll
  for (int k = 0; k < kQuads; ++k) {
    const int q = pixel_of(t, 4 * k);
    if constexpr (X4) {
      float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
      if (q < n) w = *reinterpret_cast<const float4*>(p + q);
      v[4 * k] = w.x; v[4 * k + 1] = w.y; v[4 * k + 2] = w.z; v[4 * k + 3] = w.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[4 * k + j] = q + j < n ? p[q + j] : 0.f;
    }
  }
}

template <bool X4>
__device__ __forceinline__ void store_slab(float* __restrict__ p, int n, int t, const float (&v)[kVals]) {
#pragma unroll
  for (int k = 0; k < kQuads; ++k) {
    const int q = pixel_of(t, 4 * k);
    if constexpr (X4) {
      if (q < n) *reinterpret_cast<float4*>(p + q) = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (q + j < n) p[q + j] = v[4 * k + j];
    }
  }
}

template <bool X4>
__global__ __launch_bounds__(kBn2dThreads) void bn2d_stats_kernel(Bn2dArgs a) {
  __shared__ float red[2][4];
  const int t = threadIdx.x;
  const Slab sl = slab_of(a);
  const float* p = a.x + sl.base;
  float v[kVals];
  load_slab<X4>(p, sl.n, t, v);
  const float pivot = p[0], nf = (float)sl.n;
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < kVals; ++i)
    if (pixel_of(t, i) < sl.n) acc += v[i] - pivot;
  const float mean = pivot + block_sum(acc, red[0], t) / nf;
  acc = 0.f;
#pragma unroll
  for (int i = 0; i < kVals; ++i)
    if (pixel_of(t, i) < sl.n) {
      const float d = v[i] - mean;
      acc = __builtin_fmaf(d, d, acc);
    }
  const float m2 = block_sum(acc, red[1], t);
  if (t == 0) {
    float* o = a.part + 2 * ((((size_t)blockIdx.y * a.B + blockIdx.z) * gridDim.x) + blockIdx.x);
    o[0] = mean;
    o[1] = m2;
  }
}

// pixels of slab s of a map of HW pixels
__device__ __forceinline__ double slab_count(int HW, int s) {
  const int rest = HW - s * kBn2dSlab;
  return (double)(rest < kBn2dSlab ? rest : kBn2dSlab);
}
// (n, mean, M2) of a set joined with those of the set that follows it
__device__ __forceinline__ void join(double& n, double& mean, double& M2, double nb, double mb, double qb) {
  const double tot = n + nb, d = mb - mean;
  mean = mean + d * nb / tot;
  M2 = M2 + qb + d * d * n * nb / tot;
  n = tot;
}

__global__ __launch_bounds__(kBn2dFinal) void bn2d_finalize_kernel(Bn2dArgs a) {
  __shared__ double smean[kBn2dFinal], sm2[kBn2dFinal];
  const int c = blockIdx.x, l = threadIdx.x, S = bn2d_slabs(a.HW);
  double n = 0., mean = 0., M2 = 0.;                   // lane 0: the images so far
  for (int b0 = 0; b0 < a.B; b0 += kBn2dFinal) {
    const int b = b0 + l;
    if (b < a.B) {                                     // the slabs of image b, ascending
      const float* p = a.part + 2 * (((size_t)c * a.B + b) * S);
      double ni = slab_count(a.HW, 0), mi = (double)p[0], qi = (double)p[1];
      for (int s = 1; s < S; ++s) join(ni, mi, qi, slab_count(a.HW, s), (double)p[2 * s], (double)p[2 * s + 1]);
      smean[l] = mi;
      sm2[l] = qi;
    }
    __syncthreads();
    if (l == 0) {                                      // the images of this group, ascending
      const int cnt = a.B - b0 < kBn2dFinal ? a.B - b0 : kBn2dFinal;
      for (int i = 0; i < cnt; ++i) {
        if (b0 + i == 0) {
          n = (double)a.HW; mean = smean[0]; M2 = sm2[0];
        } else {
          join(n, mean, M2, (double)a.HW, smean[i], sm2[i]);
        }
      }
    }
    __syncthreads();
  }
  if (l == 0) {
    const double var = M2 / n;
    const float meanf = (float)mean, varf = (float)var;
    a.mean[c] = meanf;
    a.rstd[c] = 1.f / sqrtf(varf + a.eps);
    if (a.running_mean) a.running_mean[c] = (1.f - a.momentum) * a.running_mean[c] + a.momentum * meanf;
    if (a.running_var) a.running_var[c] = (1.f - a.momentum) * a.running_var[c] + a.momentum * (float)(var * n / (n - 1.));
    if (a.num_batches_tracked && c == 0) *a.num_batches_tracked = *a.num_batches_tracked + 1;
  }
}

template <bool X4>
__global__ __launch_bounds__(kBn2dThreads) void bn2d_apply_kernel(Bn2dArgs a) {
  const int t = threadIdx.x, c = blockIdx.y;
  const Slab sl = slab_of(a);
  float v[kVals];
  load_slab<X4>(a.x + sl.base, sl.n, t, v);
  float mean, rstd;
  if (a.train) {
    mean = a.mean[c];
    rstd = a.rstd[c];
  } else {
    mean = a.running_mean[c];
    rstd = 1.f / sqrtf(a.running_var[c] + a.eps);
    if (t == 0 && blockIdx.x == 0 && blockIdx.z == 0) {
      a.mean[c] = mean;
      a.rstd[c] = rstd;
    }
  }
  const float gamma = a.gamma[c], beta = a.beta[c];
#pragma unroll
  for (int i = 0; i < kVals; ++i) {
    const float z = z_of(xhat_of(v[i], mean, rstd), gamma, beta);
    v[i] = a.relu ? (z > 0.f ? z : 0.f) : z;
  }
  store_slab<X4>(a.y + sl.base, sl.n, t, v);
}

// xhat and the masked cotangent of one element: the mask from the forward's own expression, dy selected, never multiplied
__device__ __forceinline__ void element(const Bn2dArgs& a, float x, float dy, float mean, float rstd, float gamma, float beta, float& xh, float& g) {
  xh = xhat_of(x, mean, rstd);
  g = a.relu ? (z_of(xh, gamma, beta) > 0.f ? dy : 0.f) : dy;
}

template <bool X4>
__global__ __launch_bounds__(kBn2dThreads) void bn2d_bwd_sums_kernel(Bn2dArgs a) {
  __shared__ float red[2][4];
  const int t = threadIdx.x, c = blockIdx.y;
  const Slab sl = slab_of(a);
  float v[kVals], d[kVals];
  load_slab<X4>(a.x + sl.base, sl.n, t, v);
  load_slab<X4>(a.dy + sl.base, sl.n, t, d);
  const float gamma = a.gamma[c], beta = a.beta[c], mean = a.mean_in[c], rstd = a.rstd_in[c];
  float sb = 0.f, sg = 0.f;
#pragma unroll
  for (int i = 0; i < kVals; ++i)
    if (pixel_of(t, i) < sl.n) {
      float xh, g;
      element(a, v[i], d[i], mean, rstd, gamma, beta, xh, g);
      sb += g;
      sg = __builtin_fmaf(g, xh, sg);
    }
  sb = block_sum(sb, red[0], t);
  sg = block_sum(sg, red[1], t);
  if (t == 0) {
    float* o = a.part + 2 * ((((size_t)c * a.B + blockIdx.z) * gridDim.x) + blockIdx.x);
    o[0] = sb;
    o[1] = sg;
  }
}

__global__ __launch_bounds__(kBn2dFinal) void bn2d_bwd_finalize_kernel(Bn2dArgs a) {
  __shared__ double sbeta[kBn2dFinal], sgamma[kBn2dFinal];
  const int c = blockIdx.x, l = threadIdx.x, S = bn2d_slabs(a.HW);
  float* mine = a.part + 2 * ((size_t)c * a.B * S);     // the channel's partials
  double tb = 0., tg = 0.;                              // lane 0: the images so far
  for (int b0 = 0; b0 < a.B; b0 += kBn2dFinal) {
    const int b = b0 + l;
    if (b < a.B) {                                      // the slabs of image b, ascending
      const float* p = mine + 2 * ((size_t)b * S);
      double ub = (double)p[0], ug = (double)p[1];
      for (int s = 1; s < S; ++s) {
        ub += (double)p[2 * s];
        ug += (double)p[2 * s + 1];
      }
      sbeta[l] = ub;
      sgamma[l] = ug;
    }
    __syncthreads();
    if (l == 0) {                                       // the images of this group, ascending
      const int cnt = a.B - b0 < kBn2dFinal ? a.B - b0 : kBn2dFinal;
      for (int i = 0; i < cnt; ++i) {
        if (b0 + i == 0) {
          tb = sbeta[0]; tg = sgamma[0];
        } else {
          tb += sbeta[i]; tg += sgamma[i];
        }
      }
    }
    __syncthreads();
  }
  if (l == 0) {                                         // every partial of the channel has been read: its first pair now carries the totals
    const float fb = (float)tb, fg = (float)tg;
    mine[0] = fb;
    mine[1] = fg;
    if (a.dbeta) a.dbeta[c] = fb;
    if (a.dgamma) a.dgamma[c] = fg;
  }
}

template <bool X4>
__global__ __launch_bounds__(kBn2dThreads) void bn2d_bwd_dx_kernel(Bn2dArgs a) {
  const int t = threadIdx.x, c = blockIdx.y;
  const Slab sl = slab_of(a);
  float v[kVals], d[kVals];
  load_slab<X4>(a.x + sl.base, sl.n, t, v);
  load_slab<X4>(a.dy + sl.base, sl.n, t, d);
  const float gamma = a.gamma[c], beta = a.beta[c], mean = a.mean_in[c], rstd = a.rstd_in[c];
  const float k = gamma * rstd;
  float mb = 0.f, mg = 0.f;
  if (a.train) {
    const float* tot = a.part + 2 * ((size_t)c * a.B * gridDim.x);
    const float Mf = (float)((long long)a.B * a.HW);
    mb = tot[0] / Mf;
    mg = tot[1] / Mf;
  }
#pragma unroll
  for (int i = 0; i < kVals; ++i) {
    float xh, g;
    element(a, v[i], d[i], mean, rstd, gamma, beta, xh, g);
    v[i] = a.train ? k * ((g - mb) - xh * mg) : k * g;
  }
  store_slab<X4>(a.dx + sl.base, sl.n, t, v);
}

dim3 slab_grid(const Bn2dArgs& a) { return dim3(bn2d_slabs(a.HW), a.C, a.B); }

}  // namespace

hipError_t launch_bn2d_stats(const Bn2dArgs& a, hipStream_t s) {
  if (bn2d_x4(a.HW, a.x)) hipLaunchKernelGGL(bn2d_stats_kernel<true>, slab_grid(a), dim3(kBn2dThreads), 0, s, a);
  else hipLaunchKernelGGL(bn2d_stats_kernel<false>, slab_grid(a), dim3(kBn2dThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_bn2d_finalize(const Bn2dArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(bn2d_finalize_kernel, dim3(a.C), dim3(kBn2dFinal), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_bn2d_apply(const Bn2dArgs& a, hipStream_t s) {
  if (bn2d_x4(a.HW, a.x, a.y)) hipLaunchKernelGGL(bn2d_apply_kernel<true>, slab_grid(a), dim3(kBn2dThreads), 0, s, a);
  else hipLaunchKernelGGL(bn2d_apply_kernel<false>, slab_grid(a), dim3(kBn2dThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_bn2d_bwd_sums(const Bn2dArgs& a, hipStream_t s) {
  if (bn2d_x4(a.HW, a.x, a.dy)) hipLaunchKernelGGL(bn2d_bwd_sums_kernel<true>, slab_grid(a), dim3(kBn2dThreads), 0, s, a);
  else hipLaunchKernelGGL(bn2d_bwd_sums_kernel<false>, slab_grid(a), dim3(kBn2dThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_bn2d_bwd_finalize(const Bn2dArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(bn2d_bwd_finalize_kernel, dim3(a.C), dim3(kBn2dFinal), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_bn2d_bwd_dx(const Bn2dArgs& a, hipStream_t s) {
  if (bn2d_x4(a.HW, a.x, a.dy, a.dx)) hipLaunchKernelGGL(bn2d_bwd_dx_kernel<true>, slab_grid(a), dim3(kBn2dThreads), 0, s, a);
  else hipLaunchKernelGGL(bn2d_bwd_dx_kernel<false>, slab_grid(a), dim3(kBn2dThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace imx
