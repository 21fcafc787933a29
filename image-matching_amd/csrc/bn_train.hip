// bn_train.hip -- nn.BatchNorm1d followed by nn.ReLU in their training form (include/imx_train.h), one launch
// forward and one backward, no workspace.  One workgroup of 256 threads per channel c; with n[b] the pair's count and M their sum:
//
//   bn_relu_fwd   mean = sum x / M,  var = sum (x - mean)^2 / M,  rstd = 1 / sqrt(var + eps)       (training; evaluation: the running ones)
//                 xhat = (x - mean) rstd,  z = fma(xhat, gamma, beta),  y = z > 0 ? z : 0;  mean, rstd and the running statistics written
//   bn_relu_bwd   g = z > 0 ? dy : 0 (z recomputed by the same expression),  dbeta = sum g,  dgamma = sum g xhat,
//                 dx = gamma rstd (g - dbeta / M - xhat dgamma / M)                                (evaluation: dx = gamma rstd g)
//
// Summation order, fixed at compile time and a function of the counts only: thread t adds the valid columns t, t + 256, ... of pair 0
// in ascending order, then those of pair 1, and so on, into one accumulator that starts at +0; a butterfly over the 64 lanes (xor 32,
// 16, 8, 4, 2, 1: every lane ends with the same bits) gives the wave's sum, and the four waves are added in ascending order through
// LDS.  No partials in memory, no floating-point atomics, no workgroup that waits on another.  The mean is formed around a pivot (the
// channel's first valid value: column 0 of the first pair whose count is not 0), mean = pivot + sum (x - pivot) / M, and the variance in
// a second pass around the mean, so a constant channel has mean = its value and var = 0 exactly.
//
// Two forms, chosen by the launcher from the frame (bn_in_registers): with at most 16 (pair, 256-column) slots per thread the channel's
// values are loaded once and stay in registers between the passes; otherwise every pass reads them again (out of L2).  Both visit the
// same values in the same order with the same operations, so the form does not reach the bits.  The second form issues the loads of four
// columns before it uses the first (a thread's loads do not depend on its sums; the order of the sums is unchanged).  Contraction is
// off in this file: every fused multiply-add is written as one, which is what makes the mask of the backward equal y > 0 bit for bit.
// Loads are single dwords (a row of N floats is not 16-byte aligned when N % 4 != 0) and predicated: nothing past a count is ever loaded.
#include "bn_train.h"
#include "train_dev.h"

#pragma clang fp contract(off)

namespace imx {

namespace {

__device__ __forceinline__ int count_of(const BnArgs& a, int b) {
  const int v = a.n ? a.n[b] : a.N;
  return v < 0 ? 0 : v > a.N ? a.N : v;
}

// M = the sum of the counts, first = the first pair whose count is not 0 (B when there is none): integer sums, any order
__device__ __forceinline__ void channel_counts(const BnArgs& a, int t, unsigned long long* sM, int* sFirst, long long& M, int& first) {
  if (t == 0) {
    *sM = 0ull;
    *sFirst = a.B;
  }
  __syncthreads();
  unsigned long long m = 0ull;
  int f = a.B;
  for (int b = t; b < a.B; b += kBnThreads) {
    const int cnt = count_of(a, b);
    m += (unsigned long long)cnt;
    if (cnt > 0 && b < f) f = b;
  }
  if (m) atomicAdd(sM, m);
  if (f < a.B) atomicMin(sFirst, f);
  __syncthreads();
  M = (long long)*sM;
  first = *sFirst;
}

// the workgroup's sum of u, on every thread; red: four floats of LDS that nothing else uses before the next barrier
__device__ __forceinline__ float block_sum(float u, float* red, int t) {
  u = wave_sum(u);
  if ((t & 63) == 0) red[t >> 6] = u;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

struct BnPair {                               // one element's x and dy (dy only in the backward)
  float x, d;
};

constexpr int kBnAhead = 4;                   // the form that reads x again: loads of this many columns are issued before their values are used

// f(slot, pair, column, values) for the thread's columns below limit(pair) of every pair, pairs ascending, columns ascending.  REG: the
// 16 slots unrolled, so that slot indexes registers (values is not filled: f reads its registers); slots past the last pair are
// skipped.  Otherwise values = load(pair, column), four columns' loads ahead of their use; the order of the calls of f is the same.
template <bool REG, bool FULL, class L, class F>
__device__ __forceinline__ void visit(const BnArgs& a, int t, L&& load, F&& f) {
  if constexpr (REG) {
    const int per_pair = (a.N + kBnThreads - 1) / kBnThreads;
    int b = 0, k = 0;
#pragma unroll
    for (int s = 0; s < kBnSlots; ++s) {
      const int col = t + kBnThreads * k;
      if (b < a.B && col < (FULL ? a.N : count_of(a, b))) f(s, b, col, BnPair{0.f, 0.f});
      if (++k == per_pair) {
        k = 0;
        ++b;
      }
    }
  } else {
    for (int b = 0; b < a.B; ++b) {
      const int lim = FULL ? a.N : count_of(a, b);
      for (int col0 = t; col0 < lim; col0 += kBnAhead * kBnThreads) {
        BnPair v[kBnAhead];
#pragma unroll
        for (int u = 0; u < kBnAhead; ++u) {
          const int col = col0 + u * kBnThreads;
          v[u] = col < lim ? load(b, col) : BnPair{0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < kBnAhead; ++u) {
          const int col = col0 + u * kBnThreads;
          if (col < lim) f(0, b, col, v[u]);
        }
      }
    }
  }
}

__device__ __forceinline__ size_t at(const BnArgs& a, int b, int c, int col) { return ((size_t)b * a.C + c) * a.N + col; }

// the one expression of the normalised value and of the pre-activation, shared by the forward and the mask of the backward
__device__ __forceinline__ float xhat_of(float x, float mean, float rstd) { return (x - mean) * rstd; }
__device__ __forceinline__ float z_of(float xh, float gamma, float beta) { return __builtin_fmaf(xh, gamma, beta); }

template <bool REG>
__global__ __launch_bounds__(kBnThreads) void bn_relu_fwd_kernel(BnArgs a) {
  __shared__ float red[2][4];
  __shared__ unsigned long long sM;
  __shared__ int sFirst;
  const int t = threadIdx.x, c = blockIdx.x;
  long long M;
  int first;
  channel_counts(a, t, &sM, &sFirst, M, first);
  auto nothing = [](int, int) { return BnPair{0.f, 0.f}; };
  if (M == 0) {                              // block-uniform: no valid column anywhere
    visit<false, true>(a, t, nothing, [&](int, int b, int col, BnPair) { a.y[at(a, b, c, col)] = 0.f; });
    if (t == 0) {
      a.mean[c] = 0.f;
      a.rstd[c] = 0.f;
    }
    return;
  }
  const float gamma = a.gamma[c], beta = a.beta[c], Mf = (float)M;
  // x of a column, or 0 past the pair's count: nothing past a count is loaded
  auto load = [&](int b, int col) { return BnPair{col < count_of(a, b) ? a.x[at(a, b, c, col)] : 0.f, 0.f}; };
  float xv[kBnSlots];
  if constexpr (REG) {
#pragma unroll
    for (int s = 0; s < kBnSlots; ++s) xv[s] = 0.f;
    visit<true, false>(a, t, nothing, [&](int s, int b, int col, BnPair) { xv[s] = a.x[at(a, b, c, col)]; });
  }
  auto value = [&](int s, BnPair v) { return REG ? xv[s] : v.x; };
  float mean, rstd;
  if (a.train) {
    const float pivot = a.x[at(a, first, c, 0)];
    float acc = 0.f;
    visit<REG, false>(a, t, load, [&](int s, int, int, BnPair v) { acc += value(s, v) - pivot; });
    mean = pivot + block_sum(acc, red[0], t) / Mf;
    acc = 0.f;
    visit<REG, false>(a, t, load, [&](int s, int, int, BnPair v) {
      const float d = value(s, v) - mean;
      acc = __builtin_fmaf(d, d, acc);
    });
    const float var = block_sum(acc, red[1], t) / Mf;
    rstd = 1.f / sqrtf(var + a.eps);
    if (t == 0) {
      if (a.running_mean) a.running_mean[c] = (1.f - a.momentum) * a.running_mean[c] + a.momentum * mean;
      if (a.running_var && M > 1) a.running_var[c] = (1.f - a.momentum) * a.running_var[c] + a.momentum * (var * Mf / (Mf - 1.f));
      if (a.num_batches_tracked && c == 0) *a.num_batches_tracked = *a.num_batches_tracked + 1;
    }
  } else {
    mean = a.running_mean[c];
    rstd = 1.f / sqrtf(a.running_var[c] + a.eps);
  }
  if (t == 0) {
    a.mean[c] = mean;
    a.rstd[c] = rstd;
  }
  visit<REG, true>(a, t, load, [&](int s, int b, int col, BnPair v) {
    float y = 0.f;
    if (col < count_of(a, b)) {
      const float z = z_of(xhat_of(value(s, v), mean, rstd), gamma, beta);
      y = z > 0.f ? z : 0.f;
    }
    a.y[at(a, b, c, col)] = y;
  });
}

template <bool REG>
__global__ __launch_bounds__(kBnThreads) void bn_relu_bwd_kernel(BnArgs a) {
  __shared__ float red[2][4];
  __shared__ unsigned long long sM;
  __shared__ int sFirst;
  const int t = threadIdx.x, c = blockIdx.x;
  long long M;
  int first;
  channel_counts(a, t, &sM, &sFirst, M, first);
  if (M == 0) {                              // block-uniform
    if (a.dx) visit<false, true>(a, t, [](int, int) { return BnPair{0.f, 0.f}; }, [&](int, int b, int col, BnPair) { a.dx[at(a, b, c, col)] = 0.f; });
    if (t == 0) {
      if (a.dgamma) a.dgamma[c] = 0.f;
      if (a.dbeta) a.dbeta[c] = 0.f;
    }
    return;
  }
  const float gamma = a.gamma[c], beta = a.beta[c], mean = a.mean_in[c], rstd = a.rstd_in[c], Mf = (float)M;
  // x and dy of a column, or 0 past the pair's count: nothing past a count is loaded
  auto load = [&](int b, int col) {
    const size_t i = at(a, b, c, col);
    return col < count_of(a, b) ? BnPair{a.x[i], a.dy[i]} : BnPair{0.f, 0.f};
  };
  // xhat and the masked cotangent of one valid element: the mask from the forward's own expression, dy selected, never multiplied
  auto element = [&](BnPair v, float& xh, float& g) {
    xh = xhat_of(v.x, mean, rstd);
    g = z_of(xh, gamma, beta) > 0.f ? v.d : 0.f;
  };
  float hv[kBnSlots], gv[kBnSlots];
  float sb = 0.f, sg = 0.f;
  visit<REG, false>(a, t, load, [&](int s, int b, int col, BnPair v) {
    if constexpr (REG) v = load(b, col);
    float xh, g;
    element(v, xh, g);
    if constexpr (REG) {
      hv[s] = xh;
      gv[s] = g;
    }
    sb += g;
    sg = __builtin_fmaf(g, xh, sg);
  });
  sb = block_sum(sb, red[0], t);
  sg = block_sum(sg, red[1], t);
  if (t == 0) {
    if (a.dgamma) a.dgamma[c] = sg;
    if (a.dbeta) a.dbeta[c] = sb;
  }
  if (!a.dx) return;
  const float k = gamma * rstd, mb = sb / Mf, mg = sg / Mf;
  visit<REG, true>(a, t, load, [&](int s, int b, int col, BnPair v) {
    float d = 0.f;
    if (col < count_of(a, b)) {
      float xh, g;
      if constexpr (REG) {
        xh = hv[s];
        g = gv[s];
      } else {
        element(v, xh, g);
      }
      d = a.train ? k * ((g - mb) - xh * mg) : k * g;
    }
    a.dx[at(a, b, c, col)] = d;
  });
}

}  // namespace

hipError_t launch_bn_relu_fwd(const BnArgs& a, hipStream_t s) {
  if (bn_in_registers(a.B, a.N)) hipLaunchKernelGGL(bn_relu_fwd_kernel<true>, dim3(a.C), dim3(kBnThreads), 0, s, a);
  else hipLaunchKernelGGL(bn_relu_fwd_kernel<false>, dim3(a.C), dim3(kBnThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_bn_relu_bwd(const BnArgs& a, hipStream_t s) {
  if (bn_in_registers(a.B, a.N)) hipLaunchKernelGGL(bn_relu_bwd_kernel<true>, dim3(a.C), dim3(kBnThreads), 0, s, a);
  else hipLaunchKernelGGL(bn_relu_bwd_kernel<false>, dim3(a.C), dim3(kBnThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace imx
