// otgrad.hip -- the SuperGlue match loss (superglue/models/superglue_train.py:267-299) through the unrolled log-domain Sinkhorn, as value
// and gradient (include/imx_train.h).  Per pair, with C the (m+1) x (n+1) coupling matrix (never materialised:
// scores inside, bin_score in the last row and column):
//
//   forward   u_t = log_mu - LSE_j(C + v_{t-1}),  v_t = log_nu - LSE_i(C + u_t),  t = 1..T, every u_t and v_t kept    (2T launches)
//   gather    loss = mean over the listed (x, y) of -logf(expf(Z[x][y])), Z = C + u_T + v_T - norm; the listings counted per row, per
//             column and per element (integer atomics; the per-element counts sit in grad until the assembly overwrites them)
//   backward  on the VECTORS only, t = T..1:  u-bar_t[i] = u-bar_in[i] - sum_j v-bar_t[j] Pc_t[i][j]   (u-bar_in = G 1 at t = T, else 0)
//                                             v-bar_{t-1}[j] = - sum_i u-bar_t[i] Pr_t[i][j]                            (2T launches)
//   assembly  C-bar[i][j] = G[i][j] - sum_{t = T..1} (v-bar_t[j] Pc_t[i][j] + u-bar_t[i] Pr_t[i][j]) in registers, one pass over the matrix
//
// Pc_t = exp(C + u_t[i] + v_t[j] - log_nu[j]) and Pr_t = exp(C + u_t[i] + v_{t-1}[j] - log_mu[i]) are recomputed from the score and the
// kept potentials wherever they are needed: the matrix is only ever read.  One plain launch per half-iteration, no workgroup waits on
// another.  No floating-point atomics: a row sum is 64 lane-strided partial sums (j ascending) folded by a butterfly, a column sum 32
// row-strided partial sums (i ascending) added in ascending order, the loss and grad_bin 256 strided partial sums and a tree -- the
// constants are compile-time, so equal inputs give equal bits whatever the batch, the padding or the workspace held before.
#include "otgrad.h"
#include "train_dev.h"

namespace imx {
namespace {

constexpr int kRowWaves = 4;                 // rows per workgroup of the row passes (one wave per row)
constexpr int kColTile = 32;                 // columns per workgroup of the column passes, and the row-strided partial sums per column
constexpr int kAsmRows = 8, kAsmWaves = 4;   // the assembly: a wave holds 8 rows x 64 columns of C-bar in registers

__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

struct Pair {
  int m, n;
  bool ok;                                   // both sides non-empty
  float alpha, norm, lmu_last, lnu_last;     // bin_score; log_mu / log_nu are norm except on the dustbin
};
__device__ inline Pair pair_of(const OtArgs& a, int b) {
  Pair p;
  p.m = clampi(a.n0 ? a.n0[b] : a.N0, 0, a.N0);
  p.n = clampi(a.n1 ? a.n1[b] : a.N1, 0, a.N1);
  p.ok = p.m > 0 && p.n > 0;
  p.alpha = *a.bin;
  p.norm = ot_norm(p.m, p.n);
  p.lmu_last = logf((float)p.n) + p.norm;
  p.lnu_last = logf((float)p.m) + p.norm;
  return p;
}
// the cotangent of one listing: gout / K
__device__ inline float weight_of(const OtArgs& a, int b) {
  const int na = clampi(a.n_all[b], 0, a.L);
  return na > 0 ? (a.gout ? a.gout[b] : 1.f) / (float)na : 0.f;
}
__device__ inline size_t urow(const OtArgs& a, int b, int t) { return ((size_t)b * (a.T + 1) + t) * (a.N0 + 1); }
__device__ inline size_t vrow(const OtArgs& a, int b, int t) { return ((size_t)b * (a.T + 1) + t) * (a.N1 + 1); }

__device__ inline float wave_max(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// ---------------------------------------------------------------------------------------------- the recorded forward
__global__ __launch_bounds__(256) void ot_zero_kernel(OtArgs a) {
  const int b = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
  if (k <= a.N0) a.U[urow(a, b, 0) + k] = 0.f;
  if (k <= a.N1) a.V[vrow(a, b, 0) + k] = 0.f;
}

// One wave per row i of C.  BWD = false: u_t[i] = log_mu[i] - LSE_j(C[i][j] + v_{t-1}[j]).
// BWD = true: u-bar_t[i] = u-bar_in[i] - sum_j v-bar_t[j] exp(((C[i][j] + u_t[i]) + v_t[j]) - log_nu[j]).
template <bool BWD>
__global__ __launch_bounds__(64 * kRowWaves) void ot_row_kernel(OtArgs a, int t) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const Pair p = pair_of(a, b);
  const int i = blockIdx.x * kRowWaves + (threadIdx.x >> 6);
  if (!p.ok || i > p.m) return;                                          // (no workgroup barrier below: a wave may leave)
  const float* S = a.scores + ((size_t)b * a.N0 + (i < p.m ? i : 0)) * a.N1;
  const bool inner = i < p.m;
  if (!BWD) {
    const float* vp = a.V + vrow(a, b, t - 1);
    float mx = -INFINITY;
    for (int j = lane; j <= p.n; j += 64) mx = fmaxf(mx, (inner && j < p.n ? S[j] : p.alpha) + vp[j]);
    mx = wave_max(mx);
    float s = 0.f;
    for (int j = lane; j <= p.n; j += 64) s += expf(((inner && j < p.n ? S[j] : p.alpha) + vp[j]) - mx);
    s = wave_sum(s);
    if (lane == 0) a.U[urow(a, b, t) + i] = (inner ? p.norm : p.lmu_last) - (mx + logf(s));
  } else {
    const float* vt = a.V + vrow(a, b, t);
    const float* vb = a.VB + vrow(a, b, t);
    const float ut = a.U[urow(a, b, t) + i];
    float acc = 0.f;
    for (int j = lane; j <= p.n; j += 64) {
      const float c = inner && j < p.n ? S[j] : p.alpha;
      acc = fmaf(vb[j], expf(((c + ut) + vt[j]) - (j < p.n ? p.norm : p.lnu_last)), acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) a.UB[urow(a, b, t) + i] = (t == a.T ? a.UB[urow(a, b, 0) + i] : 0.f) - acc;
  }
}

// 32 columns of C per workgroup, 32 threads per column, thread r of a column taking the rows i = r, r + 32, ...
// BWD = false: v_t[j] = log_nu[j] - LSE_i(C[i][j] + u_t[i]).
// BWD = true: v-bar_{t-1}[j] = - sum_i u-bar_t[i] exp(((C[i][j] + u_t[i]) + v_{t-1}[j]) - log_mu[i]).
template <bool BWD>
__global__ __launch_bounds__(kColTile * kColTile) void ot_col_kernel(OtArgs a, int t) {
  __shared__ float red[kColTile][kColTile + 1];
  const int b = blockIdx.y, cx = threadIdx.x % kColTile, ry = threadIdx.x / kColTile;
  const Pair p = pair_of(a, b);
  if (!p.ok || (int)blockIdx.x * kColTile > p.n) return;                 // (the same for every thread of the workgroup)
  const int j = blockIdx.x * kColTile + cx;
  const bool live = j <= p.n, inner = j < p.n;
  const float* S = a.scores + (size_t)b * a.N0 * a.N1 + (inner ? j : 0);
  const float* ut = a.U + urow(a, b, t);
  if (!BWD) {
    float mx = -INFINITY;
    if (live)
      for (int i = ry; i <= p.m; i += kColTile) mx = fmaxf(mx, (inner && i < p.m ? S[(size_t)i * a.N1] : p.alpha) + ut[i]);
    red[ry][cx] = mx;
    __syncthreads();
    for (int r = 0; r < kColTile; ++r) mx = fmaxf(mx, red[r][cx]);
    __syncthreads();
    float s = 0.f;
    if (live)
      for (int i = ry; i <= p.m; i += kColTile) s += expf(((inner && i < p.m ? S[(size_t)i * a.N1] : p.alpha) + ut[i]) - mx);
    red[ry][cx] = s;
    __syncthreads();
    if (ry == 0 && live) {
      float tot = 0.f;
      for (int r = 0; r < kColTile; ++r) tot += red[r][cx];
      a.V[vrow(a, b, t) + j] = (inner ? p.norm : p.lnu_last) - (mx + logf(tot));
    }
  } else {
    const float* ub = a.UB + urow(a, b, t);
    float acc = 0.f;
    if (live) {
      const float vp = a.V[vrow(a, b, t - 1) + j];
      for (int i = ry; i <= p.m; i += kColTile) {
        const float c = inner && i < p.m ? S[(size_t)i * a.N1] : p.alpha;
        acc = fmaf(ub[i], expf(((c + ut[i]) + vp) - (i < p.m ? p.norm : p.lmu_last)), acc);
      }
    }
    red[ry][cx] = acc;
    __syncthreads();
    if (ry == 0 && live) {
      float tot = 0.f;
      for (int r = 0; r < kColTile; ++r) tot += red[r][cx];
      a.VB[vrow(a, b, t - 1) + j] = -tot;
    }
  }
}

// ---------------------------------------------------------------------------------------------- the loss and the listings
// One workgroup per pair, the summation of match_loss_kernel (trainpairs.hip): each thread its columns in ascending order, then a
// fixed tree.  With grad given, every listing is counted: per row and per column of C (the seeds G 1 and G^T 1), and per element --
// inside the matrix in grad itself (as integers; the assembly reads each count before it writes the element), on the dustbin in cnt_bin.
__global__ __launch_bounds__(256) void ot_gather_kernel(OtArgs a) {
  __shared__ float part[256];
  __shared__ int bad;
  const int b = blockIdx.x, t = threadIdx.x;
  const Pair p = pair_of(a, b);
  const int na = clampi(a.n_all[b], 0, a.L);
  if (t == 0) bad = 0;
  __syncthreads();
  float acc = 0.f;
  if (p.ok && na > 0) {
    const float* uT = a.U + urow(a, b, a.T);
    const float* vT = a.V + vrow(a, b, a.T);
    const float* S = a.scores + (size_t)b * a.N0 * a.N1;
    const long long* xs = a.all_matches + (size_t)b * 2 * a.L;
    const long long* ys = xs + a.L;
    int* cr = a.cnt_row + (size_t)b * (a.N0 + 1);
    int* cc = a.cnt_col + (size_t)b * (a.N1 + 1);
    int* cb = a.cnt_bin + (size_t)b * (a.N0 + a.N1 + 1);
    int* ce = reinterpret_cast<int*>(a.grad) + (size_t)b * a.N0 * a.N1;
    for (int c = t; c < na; c += 256) {
      const long long x = xs[c], y = ys[c];
      if (x < 0 || x > p.m || y < 0 || y > p.n) {                         // outside the coupling matrix: flagged, not read, not counted
        atomicOr(&bad, kOtFlagIndex);
        continue;
      }
      const bool inner = x < p.m && y < p.n;
      const float s = inner ? S[(size_t)x * a.N1 + y] : p.alpha;
      const float z = ((s + uT[x]) + vT[y]) - p.norm;
      acc += -logf(expf(z));                                              // as written (:293): an exp that underflows makes the term +inf
      if (a.grad) {
        atomicAdd(&cr[x], 1);
        atomicAdd(&cc[y], 1);
        if (inner) atomicAdd(&ce[(size_t)x * a.N1 + y], 1);
        else atomicAdd(&cb[x == p.m ? (int)y : a.N1 + 1 + (int)x], 1);
      }
    }
  }
  part[t] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) part[t] += part[t + o];
    __syncthreads();
  }
  if (t == 0) {
    a.loss[b] = p.ok && na > 0 ? part[0] / (float)na : 0.f;
    if (a.flag) a.flag[b] = bad;
  }
}

// u-bar = G 1 (slot 0 of UB) and v-bar_T = G^T 1, G = -w (listings per element)
__global__ __launch_bounds__(256) void ot_seed_kernel(OtArgs a) {
  const int b = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
  const Pair p = pair_of(a, b);
  if (!p.ok) return;
  const float w = weight_of(a, b);
  if (k <= p.m) a.UB[urow(a, b, 0) + k] = -w * (float)a.cnt_row[(size_t)b * (a.N0 + 1) + k];
  if (k <= p.n) a.VB[vrow(a, b, a.T) + k] = -w * (float)a.cnt_col[(size_t)b * (a.N1 + 1) + k];
}

// ---------------------------------------------------------------------------------------------- the assembly of C-bar
// A workgroup covers 32 rows x 64 columns of the (N0+1) x (N1+1) frame, a wave 8 rows, a lane one column: per t the column's v_t,
// v_{t-1}, v-bar_t come in once per lane and the rows' u_t, u-bar_t are uniform over the wave.  The 2T terms of an element are
// subtracted in registers, t descending, the column term before the row term.  grad is written in full (0 past the counts); the
// dustbin row and column of C-bar go to binv.
__global__ __launch_bounds__(64 * kAsmWaves) void ot_assemble_kernel(OtArgs a) {
  const int b = blockIdx.z, lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = blockIdx.x * 64 + lane, i0 = (blockIdx.y * kAsmWaves + wave) * kAsmRows;
  const Pair p = pair_of(a, b);
  float* G = a.grad + (size_t)b * a.N0 * a.N1;
  if (!p.ok || i0 > p.m || (int)blockIdx.x * 64 > p.n) {                  // (uniform over the wave) nothing of C here: the padding is 0
    for (int r = 0; r < kAsmRows; ++r)
      if (i0 + r < a.N0 && j < a.N1) G[(size_t)(i0 + r) * a.N1 + j] = 0.f;
    return;
  }
  const float w = weight_of(a, b);
  const float* S = a.scores + (size_t)b * a.N0 * a.N1;
  const int* cb = a.cnt_bin + (size_t)b * (a.N0 + a.N1 + 1);
  const bool live = j <= p.n;
  const float lnu = j < p.n ? p.norm : p.lnu_last;
  float c[kAsmRows], acc[kAsmRows];
  for (int r = 0; r < kAsmRows; ++r) {
    const int i = i0 + r;
    c[r] = 0.f;
    acc[r] = 0.f;
    if (live && i <= p.m) {
      const bool inner = i < p.m && j < p.n;
      c[r] = inner ? S[(size_t)i * a.N1 + j] : p.alpha;
      const int cnt = inner ? reinterpret_cast<const int*>(G)[(size_t)i * a.N1 + j] : cb[i == p.m ? j : a.N1 + 1 + i];
      acc[r] = -w * (float)cnt;
    }
  }
  float vt = live && a.T > 0 ? a.V[vrow(a, b, a.T) + j] : 0.f;
  for (int t = a.T; t >= 1; --t) {
    const float vtm = live ? a.V[vrow(a, b, t - 1) + j] : 0.f;
    const float vbt = live ? a.VB[vrow(a, b, t) + j] : 0.f;
    const float* ut = a.U + urow(a, b, t) + i0;
    const float* ubt = a.UB + urow(a, b, t) + i0;
#pragma unroll
    for (int r = 0; r < kAsmRows; ++r) {
      if (i0 + r <= p.m) {                                                // (uniform over the wave)
        const float cu = c[r] + ut[r];
        acc[r] -= vbt * expf((cu + vt) - lnu);
        acc[r] -= ubt[r] * expf((cu + vtm) - (i0 + r < p.m ? p.norm : p.lmu_last));
      }
    }
    vt = vtm;
  }
  float* bv = a.binv + (size_t)b * (a.N0 + a.N1 + 1);
  for (int r = 0; r < kAsmRows; ++r) {
    const int i = i0 + r;
    if (i < a.N0 && j < a.N1) G[(size_t)i * a.N1 + j] = i < p.m && j < p.n ? acc[r] : 0.f;
    if (live && i == p.m) bv[j] = acc[r];
    else if (j == p.n && i < p.m) bv[a.N1 + 1 + i] = acc[r];
  }
}

// grad_bin = the sum of C-bar over the dustbin row (j ascending, the corner last) and then the dustbin column (i ascending)
__global__ __launch_bounds__(256) void ot_bin_kernel(OtArgs a) {
  __shared__ float part[256];
  const int b = blockIdx.x, t = threadIdx.x;
  const Pair p = pair_of(a, b);
  const float* bv = a.binv + (size_t)b * (a.N0 + a.N1 + 1);
  float acc = 0.f;
  if (p.ok)
    for (int k = t; k < p.n + 1 + p.m; k += 256) acc += bv[k <= p.n ? k : a.N1 + 1 + (k - p.n - 1)];
  part[t] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) part[t] += part[t + o];
    __syncthreads();
  }
  if (t == 0) a.grad_bin[b] = part[0];
}

}  // namespace

hipError_t launch_ot_init(const OtArgs& a, hipStream_t s) {
  const int len = (a.N0 > a.N1 ? a.N0 : a.N1) + 1;
  hipLaunchKernelGGL(ot_zero_kernel, dim3(cdiv(len, 256), a.B), dim3(256), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !a.grad) return e;
  // cnt_row | cnt_col | cnt_bin are one allocation, in this order
  e = hipMemsetAsync(a.cnt_row, 0, (size_t)a.B * 2 * (a.N0 + a.N1 + 1) * sizeof(int) + (size_t)a.B * sizeof(int), s);
  if (e != hipSuccess) return e;
  return hipMemsetAsync(a.grad, 0, (size_t)a.B * a.N0 * a.N1 * sizeof(float), s);
}

hipError_t launch_ot_row_lse(const OtArgs& a, int t, hipStream_t s) {
  hipLaunchKernelGGL(ot_row_kernel<false>, dim3(cdiv(a.N0 + 1, kRowWaves), a.B), dim3(64 * kRowWaves), 0, s, a, t);
  return hipGetLastError();
}
hipError_t launch_ot_col_lse(const OtArgs& a, int t, hipStream_t s) {
  hipLaunchKernelGGL(ot_col_kernel<false>, dim3(cdiv(a.N1 + 1, kColTile), a.B), dim3(kColTile * kColTile), 0, s, a, t);
  return hipGetLastError();
}
hipError_t launch_ot_gather(const OtArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(ot_gather_kernel, dim3(a.B), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_ot_seed(const OtArgs& a, hipStream_t s) {
  const int len = (a.N0 > a.N1 ? a.N0 : a.N1) + 1;
  hipLaunchKernelGGL(ot_seed_kernel, dim3(cdiv(len, 256), a.B), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_ot_row_bwd(const OtArgs& a, int t, hipStream_t s) {
  hipLaunchKernelGGL(ot_row_kernel<true>, dim3(cdiv(a.N0 + 1, kRowWaves), a.B), dim3(64 * kRowWaves), 0, s, a, t);
  return hipGetLastError();
}
hipError_t launch_ot_col_bwd(const OtArgs& a, int t, hipStream_t s) {
  hipLaunchKernelGGL(ot_col_kernel<true>, dim3(cdiv(a.N1 + 1, kColTile), a.B), dim3(kColTile * kColTile), 0, s, a, t);
  return hipGetLastError();
}
hipError_t launch_ot_assemble(const OtArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(ot_assemble_kernel, dim3(cdiv(a.N1 + 1, 64), cdiv(a.N0 + 1, kAsmRows * kAsmWaves), a.B), dim3(64 * kAsmWaves), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_ot_bin(const OtArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(ot_bin_kernel, dim3(a.B), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace imx
