// sgloop.hip -- the match extraction of SuperGlue's training forward (superglue/models/superglue_train.py:276-286) from the score matrix
// and the FINAL potentials of the loss's own Sinkhorn (include/imx_sgloop.h).  Per pair, for i < m and j < n,
//
//   Z[i][j] = ((scores[i][j] + u[i]) + v[j]) - norm          the expression of otgrad.hip's gather, norm = ot_norm(m, n) (otgrad.h)
//
// is formed element by element and never stored.  Three plain launches, no workgroup waits on another, no floating-point atomics:
//
//   rows     one wave per row, lane l the columns l, l + 64, ... ascending, keeping (value, column) under a strict `>`; the 64 lanes are
//            folded by a butterfly whose combine is "the larger value, then the lower index" (sgl_better)
//   columns  32 columns per workgroup, 32 threads per column, thread r the rows r, r + 32, ... ascending (128-byte row segments), the
//            same rule; the 32 partial results are folded in LDS with the same combine
//   mutual   one workgroup per pair: the mutual test, expf of the row maximum, the strict threshold, side 1 gathered from side 0, -1 / 0
//            past the counts, the three counts against gt0
//
// The combine is associative and commutative on (finite or -inf value, index) pairs with distinct indices, so neither the fold order nor
// the partition into lanes reaches the result: among equal fp32 Z the lowest index wins, on both sides -- numpy's and torch-CPU's
// first-occurrence argmax.  A NaN never satisfies `>` and so never becomes a candidate; a row or column without a candidate (all -inf
// or NaN) reports index 0, which is in range.  The matrix is read twice and never written; offsets are 64-bit.
#include "sgloop.h"
#include "otgrad.h"
#include "train_dev.h"

namespace imx {
namespace {

constexpr int kSglRowWaves = 4;              // rows per workgroup of the row pass (one wave per row)
constexpr int kSglColTile = 32;              // columns per workgroup of the column pass, and the row-strided partial maxima per column
constexpr int kSglNone = 0x7fffffff;         // the index of "no candidate yet": loses every tie

struct SglPair {
  int m, n;
  bool ok;                                   // both sides non-empty
  float norm;
};
__device__ inline SglPair sgl_pair_of(const SglArgs& a, int b) {
  SglPair p;
  p.m = clampi(a.n0 ? a.n0[b] : a.N0, a.N0);
  p.n = clampi(a.n1 ? a.n1[b] : a.N1, a.N1);
  p.ok = p.m > 0 && p.n > 0;
  p.norm = ot_norm(p.m, p.n);
  return p;
}
// (v2, i2) beats (v1, i1): the larger value, then the lower index
__device__ inline bool sgl_better(float v2, int i2, float v1, int i1) { return v2 > v1 || (v2 == v1 && i2 < i1); }

// One wave per row i < m: row_val[i] = max_j Z[i][j] over j < n, row_idx[i] its lowest column.
__global__ __launch_bounds__(64 * kSglRowWaves) void sgl_row_kernel(SglArgs a) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const SglPair p = sgl_pair_of(a, b);
  const int i = blockIdx.x * kSglRowWaves + (threadIdx.x >> 6);
  if (!p.ok || i >= p.m) return;                                         // (no workgroup barrier below: a wave may leave)
  const float* S = a.scores + ((size_t)b * a.N0 + i) * a.N1;
  const float* vp = a.v ? a.v + (size_t)b * a.sv : nullptr;
  const float ui = a.u ? a.u[(size_t)b * a.su + i] : 0.f;
  float best = -INFINITY;
  int arg = kSglNone;
  for (int j = lane; j < p.n; j += 64) {
    const float z = ((S[j] + ui) + (vp ? vp[j] : 0.f)) - p.norm;
    if (z > best) { best = z; arg = j; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o);
    const int oi = __shfl_xor(arg, o);
    if (sgl_better(ov, oi, best, arg)) { best = ov; arg = oi; }
  }
  if (lane == 0) {
    a.row_val[(size_t)b * a.N0 + i] = best;
    a.row_idx[(size_t)b * a.N0 + i] = arg == kSglNone ? 0 : arg;
  }
}

// 32 columns per workgroup, 32 threads per column, thread r of a column taking the rows i = r, r + 32, ...:
// col_idx[j] = the lowest row of max_i Z[i][j] over i < m (the value is not kept: a mutual pair's is its row's).
__global__ __launch_bounds__(kSglColTile * kSglColTile) void sgl_col_kernel(SglArgs a) {
  __shared__ float red_v[kSglColTile][kSglColTile + 1];
  __shared__ int red_i[kSglColTile][kSglColTile + 1];
  const int b = blockIdx.y, cx = threadIdx.x % kSglColTile, ry = threadIdx.x / kSglColTile;
  const SglPair p = sgl_pair_of(a, b);
  if (!p.ok || (int)blockIdx.x * kSglColTile >= p.n) return;             // (the same for every thread of the workgroup)
  const int j = blockIdx.x * kSglColTile + cx;
  const bool live = j < p.n;
  float best = -INFINITY;
  int arg = kSglNone;
  if (live) {
    const float* S = a.scores + (size_t)b * a.N0 * a.N1 + j;
    const float* up = a.u ? a.u + (size_t)b * a.su : nullptr;
    const float vj = a.v ? a.v[(size_t)b * a.sv + j] : 0.f;
    for (int i = ry; i < p.m; i += kSglColTile) {
      const float z = ((S[(size_t)i * a.N1] + (up ? up[i] : 0.f)) + vj) - p.norm;
      if (z > best) { best = z; arg = i; }
    }
  }
  red_v[ry][cx] = best;
  red_i[ry][cx] = arg;
  __syncthreads();
  if (ry == 0 && live) {
    for (int r = 1; r < kSglColTile; ++r) {
      const float ov = red_v[r][cx];
      const int oi = red_i[r][cx];
      if (sgl_better(ov, oi, best, arg)) { best = ov; arg = oi; }
    }
    a.col_idx[(size_t)b * a.N1 + j] = arg == kSglNone ? 0 : arg;
  }
}

// One workgroup per pair.  Side 0: i and j = row_idx[i] are mutual where col_idx[j] == i; ms0 = expf(row_val[i]) there, else 0; the match
// stands where ms0 > threshold.  Side 1: j and i = col_idx[j] are mutual where row_idx[i] == j, which implies col_idx[row_idx[i]] == i, so
// ms0[i] = expf(row_val[i]) is recomputed, not read: no thread waits for another.  Past the counts -1 and 0.
__global__ __launch_bounds__(256) void sgl_mutual_kernel(SglArgs a) {
  __shared__ int cnt[3];
  const int b = blockIdx.x, t = threadIdx.x;
  const SglPair p = sgl_pair_of(a, b);
  const float* rv = a.row_val + (size_t)b * a.N0;
  const int* ri = a.row_idx + (size_t)b * a.N0;
  const int* ci = a.col_idx + (size_t)b * a.N1;
  if (t < 3) cnt[t] = 0;
  __syncthreads();
  int g = 0, q = 0, c = 0;
  for (int i = t; i < a.N0; i += 256) {
    long long mt = -1;
    float ms = 0.f;
    if (p.ok && i < p.m) {
      const int j = clampi(ri[i], p.n - 1);
      if (ci[j] == i) {
        ms = expf(rv[i]);
        if (ms > a.threshold) mt = j;
      }
      if (a.stats) {
        const long long gi = a.gt0[(size_t)b * a.N0 + i];
        g += gi >= 0;
        q += mt > -1;
        c += gi >= 0 && mt == gi;
      }
    }
    a.matches0[(size_t)b * a.N0 + i] = mt;
    a.mscores0[(size_t)b * a.N0 + i] = ms;
  }
  for (int j = t; j < a.N1; j += 256) {
    long long mt = -1;
    float ms = 0.f;
    if (p.ok && j < p.n) {
      const int i = clampi(ci[j], p.m - 1);
      if (ri[i] == j) {
        ms = expf(rv[i]);
        if (ms > a.threshold) mt = i;
      }
    }
    a.matches1[(size_t)b * a.N1 + j] = mt;
    a.mscores1[(size_t)b * a.N1 + j] = ms;
  }
  if (a.stats) {
    atomicAdd(&cnt[0], g);
    atomicAdd(&cnt[1], q);
    atomicAdd(&cnt[2], c);
    __syncthreads();
    if (t < 3) a.stats[(size_t)b * 3 + t] = cnt[t];
  }
}

}  // namespace

hipError_t launch_sgl_row_max(const SglArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(sgl_row_kernel, dim3(cdiv(a.N0, kSglRowWaves), a.B), dim3(64 * kSglRowWaves), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_sgl_col_max(const SglArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(sgl_col_kernel, dim3(cdiv(a.N1, kSglColTile), a.B), dim3(kSglColTile * kSglColTile), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_sgl_mutual(const SglArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(sgl_mutual_kernel, dim3(a.B), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace imx
