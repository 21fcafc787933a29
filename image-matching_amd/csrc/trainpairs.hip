// SuperGlue training pairs (datasets/GlueSparse.py:24-104, superglue/models/superglue_train.py:289-299) for gfx950:
//
//   warp_perspective_u8 : cv2.warpPerspective(image, M, (W,H)), INTER_LINEAR, constant border 0      GlueSparse.py:32
//   gt_project / gt_nearest / gt_assign : cv2.perspectiveTransform, cdist, the two argmins and the set operations
//                                         that build `matches` and `all_matches`                      GlueSparse.py:64-82
//   match_loss          : mean over the columns of -log(exp(Z[x][y])) on the last forward's transport matrix, and
//                         the precision / recall counts                                               superglue_train.py:289-299
//
// OpenCV is a third-party dependency absent from the reference tree: the warp and the projection follow its published
// algorithms (restated in tests/trainpairs_ref.py; parity with cv2 itself is unpinned).  All coordinate
// arithmetic is exactly-rounded double with contraction off, the interpolation is integer: the kernels are bit-exact twins of
// the restatement.  Nothing here uses atomics on an output: every order is fixed.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "imx_kernels.h"

namespace imx {
namespace {

__device__ __forceinline__ int sat_int(double v) { return (int)rint(fmin(fmax(v, -2147483648.0), 2147483647.0)); }

// One destination pixel per thread.  Source coordinates in fixed point with 5 fractional bits (INTER_BITS), the four
// bilinear weights as integers of 15 fractional bits (INTER_REMAP_COEF_BITS): (32 - a)(32 - b) 32 and so on, which are exact and
// sum to 2^15, so the rounded shift is the whole interpolation.
__global__ __launch_bounds__(256) void warp_perspective_u8_kernel(const uint8_t* __restrict__ src, long sstride,
                                                                  const double* __restrict__ minv, uint8_t* __restrict__ dst,
                                                                  int H, int W) {
#pragma clang fp contract(off)      // OpenCV's host arithmetic has no fused multiply-add: keep every rounding
  const int x = blockIdx.x * 64 + (threadIdx.x & 63);
  const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= W || y >= H) return;
  const int b = blockIdx.z;
  const double* m = minv + (size_t)b * 9;
  const uint8_t* im = src + (size_t)b * sstride;
  const double xd = (double)x, yd = (double)y;
  const double w = m[6] * xd + m[7] * yd + m[8];
  const double sc = w != 0.0 ? 32.0 / w : 0.0;
  const int X = sat_int((m[0] * xd + m[1] * yd + m[2]) * sc);
  const int Y = sat_int((m[3] * xd + m[4] * yd + m[5]) * sc);
  const int ix = X >> 5, iy = Y >> 5;                       // arithmetic shifts: floor
  const int fx = X & 31, fy = Y & 31;
  auto px = [&](int yy, int xx) -> int {
    if ((unsigned)yy >= (unsigned)H || (unsigned)xx >= (unsigned)W) return 0;
    return im[(size_t)yy * W + xx];
  };
  const int acc = px(iy, ix) * ((32 - fy) * (32 - fx) * 32) + px(iy, ix + 1) * ((32 - fy) * fx * 32) +
                  px(iy + 1, ix) * (fy * (32 - fx) * 32) + px(iy + 1, ix + 1) * (fy * fx * 32);
  const int v = (acc + (1 << 14)) >> 15;
  dst[((size_t)b * H + y) * W + x] = (uint8_t)min(max(v, 0), 255);
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// cv2.perspectiveTransform on float32 points with a double matrix: one point per thread, rows past the count are not read
__global__ __launch_bounds__(256) void gt_project_kernel(GtArgs a) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  const int n0 = clampi(a.n0 ? a.n0[b] : a.N0, 0, a.N0);
  if (i >= n0) return;
  const double* m = a.m + (size_t)b * 9;
  const double x = (double)a.kpts0[((size_t)b * a.N0 + i) * 2], y = (double)a.kpts0[((size_t)b * a.N0 + i) * 2 + 1];
  double w = x * m[6] + y * m[7] + m[8];
  w = fabs(w) > 2.220446049250313e-16 ? 1.0 / w : 0.0;
  const float px = (float)((x * m[0] + y * m[1] + m[2]) * w), py = (float)((x * m[3] + y * m[4] + m[5]) * w);
  a.proj[((size_t)b * a.N0 + i) * 2] = px;
  a.proj[((size_t)b * a.N0 + i) * 2 + 1] = py;
  if (a.proj_out) {
    a.proj_out[((size_t)b * a.N0 + i) * 2] = px;
    a.proj_out[((size_t)b * a.N0 + i) * 2 + 1] = py;
  }
}

// numpy's argmin over one line of cdist's matrix: each thread owns one point of its side, the opposite side passes through LDS in
// tiles of 256 points, candidates in ascending index under a strict `<` (the lowest index wins among equal distances).
// blockIdx.z = 0: every projected point of side 0 against side 1 (also keeps the distance); 1: every point of side 1 against them.
__global__ __launch_bounds__(256) void gt_nearest_kernel(GtArgs a) {
#pragma clang fp contract(off)
  __shared__ float tx[256], ty[256];
  const int b = blockIdx.y, dir = blockIdx.z;
  const int n0 = clampi(a.n0 ? a.n0[b] : a.N0, 0, a.N0), n1 = clampi(a.n1 ? a.n1[b] : a.N1, 0, a.N1);
  const int nq = dir ? n1 : n0, no = dir ? n0 : n1;
  if ((int)blockIdx.x * 256 >= nq) return;                  // (uniform over the workgroup)
  const float* q = dir ? a.kpts1 + (size_t)b * a.N1 * 2 : a.proj + (size_t)b * a.N0 * 2;
  const float* o = dir ? a.proj + (size_t)b * a.N0 * 2 : a.kpts1 + (size_t)b * a.N1 * 2;
  const int i = blockIdx.x * 256 + threadIdx.x;
  double qx = 0.0, qy = 0.0;
  if (i < nq) { qx = (double)q[(size_t)i * 2]; qy = (double)q[(size_t)i * 2 + 1]; }
  double best = INFINITY;
  int bi = 0;
  for (int t0 = 0; t0 < no; t0 += 256) {
    const int c = t0 + threadIdx.x;
    if (c < no) { tx[threadIdx.x] = o[(size_t)c * 2]; ty[threadIdx.x] = o[(size_t)c * 2 + 1]; }
    __syncthreads();
    const int cnt = min(256, no - t0);
    if (i < nq) {
      for (int k = 0; k < cnt; ++k) {
        // (cdist sums the squares from the first coordinate on; the sign of a difference does not reach its square, so both
        // directions see the same value for a pair)
        const double dx = qx - (double)tx[k], dy = qy - (double)ty[k];
        const double d = sqrt(dx * dx + dy * dy);
        if (d < best) { best = d; bi = t0 + k; }
      }
    }
    __syncthreads();
  }
  if (i >= nq) return;
  if (dir) {
    a.nn1[(size_t)b * a.N1 + i] = bi;
  } else {
    a.nn0[(size_t)b * a.N0 + i] = bi;
    a.d0[(size_t)b * a.N0 + i] = best;
  }
}

// exclusive prefix count of a 0/1 flag over a 256-thread workgroup, in thread order; `total` receives the workgroup's sum.
// wsum: 4 words of LDS.  Every thread of the workgroup calls it.
__device__ __forceinline__ int block_rank(bool flag, int* wsum, int& total) {
  const unsigned long long mask = __ballot(flag);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int within = __popcll(mask & ((1ull << lane) - 1ull));
  __syncthreads();                                            // (the previous round's readers are done with wsum)
  if (lane == 0) wsum[wv] = __popcll(mask);
  __syncthreads();
  int before = 0;
  total = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k < wv) before += wsum[k];
    total += wsum[k];
  }
  return before + within;
}

// One workgroup per pair: the mutual test and the three runs of columns, each placed by a prefix count in index order.
__global__ __launch_bounds__(256) void gt_assign_kernel(GtArgs a) {
  __shared__ int wsum[4];
  const int b = blockIdx.x, t = threadIdx.x;
  const int n0 = clampi(a.n0 ? a.n0[b] : a.N0, 0, a.N0), n1 = clampi(a.n1 ? a.n1[b] : a.N1, 0, a.N1);
  const int L = a.N0 + a.N1;
  long long* gt0 = a.gt0 + (size_t)b * a.N0;
  long long* gt1 = a.gt1 + (size_t)b * a.N1;
  long long* row_i = a.all_matches + (size_t)b * 2 * L;
  long long* row_j = row_i + L;
  if (n0 == 0 || n1 == 0) {                                 // the reference's skip sample (GlueSparse.py:52-61)
    for (int i = t; i < a.N0; i += 256) gt0[i] = -1;
    for (int j = t; j < a.N1; j += 256) gt1[j] = -1;
    for (int c = t; c < L; c += 256) { row_i[c] = -1; row_j[c] = -1; }
    if (t == 0) { a.n_matches[b] = 0; a.n_all[b] = 0; }
    return;
  }
  const int* nn0 = a.nn0 + (size_t)b * a.N0;
  const int* nn1 = a.nn1 + (size_t)b * a.N1;
  const double* d0 = a.d0 + (size_t)b * a.N0;
  // (i, j) is a match when each is the other's nearest and the distance is below the radius
  auto partner_of_j = [&](int j) -> int {
    const int i = nn1[j];
    if ((unsigned)i >= (unsigned)n0) return -1;
    return nn0[i] == j && d0[i] < a.radius ? i : -1;
  };
  auto partner_of_i = [&](int i) -> int {
    const int j = nn0[i];
    if ((unsigned)j >= (unsigned)n1) return -1;
    return nn1[j] == i && d0[i] < a.radius ? j : -1;
  };
  // the matches, ascending in j
  int n = 0;
  for (int j0 = 0; j0 < n1; j0 += 256) {
    const int j = j0 + t;
    const int i = j < n1 ? partner_of_j(j) : -1;
    int total;
    const int r = block_rank(i >= 0, wsum, total);
    if (j < n1) gt1[j] = i;
    if (i >= 0) { row_i[n + r] = i; row_j[n + r] = j; }
    n += total;
  }
  for (int j = n1 + t; j < a.N1; j += 256) gt1[j] = -1;
  // every unmatched i, ascending, against the dustbin column n1
  int pos = n;
  for (int i0 = 0; i0 < n0; i0 += 256) {
    const int i = i0 + t;
    const int j = i < n0 ? partner_of_i(i) : -1;
    int total;
    const int r = block_rank(i < n0 && j < 0, wsum, total);
    if (i < n0) gt0[i] = j;
    if (i < n0 && j < 0) { row_i[pos + r] = i; row_j[pos + r] = n1; }
    pos += total;
  }
  for (int i = n0 + t; i < a.N0; i += 256) gt0[i] = -1;
  // every unmatched j, ascending, against the dustbin row n0
  for (int j0 = 0; j0 < n1; j0 += 256) {
    const int j = j0 + t;
    const bool un = j < n1 && partner_of_j(j) < 0;
    int total;
    const int r = block_rank(un, wsum, total);
    if (un) { row_i[pos + r] = n0; row_j[pos + r] = j; }
    pos += total;
  }
  for (int c = pos + t; c < L; c += 256) { row_i[c] = -1; row_j[c] = -1; }
  if (t == 0) { a.n_matches[b] = n; a.n_all[b] = pos; }      // pos = n0 + n1 - n
}

// One workgroup per pair.  Z[x][y] = ((S[x][y] + u[x]) + v[y]) - norm in the operation order of the match kernels (sg_misc.hip); the
// dustbin row / column couples with bin_score.  Each thread adds its columns in ascending order, then a fixed tree over the 256
// partial sums: the same input gives the same bits.
__global__ __launch_bounds__(256) void match_loss_kernel(LossArgs a) {
  __shared__ float part[256];
  __shared__ int cnt[3];
  const int b = blockIdx.x, t = threadIdx.x;
  const int m = clampi(a.n0 ? a.n0[b] : a.N0, 0, a.N0), n = clampi(a.n1 ? a.n1[b] : a.N1, 0, a.N1);
  const int na = clampi(a.n_all[b], 0, a.L);
  if (t < 3) cnt[t] = 0;
  float acc = 0.f;
  if (na > 0 && m > 0 && n > 0) {
    const float norm = -logf((float)(m + n));
    const float* u = a.u + (size_t)b * (a.N0p + 1);
    const float* v = a.v + (size_t)b * (a.N1p + 1);
    const float* S = a.S + (size_t)b * a.N0p * a.N1p;
    const long long* xs = a.all_matches + (size_t)b * 2 * a.L;
    const long long* ys = xs + a.L;
    for (int c = t; c < na; c += 256) {
      const long long x = xs[c], y = ys[c];
      float term = __builtin_nanf("");                      // an index outside the transport matrix is not read
      if (x >= 0 && x <= m && y >= 0 && y <= n) {
        const float s = x < m && y < n ? S[(size_t)x * a.N1p + y] : a.alpha;
        const float z = ((s + u[x]) + v[y]) - norm;
        term = -logf(expf(z));                              // as written (:293): an exp that underflows makes the term +inf
      }
      acc += term;
    }
  }
  part[t] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) part[t] += part[t + o];
    __syncthreads();
  }
  if (t == 0) a.loss[b] = na > 0 && m > 0 && n > 0 ? part[0] / (float)na : 0.f;
  if (a.stats) {
    int g = 0, p = 0, c = 0;
    for (int i = t; i < a.N0; i += 256) {
      const long long mi = a.matches0[(size_t)b * a.N0 + i], gi = a.gt0[(size_t)b * a.N0 + i];
      g += gi >= 0;
      p += mi > -1;
      c += gi >= 0 && mi == gi;
    }
    atomicAdd(&cnt[0], g);                                  // (LDS, integers: the order cannot show)
    atomicAdd(&cnt[1], p);
    atomicAdd(&cnt[2], c);
    __syncthreads();
    if (t < 3) a.stats[(size_t)b * 3 + t] = cnt[t];
  }
}

}  // namespace

hipError_t launch_warp_perspective_u8(const uint8_t* src, long sstride, const double* minv, uint8_t* dst, int B, int H, int W, hipStream_t s) {
  hipLaunchKernelGGL(warp_perspective_u8_kernel, dim3((W + 63) / 64, (H + 3) / 4, B), dim3(256), 0, s, src, sstride, minv, dst, H, W);
  return hipGetLastError();
}

hipError_t launch_gt_matches(const GtArgs& a, hipStream_t s) {
  if (a.N0 > 0) hipLaunchKernelGGL(gt_project_kernel, dim3((a.N0 + 255) / 256, a.B), dim3(256), 0, s, a);
  const int nmax = a.N0 > a.N1 ? a.N0 : a.N1;
  if (a.N0 > 0 && a.N1 > 0) hipLaunchKernelGGL(gt_nearest_kernel, dim3((nmax + 255) / 256, a.B, 2), dim3(256), 0, s, a);
  hipLaunchKernelGGL(gt_assign_kernel, dim3(a.B), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_match_loss(const LossArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(match_loss_kernel, dim3(a.B), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace imx
