// homog.hip -- RANSAC homography fit on matched keypoints, one workgroup per image pair: the cv2.findHomography(mkpts0, mkpts1,
// cv2.RANSAC, thr) counterpart of registration.hip's 4-DoF similarity fit, and the corner error of a fit against a known warp.
// OpenCV's arithmetic is third-party and absent from the reference tree: parity is against tests/homography_ref.py, which restates the
// integer index draw exactly and solves every system with numpy's own routines.
//
// The matched coordinates are staged as the fp32 values they are; every operation after the staging is float64.  The inlier test is
// written with explicit fma() so that its three call sites (the count, the mask, the refit's selection) round alike, and the winning
// model is never recomputed: the thread that formed it hands its registers over.  No atomics, no workgroup waits on another.
#include "homog.h"
#include "imx_kernels.h"

namespace imx {
namespace {

__device__ __forceinline__ unsigned mix32(unsigned x) {     // murmur3 finaliser
  x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
  return x;
}

// the four distinct indices of hypothesis h among n >= 4 points: an integer hash of (seed, h, n) and of nothing else.  Draw k takes one
// of the n - k indices still free, counted in ascending order (tests/homography_ref.py: draw4 restates this)
__device__ __forceinline__ void draw4(unsigned seed, int h, int n, int& i0, int& i1, int& i2, int& i3) {
  unsigned s = mix32(seed + 0x9E3779B9u * (unsigned)(h + 1));
  s = mix32(s ^ (0x85EBCA6Bu * (unsigned)n));
  i0 = (int)(s % (unsigned)n);
  s = mix32(s + 0x27D4EB2Fu);
  i1 = (int)(s % (unsigned)(n - 1));
  s = mix32(s + 0x27D4EB2Fu);
  i2 = (int)(s % (unsigned)(n - 2));
  s = mix32(s + 0x27D4EB2Fu);
  i3 = (int)(s % (unsigned)(n - 3));
  if (i1 >= i0) ++i1;
  const int a = min(i0, i1), b = max(i0, i1);
  if (i2 >= a) ++i2;
  if (i2 >= b) ++i2;
  const int lo = min(a, i2), hi = max(b, i2), mid = a + b + i2 - lo - hi;
  if (i3 >= lo) ++i3;
  if (i3 >= mid) ++i3;
  if (i3 >= hi) ++i3;
}

// block-wide sum of a double over 256 threads in a fixed order (LDS scratch of 4 doubles): every thread gets the same bits
__device__ double block_sum(double v, double* scratch) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  return (scratch[0] + scratch[1]) + (scratch[2] + scratch[3]);
}

// the projective map of the unit square (0,0), (1,0), (1,1), (0,1) onto four points, none three of them collinear (Heckbert 1989)
__device__ __forceinline__ void square_to_quad(double x0, double y0, double x1, double y1, double x2, double y2, double x3, double y3, double* m) {
  const double dx1 = x1 - x2, dx2 = x3 - x2, sx = (x0 - x1) + (x2 - x3);
  const double dy1 = y1 - y2, dy2 = y3 - y2, sy = (y0 - y1) + (y2 - y3);
  const double den = dx1 * dy2 - dx2 * dy1;
  const double g = (sx * dy2 - dx2 * sy) / den, h = (dx1 * sy - sx * dy1) / den;
  m[0] = x1 - x0 + g * x1; m[1] = x3 - x0 + h * x3; m[2] = x0;
  m[3] = y1 - y0 + g * y1; m[4] = y3 - y0 + h * y3; m[5] = y0;
  m[6] = g; m[7] = h; m[8] = 1.0;
}

__device__ __forceinline__ double cross2(double ax, double ay, double bx, double by, double cx, double cy) {
  return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
}

// Hartley normalisation of one point set: x_n = (x - cx) s
struct Norm { double cx, cy, s; };

// T1^-1 Hn T0 for a model Hn in normalised coordinates with Hn[8] = 1
__device__ __forceinline__ void denormalise(const double* hn, const Norm& n0, const Norm& n1, double* P) {
  double g[9];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    g[3 * r] = hn[3 * r] * n0.s;
    g[3 * r + 1] = hn[3 * r + 1] * n0.s;
    g[3 * r + 2] = hn[3 * r + 2] - n0.s * (hn[3 * r] * n0.cx + hn[3 * r + 1] * n0.cy);
  }
  const double i1 = 1.0 / n1.s;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    P[c] = g[c] * i1 + n1.cx * g[6 + c];
    P[3 + c] = g[3 + c] * i1 + n1.cy * g[6 + c];
    P[6 + c] = g[6 + c];
  }
}

// the inlier rule: w > 0 and the squared forward reprojection error in destination pixels below thr^2.  Explicit fma: one rounding
// sequence wherever this is inlined.  A NaN anywhere is "no".
__device__ __forceinline__ bool is_inlier(const double* P, double x, double y, double u, double v, double thr2) {
  const double w = fma(P[6], x, fma(P[7], y, P[8]));
  const double px = fma(P[0], x, fma(P[1], y, P[2]));
  const double py = fma(P[3], x, fma(P[4], y, P[5]));
  const double ex = px / w - u, ey = py / w - v;
  const double e2 = fma(ex, ex, ey * ey);
  return w > 0.0 && e2 < thr2;
}

__device__ __forceinline__ void write_failure(const HomogArgs& a, int b) {
  const int tid = threadIdx.x;
  if (tid < 9) a.H[(size_t)b * 9 + tid] = 0.0;
  if (tid == 0) { a.n_inliers[b] = 0; a.best_h[b] = -1; }
  for (int i = tid; i < a.K0; i += 256) a.inlier[(size_t)b * a.K0 + i] = 0;
}

// The 27 distinct sums of the normal equations of the rows  [a p, 0, c1 q | b1]  and  [0, a p, c2 q | b2]  with p = (x, y, 1) and
// q = (x, y): the two standard DLT rows of a point (a = 1, c = -(u, v), b = (u, v)) and the two Jacobian rows of its reprojection
// error (a = 1/w, c = -(px, py)/w, b = -r)
struct Sums { double v[27]; };
__device__ __forceinline__ void add_rows(Sums& S, double x, double y, double a, double c1, double c2, double b1, double b2) {
  const double xx = x * x, xy = x * y, yy = y * y;
  const double a2 = a * a, ac1 = a * c1, ac2 = a * c2, cc = c1 * c1 + c2 * c2, cb = c1 * b1 + c2 * b2, ab1 = a * b1, ab2 = a * b2;
  S.v[0] += a2 * xx; S.v[1] += a2 * xy; S.v[2] += a2 * x; S.v[3] += a2 * yy; S.v[4] += a2 * y; S.v[5] += a2;
  S.v[6] += ac1 * xx; S.v[7] += ac1 * xy; S.v[8] += ac1 * yy; S.v[9] += ac1 * x; S.v[10] += ac1 * y;
  S.v[11] += ac2 * xx; S.v[12] += ac2 * xy; S.v[13] += ac2 * yy; S.v[14] += ac2 * x; S.v[15] += ac2 * y;
  S.v[16] += cc * xx; S.v[17] += cc * xy; S.v[18] += cc * yy;
  S.v[19] += ab1 * x; S.v[20] += ab1 * y; S.v[21] += ab1;
  S.v[22] += ab2 * x; S.v[23] += ab2 * y; S.v[24] += ab2;
  S.v[25] += cb * x; S.v[26] += cb * y;
}

// thread 0: the 8 x 9 augmented system from the reduced sums, Gaussian elimination with partial pivoting in LDS, the solution in x.
// false if a pivot is zero or not a number
__device__ bool solve8(const double* r, double (*A)[9], double* x) {
  for (int i = 0; i < 8; ++i)
    for (int j = 0; j < 9; ++j) A[i][j] = 0.0;
  for (int o = 0; o < 6; o += 3) {          // the block of p p^T, twice
    A[o][o] = r[0]; A[o][o + 1] = r[1]; A[o][o + 2] = r[2]; A[o + 1][o + 1] = r[3]; A[o + 1][o + 2] = r[4]; A[o + 2][o + 2] = r[5];
    const double* c = r + (o ? 11 : 6);
    A[o][6] = c[0]; A[o][7] = c[1]; A[o + 1][6] = c[1]; A[o + 1][7] = c[2]; A[o + 2][6] = c[3]; A[o + 2][7] = c[4];
  }
  A[6][6] = r[16]; A[6][7] = r[17]; A[7][7] = r[18];
  for (int i = 0; i < 8; ++i) {
    for (int j = 0; j < i; ++j) A[i][j] = A[j][i];
    A[i][8] = r[19 + i];
  }
  for (int c = 0; c < 8; ++c) {
    int piv = c;
    double best = fabs(A[c][c]);
    for (int q = c + 1; q < 8; ++q)
      if (fabs(A[q][c]) > best) { best = fabs(A[q][c]); piv = q; }
    if (!(best > 0.0) || !(best < 1e300)) return false;
    if (piv != c)
      for (int k = c; k < 9; ++k) { const double t = A[c][k]; A[c][k] = A[piv][k]; A[piv][k] = t; }
    for (int q = c + 1; q < 8; ++q) {
      const double f = A[q][c] / A[c][c];
      for (int k = c; k < 9; ++k) A[q][k] -= f * A[c][k];
    }
  }
  for (int c = 7; c >= 0; --c) {
    double t = A[c][8];
    for (int k = c + 1; k < 8; ++k) t -= A[c][k] * x[k];
    x[c] = t / A[c][c];
  }
  for (int c = 0; c < 8; ++c)
    if (!(fabs(x[c]) < 1e300)) return false;
  return true;
}

__global__ __launch_bounds__(256) void homog_ransac_kernel(HomogArgs a) {
  extern __shared__ float sm[];
  float* sx = a.K0 <= kHomogLdsSlots ? sm : a.scratch + (size_t)blockIdx.x * 4 * a.K0;
  float* sy = sx + a.K0;
  float* dx = sy + a.K0;
  float* dy = dx + a.K0;
  __shared__ int s_n, s_best_cnt, s_best_h, s_ok, s_fin;
  __shared__ int wcnt[4], wh[4];
  __shared__ double dscr[4], s_P[9], s_h[9], s_x[8], s_r[27], s_A[8][9];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* k0 = a.kpts0 + (size_t)b * a.K0 * 2;
  const float* k1 = a.kpts1 + (size_t)b * a.K1 * 2;
  const long long* m0 = a.matches0 + (size_t)b * a.K0;
  const int cnt0 = a.counts0 ? min(max(a.counts0[b], 0), a.K0) : a.K0;

  // ---- 1. ordered compaction of the matched pairs (index order); an index outside [0, K1) is "unmatched"
  if (tid == 0) s_n = 0;
  __syncthreads();
  for (int i0 = 0; i0 < cnt0; i0 += 256) {
    const int i = i0 + tid;
    const long long j = (i < cnt0) ? m0[i] : -1;
    const bool v = j >= 0 && j < a.K1;
    const unsigned long long bal = __ballot(v);
    if (lane == 0) wcnt[wave] = __popcll(bal);
    __syncthreads();
    int off = s_n;
    for (int w = 0; w < wave; ++w) off += wcnt[w];
    if (v) {
      const int pos = off + __popcll(bal & ((1ull << lane) - 1ull));
      sx[pos] = k0[2 * i]; sy[pos] = k0[2 * i + 1];
      dx[pos] = k1[2 * j]; dy[pos] = k1[2 * j + 1];
    }
    __syncthreads();
    if (tid == 0) s_n += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    __syncthreads();
  }
  const int n = s_n;
  if (n < 4) { write_failure(a, b); return; }

  // ---- 2. Hartley normalisation of both point sets over all n points: centroid to 0, mean distance to sqrt 2
  Norm n0, n1;
  {
    double t0 = 0, t1 = 0, t2 = 0, t3 = 0;
    for (int k = tid; k < n; k += 256) { t0 += (double)sx[k]; t1 += (double)sy[k]; t2 += (double)dx[k]; t3 += (double)dy[k]; }
    n0.cx = block_sum(t0, dscr) / n; n0.cy = block_sum(t1, dscr) / n;
    n1.cx = block_sum(t2, dscr) / n; n1.cy = block_sum(t3, dscr) / n;
    double d0 = 0, d1 = 0;
    for (int k = tid; k < n; k += 256) {
      const double px = (double)sx[k] - n0.cx, py = (double)sy[k] - n0.cy, qx = (double)dx[k] - n1.cx, qy = (double)dy[k] - n1.cy;
      d0 += sqrt(px * px + py * py); d1 += sqrt(qx * qx + qy * qy);
    }
    d0 = block_sum(d0, dscr) / n; d1 = block_sum(d1, dscr) / n;
    if (!(d0 > 0.0) || !(d1 > 0.0) || !(d0 < 1e300) || !(d1 < 1e300)) { write_failure(a, b); return; }   // uniform: every thread holds the same bits
    n0.s = sqrt(2.0) / d0; n1.s = sqrt(2.0) / d1;
  }
  const double thr2 = a.threshold * a.threshold;

  // ---- 3. hypotheses: one per thread at a time, the exact map through four matches, inliers counted over all n
  int best_cnt = -1, best_h = 0x7fffffff;
  double bP[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) bP[q] = 0.0;
  for (int h = tid; h < a.hypotheses; h += 256) {
    int id[4];
    draw4(a.seed, h, n, id[0], id[1], id[2], id[3]);
    double px[4], py[4], qx[4], qy[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      px[q] = ((double)sx[id[q]] - n0.cx) * n0.s; py[q] = ((double)sy[id[q]] - n0.cy) * n0.s;
      qx[q] = ((double)dx[id[q]] - n1.cx) * n1.s; qy[q] = ((double)dy[id[q]] - n1.cy) * n1.s;
    }
    // degenerate: a triple of (nearly) collinear points on either side, or a triple that changes orientation
    bool good = true;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int i = t == 3 ? 1 : 0, j = t >= 2 ? 2 : 1, k = t == 0 ? 2 : 3;      // (0,1,2) (0,1,3) (0,2,3) (1,2,3)
      const double cs = cross2(px[i], py[i], px[j], py[j], px[k], py[k]), cd = cross2(qx[i], qy[i], qx[j], qy[j], qx[k], qy[k]);
      good = good && fabs(cs) >= 1e-6 && fabs(cd) >= 1e-6 && ((cs > 0.0) == (cd > 0.0));
    }
    int cnt = -1;
    double P[9] = {};
    if (good) {
      double S[9], D[9], hn[9];
      square_to_quad(px[0], py[0], px[1], py[1], px[2], py[2], px[3], py[3], S);
      square_to_quad(qx[0], qy[0], qx[1], qy[1], qx[2], qy[2], qx[3], qy[3], D);
      const double adj[9] = {S[4] * S[8] - S[5] * S[7], S[2] * S[7] - S[1] * S[8], S[1] * S[5] - S[2] * S[4],
                             S[5] * S[6] - S[3] * S[8], S[0] * S[8] - S[2] * S[6], S[2] * S[3] - S[0] * S[5],
                             S[3] * S[7] - S[4] * S[6], S[1] * S[6] - S[0] * S[7], S[0] * S[4] - S[1] * S[3]};
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) hn[3 * r + c] = D[3 * r] * adj[c] + D[3 * r + 1] * adj[3 + c] + D[3 * r + 2] * adj[6 + c];
      // h33 = 1 in normalised coordinates: "w > 0" is the side of the horizon the centroid lies on
      const double inv = 1.0 / hn[8];
      if (fabs(inv) < 1e300) {
#pragma unroll
        for (int q = 0; q < 9; ++q) hn[q] *= inv;
        hn[8] = 1.0;
        denormalise(hn, n0, n1, P);
        cnt = 0;
#pragma unroll 1
        for (int k = 0; k < n; ++k) cnt += is_inlier(P, (double)sx[k], (double)sy[k], (double)dx[k], (double)dy[k], thr2) ? 1 : 0;
      }
    }
    if (cnt > best_cnt) {                  // ascending h per thread: the first best is kept
      best_cnt = cnt; best_h = h;
#pragma unroll
      for (int q = 0; q < 9; ++q) bP[q] = P[q];
    }
  }
  // ---- 4. the winner: the largest count, the lowest h among equals
  int rc = best_cnt, rh = best_h;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int oc = __shfl_xor(rc, o), oh = __shfl_xor(rh, o);
    if (oc > rc || (oc == rc && oh < rh)) { rc = oc; rh = oh; }
  }
  if (lane == 0) { wcnt[wave] = rc; wh[wave] = rh; }
  __syncthreads();
  if (tid == 0) {
    int bc = wcnt[0], bh = wh[0];
    for (int w = 1; w < 4; ++w)
      if (wcnt[w] > bc || (wcnt[w] == bc && wh[w] < bh)) { bc = wcnt[w]; bh = wh[w]; }
    s_best_cnt = bc; s_best_h = bh;
  }
  __syncthreads();
  const int win_cnt = s_best_cnt, win_h = s_best_h;
  if (win_cnt < 4) { write_failure(a, b); return; }
  if (best_h == win_h) {                   // exactly one thread formed hypothesis win_h: it hands the model over, nothing is recomputed
#pragma unroll
    for (int q = 0; q < 9; ++q) s_P[q] = bP[q];
  }
  __syncthreads();
  double P[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) P[q] = s_P[q];

  // ---- 5. the winning hypothesis' mask in keypoint0 index space (a later failure overwrites it: the same thread, the same addresses), and
  //         the compacted non-inliers marked in the staging itself (x0 = NaN; no input NaN reaches here: the mean distance was finite),
  //         so that the model's registers are free during the refit
  for (int i = tid; i < a.K0; i += 256) {
    const long long j = (i < cnt0) ? m0[i] : -1;
    unsigned char v = 0;
    if (j >= 0 && j < a.K1) v = is_inlier(P, (double)k0[2 * i], (double)k0[2 * i + 1], (double)k1[2 * j], (double)k1[2 * j + 1], thr2) ? 1 : 0;
    a.inlier[(size_t)b * a.K0 + i] = v;
  }
  for (int k = tid; k < n; k += 256)
    if (!is_inlier(P, (double)sx[k], (double)sy[k], (double)dx[k], (double)dy[k], thr2)) sx[k] = __int_as_float(0x7fc00000);
  __syncthreads();                         // the marks are visible to every thread: the refit may split the points any way it likes

  // ---- 6. refit on the winner's inliers in normalised coordinates: the linear problem (h33 = 1), then Gauss-Newton on the
  //         reprojection error.  Each sum runs over k = tid, tid + 256, ... and then through block_sum: a fixed order
  for (int pass = 0; pass <= a.refine_iters; ++pass) {
    Sums S;
#pragma unroll
    for (int q = 0; q < 27; ++q) S.v[q] = 0.0;
    double g[8] = {};
    if (pass > 0) {
#pragma unroll
      for (int q = 0; q < 8; ++q) g[q] = s_h[q];
    }
    for (int k = tid; k < n; k += 256) {
      const double rx = (double)sx[k], ry = (double)sy[k], ru = (double)dx[k], rv = (double)dy[k];
      if (rx != rx) continue;               // marked above: not an inlier of the winner
      const double x = (rx - n0.cx) * n0.s, y = (ry - n0.cy) * n0.s, u = (ru - n1.cx) * n1.s, v = (rv - n1.cy) * n1.s;
      if (pass == 0) {
        add_rows(S, x, y, 1.0, -u, -v, u, v);
      } else {
        const double iw = 1.0 / (g[6] * x + g[7] * y + 1.0);
        const double qx = (g[0] * x + g[1] * y + g[2]) * iw, qy = (g[3] * x + g[4] * y + g[5]) * iw;
        add_rows(S, x, y, iw, -qx * iw, -qy * iw, u - qx, v - qy);
      }
    }
#pragma unroll
    for (int q = 0; q < 27; ++q) {
      const double t = block_sum(S.v[q], dscr);
      if (tid == 0) s_r[q] = t;
    }
    if (tid == 0) {
      const bool ok = solve8(s_r, s_A, s_x);
      if (ok)
        for (int q = 0; q < 8; ++q) s_h[q] = pass == 0 ? s_x[q] : s_h[q] + s_x[q];
      s_ok = ok ? 1 : 0;
    }
    __syncthreads();
    if (!s_ok) { write_failure(a, b); return; }
  }

  // ---- 7. back to pixels, H[8] = 1
  if (tid == 0) {
    double hn[9], Hp[9];
    for (int q = 0; q < 8; ++q) hn[q] = s_h[q];
    hn[8] = 1.0;
    denormalise(hn, n0, n1, Hp);
    double fro = 0.0;
#pragma unroll
    for (int q = 0; q < 9; ++q) fro += Hp[q] * Hp[q];
    fro = sqrt(fro);
    const bool ok = fro < 1e300 && fabs(Hp[8]) >= 1e-12 * fro && fro > 0.0;
    if (ok) {
      const double inv = 1.0 / Hp[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) a.H[(size_t)b * 9 + q] = Hp[q] * inv;
      a.H[(size_t)b * 9 + 8] = 1.0;
      a.n_inliers[b] = win_cnt;
      a.best_h[b] = win_h;
    }
    s_fin = ok ? 1 : 0;
  }
  __syncthreads();
  if (!s_fin) { write_failure(a, b); return; }

}

__global__ __launch_bounds__(256) void homog_corner_error_kernel(const double* __restrict__ He, const double* __restrict__ Hg, int B, int width,
                                                                 int height, double* __restrict__ err) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const double* E = He + (size_t)b * 9;
  const double* G = Hg + (size_t)b * 9;
  bool zero = true;
#pragma unroll
  for (int q = 0; q < 9; ++q) zero = zero && E[q] == 0.0;
  const double X = (double)(width - 1), Y = (double)(height - 1);
  double sum = 0.0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const double x = (c == 1 || c == 2) ? X : 0.0, y = c >= 2 ? Y : 0.0;
    const double we = E[6] * x + E[7] * y + E[8], wg = G[6] * x + G[7] * y + G[8];
    const double ex = (E[0] * x + E[1] * y + E[2]) / we - (G[0] * x + G[1] * y + G[2]) / wg;
    const double ey = (E[3] * x + E[4] * y + E[5]) / we - (G[3] * x + G[4] * y + G[5]) / wg;
    sum += sqrt(ex * ex + ey * ey);
  }
  sum *= 0.25;
  err[b] = (zero || !(sum < INFINITY)) ? (double)INFINITY : sum;      // no fit, or a corner on a horizon: worse than every threshold
}

}  // namespace

hipError_t launch_homog_ransac(const HomogArgs& a, hipStream_t s) {
  if (a.K0 <= 0 || a.K1 <= 0 || a.B <= 0 || a.hypotheses <= 0 || a.refine_iters < 0) return hipErrorInvalidValue;
  if (a.K0 > kHomogLdsSlots && !a.scratch) return hipErrorInvalidValue;
  static unsigned long long attr = 0;
  raise_lds_limit(reinterpret_cast<const void*>(homog_ransac_kernel), kHomogLdsSlots * 4 * (int)sizeof(float), attr);
  hipLaunchKernelGGL(homog_ransac_kernel, dim3((unsigned)a.B), dim3(256), a.K0 <= kHomogLdsSlots ? (size_t)a.K0 * 4 * sizeof(float) : 0, s, a);
  return hipGetLastError();
}

hipError_t launch_homog_corner_error(const double* H_est, const double* H_gt, int B, int width, int height, double* err, hipStream_t s) {
  if (B <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(homog_corner_error_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, H_est, H_gt, B, width, height, err);
  return hipGetLastError();
}

}  // namespace imx
