// sptrain.hip -- SuperPoint descriptor training up to the forward value of the objective (superpoint_train_descriptor.py ->
// datasets/ALLSS.py -> superpoint/Train_model_heatmap.py:83-314) for gfx950:
//
//   warp_labels        : ALLSS.points_to_2D / warpLabels (datasets/data_tools.py:36-54): label and residual maps of warped points
//   erode_mask         : the margin of compute_valid_mask (utils/utils.py:449-452): cv2.erode by an elliptic element
//   detector_loss      : labels2Dto3D + getMasks + softmax-BCE (utils/utils.py:456-468, Train_model_frontend.py:362-377,
//                        Train_model_heatmap.py:72-81), one pass per 8x8 cell
//   desc_loss_sparse   : descriptor_loss_sparse (loss_functions/sparse_loss.py:98-174, pixelwise_contrastive_loss.py:132-251)
//
// All fp32 with the default compile flags (NaN honoured, correctly rounded division).  Coordinate arithmetic runs with contraction
// off and the fused multiply-adds of the reference's matrix product written out (warp_row).  No floating-point atomics: every sum is per-thread ascending, then
// a fixed tree, then one finishing workgroup.  The only atomics are integer ones whose result does not depend on arrival order
// (a maximum of point indices, an OR of error bits).  Restated in tests/sptrain_ref.py; DESIGN.md section 11.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "imx_kernels.h"
#include "sptrain_dev.h"

namespace imx {
namespace {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// (warp_row and warp_point, the matrix product of warp_points, are in sptrain_dev.h: libimx_sploop.so warps by the same function)

// ------------------------------------------------------------------------------------------------------------- warp_labels
__global__ __launch_bounds__(256) void wl_fill_kernel(WarpLabelsArgs a) {
  const size_t n = (size_t)a.B * a.H * a.W;
  if (blockIdx.x == 0 && threadIdx.x == 0 && a.flag) *a.flag = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    a.labels[i] = 0.0f;
    if (a.owner) a.owner[i] = -1;
    if (a.res) { a.res[2 * i] = 0.0f; a.res[2 * i + 1] = 0.0f; }     // (B,2,H,W) holds 2 n floats: any order fills it
  }
}

// the pixel point i of image b lands on, and its residual; false: the point is dropped (or, without matrices, an error)
__device__ __forceinline__ bool wl_pixel(const WarpLabelsArgs& a, int b, int i, int& px, int& py, float& dx, float& dy) {
#pragma clang fp contract(off)
  const float* p = a.pts + ((size_t)b * a.Kcap + i) * 2;
  const float x = truncf(p[0]), y = truncf(p[1]);                       // .long()
  const float xm = (float)(a.W - 1), ym = (float)(a.H - 1);
  if (!a.mats) {                                                       // points_to_2D: no warp, no filter
    if (!(x >= 0.0f && x <= xm && y >= 0.0f && y <= ym)) {
      if (a.flag) atomicOr(a.flag, 1);
      return false;
    }
    px = (int)x; py = (int)y; dx = 0.0f; dy = 0.0f;
    return true;
  }
  const float* m = a.mats + (size_t)b * 9;
  float wx, wy;
  warp_point(m, x, y, wx, wy);
  if (!(wx >= 0.0f && wx <= xm && wy >= 0.0f && wy <= ym)) return false;   // filter_points on the unrounded point (NaN: dropped)
  const float rx = rintf(wx), ry = rintf(wy);                          // round(): half to even
  px = (int)rx; py = (int)ry; dx = wx - rx; dy = wy - ry;
  return true;
}

template <int PASS>
__global__ __launch_bounds__(256) void wl_points_kernel(WarpLabelsArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  const int n = a.counts ? clampi(a.counts[b], 0, a.Kcap) : a.Kcap;
  if (i >= n) return;                                                  // rows past the count are never read
  int px, py;
  float dx, dy;
  if (!wl_pixel(a, b, i, px, py, dx, dy)) return;
  const size_t pix = ((size_t)b * a.H + py) * a.W + px;
  if (PASS == 0) {
    a.labels[pix] = 1.0f;                                              // (every writer of a pixel writes the same value)
    if (a.owner) atomicMax(a.owner + pix, i);                          // two points on one pixel: the higher index owns the residual
  } else if (a.owner[pix] == i) {
    const size_t plane = (size_t)a.H * a.W;
    float* r = a.res + (size_t)b * 2 * plane + (size_t)py * a.W + px;
    r[0] = dx;
    r[plane] = dy;
  }
}

// ------------------------------------------------------------------------------------------------------------- erode_mask
// cv2.erode with getStructuringElement(MORPH_ELLIPSE, (2r, 2r)), anchor (r, r): the minimum over the element's pixels that lie
// inside the image.  Row i of the element covers columns [j1, j2).
__global__ __launch_bounds__(256) void erode_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W, int r) {
  __shared__ short j1[2 * kErodeMaxRadius], j2[2 * kErodeMaxRadius];
  const int t = threadIdx.y * 64 + threadIdx.x;
  if (t < 2 * r) {
    const int dy = t - r;                                              // |dy| <= r on every row
    const double rr = (double)r;
    const int dx = (int)rint(rr * sqrt((rr * rr - (double)dy * dy) / (rr * rr)));
    j1[t] = (short)max(r - dx, 0);
    j2[t] = (short)min(r + dx + 1, 2 * r);
  }
  __syncthreads();
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, b = blockIdx.z;
  if (x >= W || y >= H) return;
  const float* img = in + (size_t)b * H * W;
  float m = INFINITY;                                                  // (the anchor itself is always in the element)
  for (int i = 0; i < 2 * r; ++i) {
    const int yy = y + i - r;
    if (yy < 0 || yy >= H) continue;
    const int x0 = max(x + j1[i] - r, 0), x1 = min(x + j2[i] - 1 - r, W - 1);
    for (int xx = x0; xx <= x1; ++xx) {
      const float v = img[(size_t)yy * W + xx];
      m = v < m ? v : m;
    }
  }
  out[((size_t)b * H + y) * W + x] = m;
}

// fixed tree over the 256 values of a workgroup; the result is in s[0]
template <class T>
__device__ __forceinline__ void block_tree(T* s, int t) {
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) s[t] += s[t + o];
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------------------- detector_loss
// One 8x8 cell per thread.  -log p_c = min(100, (max - x_c) + log S) with S the sum of exp(x - max); -log(1 - p_c) from the OTHER
// exponentials: -log1p(-e_c / S) for every channel but the (first) maximum, log S - log(S without it) there.
__global__ __launch_bounds__(256) void det_loss_cells_kernel(const float* __restrict__ semi, const float* __restrict__ labels,
                                                             const float* __restrict__ mask, int B, int Hc, int Wc, double* __restrict__ part) {
  __shared__ double sl[256], sm[256];
  const int t = threadIdx.x;
  const long cell = (long)blockIdx.x * 256 + t;
  const long cells = (long)Hc * Wc;
  double closs = 0.0, cmask = 0.0;
  if (cell < (long)B * cells) {
    const int b = (int)(cell / cells);
    const int rem = (int)(cell - (long)b * cells);
    const int cy = rem / Wc, cx = rem - cy * Wc;
    const int W = Wc * 8;
    const size_t o = ((size_t)b * Hc * 8 + (size_t)cy * 8) * W + (size_t)cx * 8;
    const float* lp = labels + o;
    const float* mp = mask + o;
    float ls = 0.0f, mprod = 1.0f;
    for (int dy = 0; dy < 8; ++dy) {
      const float4 l0 = *reinterpret_cast<const float4*>(lp + (size_t)dy * W), l1 = *reinterpret_cast<const float4*>(lp + (size_t)dy * W + 4);
      const float4 m0 = *reinterpret_cast<const float4*>(mp + (size_t)dy * W), m1 = *reinterpret_cast<const float4*>(mp + (size_t)dy * W + 4);
      ls += l0.x; ls += l0.y; ls += l0.z; ls += l0.w; ls += l1.x; ls += l1.y; ls += l1.z; ls += l1.w;
      mprod *= m0.x; mprod *= m0.y; mprod *= m0.z; mprod *= m0.w; mprod *= m1.x; mprod *= m1.y; mprod *= m1.z; mprod *= m1.w;
    }
    float dust = 1.0f - ls;
    if (dust < 1.0f) dust = 0.0f;
    const float dn = ls + dust;
    const float* xp = semi + (size_t)b * 65 * cells + rem;
    float mx = xp[0];
    int k = 0;
    for (int c = 1; c < 65; ++c) {
      const float x = xp[(size_t)c * cells];
      if (x > mx) { mx = x; k = c; }
    }
    float S = 0.0f, Srest = 0.0f;
    for (int c = 0; c < 65; ++c) {
      const float e = expf(xp[(size_t)c * cells] - mx);
      S += e;
      if (c != k) Srest += e;
    }
    const float logS = logf(S);
    float loss = 0.0f;
    for (int c = 0; c < 65; ++c) {
      const float x = xp[(size_t)c * cells];
      const float tg = (c < 64 ? lp[(size_t)(c >> 3) * W + (c & 7)] : dust) / dn;
      const float nlp = fminf(100.0f, (mx - x) + logS);
      float nl1p = c == k ? logS - logf(Srest) : -log1pf(-(expf(x - mx) / S));
      nl1p = fminf(100.0f, fmaxf(nl1p, 0.0f));
      loss += tg * nlp + (1.0f - tg) * nl1p;
    }
    closs = (double)(loss * mprod);
    cmask = (double)mprod;
  }
  sl[t] = closs;
  sm[t] = cmask;
  block_tree(sl, t);
  block_tree(sm, t);
  if (t == 0) { part[2 * (size_t)blockIdx.x] = sl[0]; part[2 * (size_t)blockIdx.x + 1] = sm[0]; }
}

__global__ __launch_bounds__(256) void det_loss_finish_kernel(const double* __restrict__ part, int nblk, float* __restrict__ out) {
  __shared__ double sl[256], sm[256];
  const int t = threadIdx.x;
  double l = 0.0, m = 0.0;
  for (int i = t; i < nblk; i += 256) { l += part[2 * (size_t)i]; m += part[2 * (size_t)i + 1]; }
  sl[t] = l;
  sm[t] = m;
  block_tree(sl, t);
  block_tree(sm, t);
  if (t == 0) { out[0] = (float)(sl[0] / (sm[0] + 1e-10)); out[1] = (float)sm[0]; }
}

// ------------------------------------------------------------------------------------------------------------- desc_loss_sparse
// exclusive prefix count of a flag over a 256-thread workgroup, in thread order (the gt_assemble pattern of trainpairs.hip)
__device__ __forceinline__ int block_rank(bool flag, int* wsum, int& total) {
  const unsigned long long mask = __ballot(flag);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int within = __popcll(mask & ((1ull << lane) - 1ull));
  __syncthreads();
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

// One workgroup per image: cells in row-major order as (x, y), warp_points in fp32, round_() half to even, filter_points against
// (Wc, Hc); the surviving (a, b) flat cell indices compacted in row-major order.  Entries past n_valid are -1.
__global__ __launch_bounds__(256) void dl_pairs_kernel(DescLossArgs a) {
#pragma clang fp contract(off)
  __shared__ int wsum[4];
  const int b = blockIdx.x, t = threadIdx.x;
  const int N = a.Hc * a.Wc;
  if (b == 0 && t == 0 && a.flag) *a.flag = 0;
  const float* h = a.hcell + (size_t)b * 9;
  int* pr = a.pairs + (size_t)b * N * 2;
  int* po = a.pairs_out ? a.pairs_out + (size_t)b * N * 2 : nullptr;
  int n = 0;
  for (int c0 = 0; c0 < N; c0 += 256) {
    const int c = c0 + t;
    bool keep = false;
    int ib = 0;
    if (c < N) {
      const int yi = c / a.Wc, xi = c - yi * a.Wc;
      const float x = (float)xi, y = (float)yi;
      const float u = warp_row(h, x, y), v = warp_row(h + 3, x, y), w = warp_row(h + 6, x, y);
      const float rx = rintf(u / w), ry = rintf(v / w);
      keep = rx >= 0.0f && rx <= (float)(a.Wc - 1) && ry >= 0.0f && ry <= (float)(a.Hc - 1);
      if (keep) ib = (int)ry * a.Wc + (int)rx;
    }
    int total;
    const int r = block_rank(keep, wsum, total);
    if (keep) {
      pr[2 * (n + r)] = c; pr[2 * (n + r) + 1] = ib;
      if (po) { po[2 * (n + r)] = c; po[2 * (n + r) + 1] = ib; }
    }
    n += total;
  }
  for (int c = n + t; c < N; c += 256) {
    pr[2 * c] = -1; pr[2 * c + 1] = -1;
    if (po) { po[2 * c] = -1; po[2 * c + 1] = -1; }
  }
  if (t == 0) a.nvalid[b] = n;
}

// (B,d,N) channel-major -> (B,N,d) cell-major, both maps (blockIdx.z = 2 b + side): 32 x 32 tiles through LDS
__global__ __launch_bounds__(256) void dl_transpose_kernel(DescLossArgs a) {
  __shared__ float tile[32][33];
  const int N = a.Hc * a.Wc, d = a.d;
  const int b = blockIdx.z >> 1, side = blockIdx.z & 1;
  const float* src = (side ? a.desc_b : a.desc_a) + (size_t)b * d * N;
  float* dst = (side ? a.tb : a.ta) + (size_t)b * N * d;
  const int n0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  for (int j = threadIdx.y; j < 32; j += 8) {
    const int c = c0 + j, n = n0 + threadIdx.x;
    if (c < d && n < N) tile[j][threadIdx.x] = src[(size_t)c * N + n];
  }
  __syncthreads();
  for (int j = threadIdx.y; j < 32; j += 8) {
    const int n = n0 + j, c = c0 + threadIdx.x;
    if (c < d && n < N) dst[(size_t)n * d + c] = tile[threadIdx.x][j];
  }
}

// One wave per match m.  A descriptor row of d floats is read by a group of LPR = min(64, pow2 >= d / 4) lanes as float4 (one
// contiguous line of the cell-major map); the 64 / LPR groups of the wave stride the R non-matches.  partial (B,M,3) =
// {max(0, 1 - <a, b>), sum_r max(0, <a_1d, nb_r> - margin), count of the non-zero ones}.
__global__ __launch_bounds__(256) void dl_main_kernel(DescLossArgs a) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= a.M) return;                                                // (wave-uniform; no workgroup barrier below)
  const int N = a.Hc * a.Wc, d = a.d;
  const int nv = a.nvalid[b];
  if (nv <= 0) return;                                                 // the finishing kernel writes NaN for this image
  float* part = a.partial + ((size_t)b * a.M + m) * 3;
  const int ch = a.choice[(size_t)b * a.M + m];
  if ((unsigned)ch >= (unsigned)nv) {                                  // a caller error: flagged, nothing read through it
    if (lane == 0) { if (a.flag) atomicOr(a.flag, 1); part[0] = 0.0f; part[1] = 0.0f; part[2] = 0.0f; }
    return;
  }
  const int ia = a.pairs[((size_t)b * N + ch) * 2], ib = a.pairs[((size_t)b * N + ch) * 2 + 1];
  const DlLane L = dl_lanes(d, lane);
  const int g = lane / L.lpr, G = 64 / L.lpr;
  const float* ta = a.ta + (size_t)b * N * d;
  const float* tb = a.tb + (size_t)b * N * d;
  float4 av[kDlBlocks], x[kDlBlocks], y[kDlBlocks];
  dl_load(ta + (size_t)ia * d, L, av);                                 // the 1d descriptor: the non-match side reads it whatever the method
  float dotm;
  if (a.method2d) {
    dl_sample(ta, dl_taps(ia, a.Hc, a.Wc), a.Hc, a.Wc, d, L, x);
    dl_sample(tb, dl_taps(ib, a.Hc, a.Wc), a.Hc, a.Wc, d, L, y);
    dotm = dl_dot(x, y, L);
  } else {
    dl_load(tb + (size_t)ib * d, L, y);
    dotm = dl_dot(av, y, L);
  }
  float mt = 1.0f - dotm;
  mt = mt < 0.0f ? 0.0f : mt;                                          // torch.clamp(min=0): NaN stays NaN
  const int* nm = a.nonmatch + ((size_t)b * a.M + m) * a.R;
  float sum = 0.0f;
  int cnt = 0;
  for (int r0 = 0; r0 < a.R; r0 += G) {
    const int r = r0 + g;
    const int idx = r < a.R ? nm[r] : 0;
    const bool ok = r < a.R && (unsigned)idx < (unsigned)N;
    if (r < a.R && !ok && L.sub == 0 && a.flag) atomicOr(a.flag, 2);
    dl_load(tb + (size_t)(ok ? idx : 0) * d, L, y);
    float v = dl_dot(av, y, L) - a.margin;
    v = v < 0.0f ? 0.0f : v;
    if (ok) { sum += v; cnt += v != 0.0f ? 1 : 0; }
  }
  for (int o = L.lpr; o < 64; o <<= 1) { sum += __shfl_xor(sum, o); cnt += __shfl_xor(cnt, o); }
  if (lane == 0) { part[0] = mt; part[1] = sum; part[2] = (float)cnt; }
}

// One workgroup: per image the M partials in ascending m per thread, then the fixed tree; then the batch means
__global__ __launch_bounds__(256) void dl_finish_kernel(DescLossArgs a) {
  __shared__ double s0[256], s1[256], s2[256];
  __shared__ double mean[3];
  const int t = threadIdx.x;
  if (t < 3) mean[t] = 0.0;
  for (int b = 0; b < a.B; ++b) {
    const int nv = a.nvalid[b];
    double p0 = 0.0, p1 = 0.0, p2 = 0.0;
    if (nv > 0)
      for (int m = t; m < a.M; m += 256) {
        const float* p = a.partial + ((size_t)b * a.M + m) * 3;
        p0 += (double)p[0]; p1 += (double)p[1]; p2 += (double)p[2];
      }
    s0[t] = p0; s1[t] = p1; s2[t] = p2;
    block_tree(s0, t);
    block_tree(s1, t);
    block_tree(s2, t);
    if (t == 0) {
      float* o = a.out + (size_t)b * 5;
      const double nan = (double)__builtin_nanf("");
      const double match = nv > 0 ? (double)a.lamda_d * (s0[0] / (double)a.M) : nan;
      const double non = nv > 0 ? s1[0] / (s2[0] + 1.0) : nan;
      o[0] = (float)(match + non); o[1] = (float)match; o[2] = (float)non; o[3] = nv > 0 ? (float)s2[0] : 0.0f; o[4] = (float)nv;
      mean[0] += (double)o[0]; mean[1] += (double)o[1]; mean[2] += (double)o[2];
    }
    __syncthreads();
  }
  if (t < 3) a.mean[t] = (float)(mean[t] / (double)a.B);
}

}  // namespace

hipError_t launch_warp_labels(const WarpLabelsArgs& a, hipStream_t s) {
  if (a.B < 1 || a.B > 65535 || a.H < 1 || a.W < 1 || a.Kcap < 0) return hipErrorInvalidValue;
  const size_t n = (size_t)a.B * a.H * a.W;
  const int fill = (int)std::min<size_t>((n + 255) / 256, 2048);
  wl_fill_kernel<<<fill, 256, 0, s>>>(a);
  if (a.Kcap > 0) {
    const dim3 grid((a.Kcap + 255) / 256, a.B);
    wl_points_kernel<0><<<grid, 256, 0, s>>>(a);
    if (a.res && a.mats) wl_points_kernel<1><<<grid, 256, 0, s>>>(a);
  }
  return hipGetLastError();
}

hipError_t launch_erode_mask(const float* in, float* out, int B, int H, int W, int radius, hipStream_t s) {
  if (B < 1 || B > 65535 || H < 1 || W < 1 || (H + 3) / 4 > 65535 || radius < 1 || radius > kErodeMaxRadius) return hipErrorInvalidValue;
  erode_kernel<<<dim3((W + 63) / 64, (H + 3) / 4, B), dim3(64, 4), 0, s>>>(in, out, H, W, radius);
  return hipGetLastError();
}

int detector_loss_blocks(int B, int Hc, int Wc) { return (int)(((long)B * Hc * Wc + 255) / 256); }

hipError_t launch_detector_loss(const float* semi, const float* labels, const float* mask, int B, int Hc, int Wc, double* part, float* out,
                                hipStream_t s) {
  if (B < 1 || Hc < 1 || Wc < 1 || (long)B * Hc * Wc > (1l << 30)) return hipErrorInvalidValue;
  const int nblk = detector_loss_blocks(B, Hc, Wc);
  det_loss_cells_kernel<<<nblk, 256, 0, s>>>(semi, labels, mask, B, Hc, Wc, part);
  det_loss_finish_kernel<<<1, 256, 0, s>>>(part, nblk, out);
  return hipGetLastError();
}

hipError_t launch_desc_pairs(const DescLossArgs& a, hipStream_t s) {
  if (a.B < 1 || a.B > 65535 || a.Hc < 1 || a.Wc < 1 || (long)a.Hc * a.Wc > (1l << 24)) return hipErrorInvalidValue;
  dl_pairs_kernel<<<a.B, 256, 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_desc_loss_sparse(const DescLossArgs& a, hipStream_t s) {
  const long N = (long)a.Hc * a.Wc;
  if (a.B < 1 || a.B > 32767 || a.Hc < 1 || a.Wc < 1 || N > (1l << 24) || a.d < 4 || a.d % 4 || a.d > 256 * kDlBlocks || a.M < 1 || a.R < 1 ||
      (a.M + 3) / 4 > 2147483647 / 2)
    return hipErrorInvalidValue;
  last_form = "desc_loss_sparse:cell-major";
  dl_pairs_kernel<<<a.B, 256, 0, s>>>(a);
  dl_transpose_kernel<<<dim3((unsigned)((N + 31) / 32), (a.d + 31) / 32, 2 * a.B), dim3(32, 8), 0, s>>>(a);
  dl_main_kernel<<<dim3((a.M + 3) / 4, a.B), 256, 0, s>>>(a);
  dl_finish_kernel<<<1, 256, 0, s>>>(a);
  return hipGetLastError();
}

}  // namespace imx
