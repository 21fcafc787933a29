// spgrad.hip -- gradients of the two SuperPoint training losses with respect to what the network emits (semi, desc), for gfx950:
//
//   detector_loss_grad      : d out[0] / d semi of sptrain.hip's detector_loss, the derivative of the conditioned form it evaluates
//   desc_loss_sparse_grad   : d mean[0] / d desc_{a,b} of sptrain.hip's desc_loss_sparse
//
// Both run AFTER the forward's own launchers (the values are theirs, bit for bit) and read what those left: out[1] (the mask sum),
// out[b][3] (the hard-negative count), the cell-major maps, the pair list.  No floating-point atomics.  The descriptor gradient is a
// scatter with heavy collisions; it is turned into a gather: every (match, slot) entry gets a destination cell and a coefficient, a
// stable counting sort groups the entries by destination (integer atomics in the histogram only; the fill places by rank), and one
// lane group per destination adds its rows in ascending entry order.  DESIGN.md section 12; restated in tests/spgrad_ref.py.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "imx_kernels.h"
#include "sptrain_dev.h"

namespace imx {
namespace {

// ------------------------------------------------------------------------------------------------------------- detector_loss_grad
// One 8x8 cell per thread, the forward's quantities formed the forward's way (targets, first maximum k, e_c = exp(x_c - max), S,
// S without k).  With q_c = -t_c [-log p_c unclamped] + (1 - t_c) [-log(1 - p_c) unclamped] p_c / (1 - p_c):
//   dL/dx_j = (m / D) (q_j - p_j sum_c q_c).
// p_c / (1 - p_c) = e_c / (sum of the other exponentials).  At the maximum that ratio overflows once the others underflow, so the
// terms that carry it are multiplied out first: ratio_k (1 - p_k) = p_k = 1 / S and p_j ratio_k = (e_j / Srest) / S.
__global__ __launch_bounds__(256) void det_grad_kernel(const float* __restrict__ semi, const float* __restrict__ labels,
                                                       const float* __restrict__ mask, int B, int Hc, int Wc, const float* __restrict__ out,
                                                       const float* __restrict__ gout, float* __restrict__ grad) {
  const long cell = (long)blockIdx.x * 256 + threadIdx.x;
  const long cells = (long)Hc * Wc;
  if (cell >= (long)B * cells) return;
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
  float* gp = grad + (size_t)b * 65 * cells + rem;
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
  // first pass: A = sum of the live t_c, Brest = sum over c != k of the live (1 - t_c) ratio_c, r_k = the live (1 - t_k)
  float A = 0.0f, Brest = 0.0f, rk = 0.0f;
  for (int c = 0; c < 65; ++c) {
    const float x = xp[(size_t)c * cells];
    const float tg = (c < 64 ? lp[(size_t)(c >> 3) * W + (c & 7)] : dust) / dn;
    const float e = expf(x - mx);
    if ((mx - x) + logS <= 100.0f) A += tg;                              // a clamped term is a constant: it contributes nothing
    if (c == k) {
      if (logS - logf(Srest) <= 100.0f) rk = 1.0f - tg;
    } else if (-log1pf(-(e / S)) <= 100.0f) {
      Brest += (1.0f - tg) * (e / (S - e));
    }
  }
  const double D = (double)out[1] + 1e-10;
  const float scale = (float)((double)(gout ? gout[0] : 1.0f) * (double)mprod / D);
  const float uk = rk != 0.0f ? rk / Srest : 0.0f;                       // (rk live means Srest > 0)
  for (int c = 0; c < 65; ++c) {
    const float x = xp[(size_t)c * cells];
    const float tg = (c < 64 ? lp[(size_t)(c >> 3) * W + (c & 7)] : dust) / dn;
    const float e = expf(x - mx);
    const float p = e / S;
    float g = (mx - x) + logS <= 100.0f ? -tg : 0.0f;
    if (c == k) {
      g += rk / S;
    } else {
      if (-log1pf(-(e / S)) <= 100.0f) g += (1.0f - tg) * (e / (S - e));
      g -= uk * e / S;
    }
    g -= p * (Brest - A);
    gp[(size_t)c * cells] = scale * g;
  }
}

// ------------------------------------------------------------------------------------------------------------- desc_loss_sparse_grad
// Slots of match m (K = 2 T + 1 + R of them, T taps), entry e = m K + slot; destinations 0 .. N-1 are a's cells, N .. 2N-1 b's:
//   [0, T)         a's match taps        row ym (b's match vector)            coefficient -w_m tap weight     where 1 - <x, y> >= 0
//   T              a's non-match sum     row an (sum of the active nb_r)      coefficient  w_n
//   [T+1, 2T+1)    b's match taps        row xm (a's match vector)            coefficient -w_m tap weight     where 1 - <x, y> >= 0
//   2T+1+r         b's non-match r       row ta[ia] (the 1d descriptor)       coefficient  w_n                where <a, nb_r> - margin > 0
// One wave per match, the forward's lane layout and the forward's dot products.
__global__ __launch_bounds__(256) void dg_rows_kernel(DescGradArgs g) {
  const DescLossArgs& a = g.f;
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= a.M) return;
  const int N = a.Hc * a.Wc, d = a.d, T = a.method2d ? 4 : 1, K = 2 * T + 1 + a.R;
  const DlLane L = dl_lanes(d, lane);
  const int grp = lane / L.lpr, G = 64 / L.lpr;
  const size_t bm = (size_t)b * a.M + m;
  int* keys = g.keys + bm * K;
  float* coef = g.coef + bm * K;
  float4* xm = reinterpret_cast<float4*>(g.xm + bm * d);
  float4* ym = reinterpret_cast<float4*>(g.ym + bm * d);
  float4* an = reinterpret_cast<float4*>(g.an + bm * d);
  const int nv = a.nvalid[b];
  const int ch = a.choice[bm];
  if (nv <= 0 || (unsigned)ch >= (unsigned)nv) {                         // this match takes no part: no destination, zero rows
    if (nv <= 0 && m == 0 && lane == 0 && a.flag) atomicOr(a.flag, 4);
    for (int q = lane; q < K; q += 64) { keys[q] = -1; coef[q] = 0.0f; }
    if (grp == 0)
      for (int kb = 0; kb < kDlBlocks; ++kb) {
        const int j = L.sub + kb * L.lpr;
        if (j < L.nvec) { xm[j] = make_float4(0.f, 0.f, 0.f, 0.f); ym[j] = xm[j]; an[j] = xm[j]; }
      }
    if (lane == 0) g.ia[bm] = -1;
    return;
  }
  const int ia = a.pairs[((size_t)b * N + ch) * 2], ib = a.pairs[((size_t)b * N + ch) * 2 + 1];
  const float go = g.gout ? g.gout[0] : 1.0f;
  const float wm = go * a.lamda_d / ((float)a.M * (float)a.B);
  const float wn = go / ((a.out[(size_t)b * 5 + 3] + 1.0f) * (float)a.B);  // the hard-negative count is a constant of the derivative
  const float* ta = a.ta + (size_t)b * N * d;
  const float* tb = a.tb + (size_t)b * N * d;
  float4 av[kDlBlocks], x[kDlBlocks], y[kDlBlocks];
  dl_load(ta + (size_t)ia * d, L, av);
  Tap4 t4a, t4b;
  if (a.method2d) {
    t4a = dl_taps(ia, a.Hc, a.Wc);
    t4b = dl_taps(ib, a.Hc, a.Wc);
    dl_sample(ta, t4a, a.Hc, a.Wc, d, L, x);
    dl_sample(tb, t4b, a.Hc, a.Wc, d, L, y);
  } else {
    dl_load(tb + (size_t)ib * d, L, y);
#pragma unroll
    for (int kb = 0; kb < kDlBlocks; ++kb) x[kb] = av[kb];
  }
  const float dotm = dl_dot(x, y, L);
  const bool live = 1.0f - dotm >= 0.0f;                                 // inclusive: clamp(min=0) passes the gradient at 0
  if (grp == 0)
    for (int kb = 0; kb < kDlBlocks; ++kb) {
      const int j = L.sub + kb * L.lpr;
      if (j < L.nvec) { xm[j] = x[kb]; ym[j] = y[kb]; }
    }
  if (lane == 0) {
    g.ia[bm] = ia;
    if (a.method2d) {
      const Tap4 ts[2] = {t4a, t4b};
      for (int side = 0; side < 2; ++side) {
        const Tap4& t = ts[side];
        const int xs[4] = {t.x0, t.x0 + 1, t.x0, t.x0 + 1}, ys[4] = {t.y0, t.y0, t.y0 + 1, t.y0 + 1};
        const float ws[4] = {t.nw, t.ne, t.sw, t.se};
        for (int q = 0; q < 4; ++q) {
          const bool in = t.ok && xs[q] >= 0 && xs[q] < a.Wc && ys[q] >= 0 && ys[q] < a.Hc;
          const int slot = side * (T + 1) + q;
          keys[slot] = live && in ? side * N + ys[q] * a.Wc + xs[q] : -1;
          coef[slot] = -wm * ws[q];
        }
      }
    } else {
      keys[0] = live ? ia : -1;         coef[0] = -wm;
      keys[T + 1] = live ? N + ib : -1; coef[T + 1] = -wm;
    }
    keys[T] = ia;
    coef[T] = wn;
  }
  const int* nm = a.nonmatch + bm * a.R;
  float4 acc[kDlBlocks];
#pragma unroll
  for (int kb = 0; kb < kDlBlocks; ++kb) acc[kb] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int r0 = 0; r0 < a.R; r0 += G) {                                  // group grp takes r = grp, grp + G, ... in ascending order
    const int r = r0 + grp;
    const int idx = r < a.R ? nm[r] : 0;
    const bool ok = r < a.R && (unsigned)idx < (unsigned)N;
    dl_load(tb + (size_t)(ok ? idx : 0) * d, L, y);
    const float v = dl_dot(av, y, L) - a.margin;
    const bool act = ok && v > 0.0f;                                     // strict
    if (act) {
#pragma unroll
      for (int kb = 0; kb < kDlBlocks; ++kb) { acc[kb].x += y[kb].x; acc[kb].y += y[kb].y; acc[kb].z += y[kb].z; acc[kb].w += y[kb].w; }
    }
    if (r < a.R && L.sub == 0) { keys[2 * T + 1 + r] = act ? N + idx : -1; coef[2 * T + 1 + r] = wn; }
  }
  for (int o = L.lpr; o < 64; o <<= 1) {                                 // the groups' sums: a fixed butterfly
#pragma unroll
    for (int kb = 0; kb < kDlBlocks; ++kb) {
      acc[kb].x += __shfl_xor(acc[kb].x, o); acc[kb].y += __shfl_xor(acc[kb].y, o);
      acc[kb].z += __shfl_xor(acc[kb].z, o); acc[kb].w += __shfl_xor(acc[kb].w, o);
    }
  }
  if (grp == 0)
    for (int kb = 0; kb < kDlBlocks; ++kb) {
      const int j = L.sub + kb * L.lpr;
      if (j < L.nvec) an[j] = acc[kb];
    }
}

// counts per (image, segment, destination): integer additions, whose result does not depend on arrival order
__global__ __launch_bounds__(256) void dg_hist_kernel(DescGradArgs g, int E, int D2) {
  const int sgm = blockIdx.x, b = blockIdx.y;
  const int* keys = g.keys + (size_t)b * E;
  int* hist = g.hist + ((size_t)b * g.S + sgm) * D2;
  const long e1 = min((long)E, ((long)sgm + 1) * g.seg);
  for (long e = (long)sgm * g.seg + threadIdx.x; e < e1; e += 256) {
    const int key = keys[e];
    if (key >= 0) atomicAdd(hist + key, 1);
  }
}

// One workgroup per image: offs[c] = entries of destinations before c; hist[s][c] becomes segment s's first position for c
__global__ __launch_bounds__(256) void dg_scan_kernel(DescGradArgs g, int D2) {
  __shared__ int sc[256];
  __shared__ int carry;
  const int b = blockIdx.x, t = threadIdx.x;
  int* hist = g.hist + (size_t)b * g.S * D2;
  int* offs = g.offs + (size_t)b * (D2 + 1);
  if (t == 0) carry = 0;
  __syncthreads();
  for (int c0 = 0; c0 < D2; c0 += 256) {
    const int c = c0 + t;
    int tot = 0;
    if (c < D2)
      for (int sgm = 0; sgm < g.S; ++sgm) tot += hist[(size_t)sgm * D2 + c];
    sc[t] = tot;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {                                  // inclusive scan over the workgroup
      const int v = t >= o ? sc[t - o] : 0;
      __syncthreads();
      sc[t] += v;
      __syncthreads();
    }
    int start = carry + sc[t] - tot;
    if (c < D2) {
      offs[c] = start;
      for (int sgm = 0; sgm < g.S; ++sgm) {
        const int n = hist[(size_t)sgm * D2 + c];
        hist[(size_t)sgm * D2 + c] = start;
        start += n;
      }
    }
    __syncthreads();
    if (t == 255) carry += sc[255];
    __syncthreads();
  }
  if (t == 0) offs[D2] = carry;
}

// The stable fill: a segment's workgroup walks its entries 256 at a time in ascending order; an entry goes to its destination's cursor
// plus its rank among the chunk's earlier entries with the same destination, then the cursor moves past the chunk's.  No tickets.
__global__ __launch_bounds__(256) void dg_fill_kernel(DescGradArgs g, int E, int D2) {
  __shared__ int sk[256];
  const int sgm = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  const int* keys = g.keys + (size_t)b * E;
  int* cursor = g.hist + ((size_t)b * g.S + sgm) * D2;                   // this workgroup's alone
  int* list = g.list + (size_t)b * E;
  const long e0 = (long)sgm * g.seg, e1 = min((long)E, e0 + g.seg);
  for (long c0 = e0; c0 < e1; c0 += 256) {
    const long e = c0 + t;
    const int key = e < e1 ? keys[e] : -1;
    sk[t] = key;
    __syncthreads();
    int rank = 0, cnt = 0;
    if (key >= 0) {
      for (int j = 0; j < 256; ++j) {
        const bool same = sk[j] == key;
        cnt += same ? 1 : 0;
        rank += same && j < t ? 1 : 0;
      }
      const int base = __hip_atomic_load(cursor + key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (a coherent read of what an earlier chunk stored)
      list[base + rank] = (int)e;
    }
    __syncthreads();
    if (key >= 0 && rank == cnt - 1) {
      const int base = __hip_atomic_load(cursor + key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(cursor + key, base + cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __threadfence_block();
    __syncthreads();
  }
}

// One lane group per destination row: coefficient times source row, in ascending entry order (m, then slot), one fused multiply-add
// per channel and entry.  A destination without entries gets zeros.
__global__ __launch_bounds__(256) void dg_reduce_kernel(DescGradArgs g, int E, int D2) {
  const DescLossArgs& a = g.f;
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int N = a.Hc * a.Wc, d = a.d, T = a.method2d ? 4 : 1, K = 2 * T + 1 + a.R;
  const DlLane L = dl_lanes(d, lane);
  const int G = 64 / L.lpr;
  const long dest = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * G + lane / L.lpr;
  if (dest >= D2) return;
  const int* offs = g.offs + (size_t)b * (D2 + 1);
  const int* list = g.list + (size_t)b * E;
  const float* coef = g.coef + (size_t)b * E;
  const float* ta = a.ta + (size_t)b * N * d;
  float4 acc[kDlBlocks], v[kDlBlocks];
#pragma unroll
  for (int kb = 0; kb < kDlBlocks; ++kb) acc[kb] = make_float4(0.f, 0.f, 0.f, 0.f);
  const int i1 = offs[dest + 1];
  for (int i = offs[dest]; i < i1; ++i) {
    const int e = list[i];
    const int m = e / K, slot = e - m * K;
    const size_t bm = (size_t)b * a.M + m;
    const float* row = slot < T ? g.ym + bm * d : slot == T ? g.an + bm * d : slot < 2 * T + 1 ? g.xm + bm * d : ta + (size_t)g.ia[bm] * d;
    const float c = coef[e];
    dl_load(row, L, v);
#pragma unroll
    for (int kb = 0; kb < kDlBlocks; ++kb) {
      acc[kb].x = fmaf(c, v[kb].x, acc[kb].x); acc[kb].y = fmaf(c, v[kb].y, acc[kb].y);
      acc[kb].z = fmaf(c, v[kb].z, acc[kb].z); acc[kb].w = fmaf(c, v[kb].w, acc[kb].w);
    }
  }
  float4* out = reinterpret_cast<float4*>(g.gt + ((size_t)b * D2 + dest) * d);
#pragma unroll
  for (int kb = 0; kb < kDlBlocks; ++kb) {
    const int j = L.sub + kb * L.lpr;
    if (j < L.nvec) out[j] = acc[kb];
  }
}

// (B,2N,d) cell-major -> the two (B,d,N) channel-major gradients (blockIdx.z = 2 b + side): 32 x 32 tiles through LDS
__global__ __launch_bounds__(256) void dg_transpose_kernel(DescGradArgs g) {
  __shared__ float tile[32][33];
  const int N = g.f.Hc * g.f.Wc, d = g.f.d;
  const int b = blockIdx.z >> 1, side = blockIdx.z & 1;
  const float* src = g.gt + ((size_t)b * 2 + side) * N * d;
  float* dst = (side ? g.grad_b : g.grad_a) + (size_t)b * d * N;
  const int n0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  for (int j = threadIdx.y; j < 32; j += 8) {
    const int n = n0 + j, c = c0 + threadIdx.x;
    if (c < d && n < N) tile[j][threadIdx.x] = src[(size_t)n * d + c];
  }
  __syncthreads();
  for (int j = threadIdx.y; j < 32; j += 8) {
    const int c = c0 + j, n = n0 + threadIdx.x;
    if (c < d && n < N) dst[(size_t)c * N + n] = tile[threadIdx.x][j];
  }
}

}  // namespace

hipError_t launch_detector_loss_grad(const float* semi, const float* labels, const float* mask, int B, int Hc, int Wc, const float* out,
                                     const float* gout, float* grad, hipStream_t s) {
  if (B < 1 || Hc < 1 || Wc < 1 || (long)B * Hc * Wc > (1l << 30)) return hipErrorInvalidValue;
  det_grad_kernel<<<detector_loss_blocks(B, Hc, Wc), 256, 0, s>>>(semi, labels, mask, B, Hc, Wc, out, gout, grad);
  return hipGetLastError();
}

hipError_t launch_desc_loss_sparse_grad(const DescGradArgs& g, hipStream_t s) {
  const DescLossArgs& a = g.f;
  const long N = (long)a.Hc * a.Wc, K = desc_grad_slots(a.R, a.method2d), E = (long)a.M * K, D2 = 2 * N;
  if (a.B < 1 || a.B > 32767 || N < 1 || N > (1l << 24) || a.d < 4 || a.d % 4 || a.d > 256 * kDlBlocks || a.M < 1 || a.R < 1 || E > (1l << 30) ||
      g.S < 1 || g.S > kDescGradMaxSegments || (long)g.S * g.seg < E)
    return hipErrorInvalidValue;
  last_form = "desc_loss_sparse_grad:inverse-list";
  dg_rows_kernel<<<dim3((a.M + 3) / 4, a.B), 256, 0, s>>>(g);
  hipError_t e = hipMemsetAsync(g.hist, 0, (size_t)a.B * g.S * D2 * sizeof(int), s);
  if (e != hipSuccess) return e;
  dg_hist_kernel<<<dim3(g.S, a.B), 256, 0, s>>>(g, (int)E, (int)D2);
  dg_scan_kernel<<<a.B, 256, 0, s>>>(g, (int)D2);
  dg_fill_kernel<<<dim3(g.S, a.B), 256, 0, s>>>(g, (int)E, (int)D2);
  int lpr = 1;
  while (lpr < a.d / 4 && lpr < 64) lpr <<= 1;
  const long per_block = 4 * (64 / lpr);
  dg_reduce_kernel<<<dim3((unsigned)((D2 + per_block - 1) / per_block), a.B), 256, 0, s>>>(g, (int)E, (int)D2);
  dg_transpose_kernel<<<dim3((unsigned)((N + 31) / 32), (a.d + 31) / 32, 2 * a.B), dim3(32, 8), 0, s>>>(g);
  return hipGetLastError();
}

}  // namespace imx
