// homoadapt.hip — homographic adaptation (pseudo-label export, superpoint_export_pseudo.py:57-110): projective warp of an
// image under N homographies, the fused un-warp + aggregation of the N detector heatmaps, and the greedy-NMS point extraction
// of the aggregated map.  All fp32, default compile flags: NaN is honoured (a pixel no warp covers is 0 / 0 = NaN, as in the
// reference) and divisions are correctly rounded.  Streaming kernels: the N x H x W stacks are read once.
#include "imx_kernels.h"

namespace imx {
namespace {

// torch.linspace(-1, 1, n)[i] in fp32 (utils/utils.py:411): the first half counts up from the start, the second half down from the end
__device__ __forceinline__ float lin_coord(int i, int n) {
  const float step = 2.0f / (float)(n - 1);
  return i < n / 2 ? -1.0f + step * (float)i : 1.0f - step * (float)(n - 1 - i);
}

// warp_points (utils/utils.py:358-386) of the normalised pixel (x, y) under the row-major 3x3 matrix m, then grid_sample's
// un-normalisation for align_corners=True: ((g + 1) / 2) (size - 1)
__device__ __forceinline__ void src_coord(const float* __restrict__ m, int x, int y, int H, int W, float& ix, float& iy) {
  const float xn = lin_coord(x, W), yn = lin_coord(y, H);
  const float u = m[0] * xn + m[1] * yn + m[2];
  const float v = m[3] * xn + m[4] * yn + m[5];
  const float w = m[6] * xn + m[7] * yn + m[8];
  ix = ((u / w + 1.0f) * 0.5f) * (float)(W - 1);
  iy = ((v / w + 1.0f) * 0.5f) * (float)(H - 1);
}

// compute_valid_mask (utils/utils.py:427-454, erosion_radius 0) = nearest sampling of an all-ones image: the rounded
// (half-to-even) source pixel lies inside the image.  NaN / infinite coordinates compare false.
__device__ __forceinline__ bool nearest_inside(float ix, float iy, int H, int W, int& xi, int& yi) {
  const float rx = rintf(ix), ry = rintf(iy);
  if (!(rx >= 0.0f && rx <= (float)(W - 1) && ry >= 0.0f && ry <= (float)(H - 1))) return false;
  xi = (int)rx; yi = (int)ry;
  return true;
}

// Bilinear taps of grid_sample (zero padding): corner (x0, y0) = floor, weights as torch forms them.  Returns false when no
// tap can lie inside (also NaN / infinite coordinates), so x0 / y0 are only converted when they are in [-1, size - 1].
struct Taps { int x0, y0; float nw, ne, sw, se; };
__device__ __forceinline__ bool bilinear_taps(float ix, float iy, int H, int W, Taps& t) {
  if (!(ix > -1.0f && ix < (float)W && iy > -1.0f && iy < (float)H)) return false;
  const float fx = floorf(ix), fy = floorf(iy);
  t.x0 = (int)fx; t.y0 = (int)fy;
  const float ex = (fx + 1.0f) - ix, ey = (fy + 1.0f) - iy, dx = ix - fx, dy = iy - fy;
  t.nw = ex * ey; t.ne = dx * ey; t.sw = ex * dy; t.se = dx * dy;
  return true;
}

// (a) inv_warp_image_batch (utils/utils.py:388-421).  src: N images spaced src_stride floats (0: one image shared by all N), or
// null = an all-ones image.  mask_out (optional): the valid mask of the same matrices.
__global__ void __launch_bounds__(256) ha_warp_kernel(const float* __restrict__ src, long src_stride, const float* __restrict__ mats, int H,
                                                      int W, int nearest, float* __restrict__ dst, float* __restrict__ mask_out) {
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, b = blockIdx.z;
  if (x >= W || y >= H) return;
  float ix, iy;
  src_coord(mats + (size_t)b * 9, x, y, H, W, ix, iy);
  const float* img = src ? src + (size_t)b * src_stride : nullptr;
  const size_t o = ((size_t)b * H + y) * W + x;
  int xi = 0, yi = 0;
  const bool inside = nearest_inside(ix, iy, H, W, xi, yi);
  if (mask_out) mask_out[o] = inside ? 1.0f : 0.0f;
  if (!dst) return;
  float r = 0.0f;
  if (nearest) {
    if (inside) r = img ? img[(size_t)yi * W + xi] : 1.0f;
  } else {
    Taps t;
    if (bilinear_taps(ix, iy, H, W, t)) {
      const bool l = t.x0 >= 0, rr = t.x0 + 1 < W, u = t.y0 >= 0, d = t.y0 + 1 < H;
      const float* p = img ? img + (long)t.y0 * W + t.x0 : nullptr;
      if (u && l) r += (p ? p[0] : 1.0f) * t.nw;
      if (u && rr) r += (p ? p[1] : 1.0f) * t.ne;
      if (d && l) r += (p ? p[W] : 1.0f) * t.sw;
      if (d && rr) r += (p ? p[W + 1] : 1.0f) * t.se;
    }
  }
  dst[o] = r;
}

// (c) combine_heatmap (utils/utils.py:507-518) in one pass: for every output pixel, i = 0 .. N-1 IN THAT ORDER, the bilinear
// sample of heat_i mask_i and of mask_i at the pixel's source under unwarp_i; out = sum heat-samples / sum mask-samples.  A
// workgroup owns a 32 x 8 output tile for all i, so its taps of one map stay inside a small patch of that map.
// RECOMPUTE: no stored masks -- the mask value of a tap pixel is evaluated from warp_i with the warp kernel's own predicate
// (the same fp32 expression: bit-identical results), four more projective coordinates per view and pixel instead of four loads.
template <bool RECOMPUTE>
__global__ void __launch_bounds__(256) ha_combine_kernel(const float* __restrict__ heat, const float* __restrict__ mask, const float* __restrict__ warp,
                                                         const float* __restrict__ unwarp, int N, int H, int W, float* __restrict__ out,
                                                         float* __restrict__ count) {
  const int x = blockIdx.x * 32 + threadIdx.x, y = blockIdx.y * 8 + threadIdx.y;
  if (x >= W || y >= H) return;
  float sh = 0.0f, sm = 0.0f;
  const size_t plane = (size_t)H * W;
  for (int i = 0; i < N; ++i) {
    float ix, iy;
    src_coord(unwarp + (size_t)i * 9, x, y, H, W, ix, iy);
    Taps t;
    float vh = 0.0f, vm = 0.0f;
    if (bilinear_taps(ix, iy, H, W, t)) {
      const bool l = t.x0 >= 0, r = t.x0 + 1 < W, u = t.y0 >= 0, d = t.y0 + 1 < H;
      const long o = (long)t.y0 * W + t.x0;
      const float* ph = heat + i * plane + o;
      const float* pm = RECOMPUTE ? nullptr : mask + i * plane + o;
      const float* wm = RECOMPUTE ? warp + (size_t)i * 9 : nullptr;
      auto mval = [&](int dx, int dy) -> float {
        if (!RECOMPUTE) return pm[dy * W + dx];
        float sx, sy;
        int xi, yi;
        src_coord(wm, t.x0 + dx, t.y0 + dy, H, W, sx, sy);
        return nearest_inside(sx, sy, H, W, xi, yi) ? 1.0f : 0.0f;
      };
      if (u && l) { const float m = mval(0, 0); vh += (ph[0] * m) * t.nw; vm += m * t.nw; }
      if (u && r) { const float m = mval(1, 0); vh += (ph[1] * m) * t.ne; vm += m * t.ne; }
      if (d && l) { const float m = mval(0, 1); vh += (ph[W] * m) * t.sw; vm += m * t.sw; }
      if (d && r) { const float m = mval(1, 1); vh += (ph[W + 1] * m) * t.se; vm += m * t.se; }
    }
    sh += vh;
    sm += vm;
  }
  const size_t o = (size_t)y * W + x;
  out[o] = sh / sm;
  if (count) count[o] = sm;
}

// ------------------------------------------------------------------------------------------------------------------ (d) points
// getPtsFromHeatmap + nms_fast (utils/utils.py:250-332) as rounds on a dense state map.  Rank: higher score first, equal scores
// by the lower row-major index.  A candidate is KEPT once every higher-ranked candidate in its window is SUPPRESSED, SUPPRESSED
// once one of them is KEPT.  States only ever move UNDECIDED -> KEPT | SUPPRESSED and a decision taken on final states is the
// greedy one, so rounds may update in place and read each other's states in any order.
enum : unsigned char { ST_NONE = 0, ST_UNDECIDED = 1, ST_KEPT = 2, ST_SUPPRESSED = 3 };

__device__ __forceinline__ unsigned char st_load(const unsigned char* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_store(unsigned char* p, unsigned char v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ void __launch_bounds__(256) hp_init_kernel(const float* __restrict__ h, int n, float thr, unsigned char* __restrict__ st) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p < n) st[p] = h[p] >= thr ? ST_UNDECIDED : ST_NONE;      // (NaN >= thr is false: never a candidate)
}

// one attempt to decide pixel p; returns the state it has afterwards.  Neighbour states are read past the L1 (st_load): plain
// loads -- a stale UNDECIDED would only postpone a decision -- with four pixels per thread were measured SLOWER, 133 vs 61 us
// per round at 480 x 640 with half the pixels candidates
__device__ __forceinline__ unsigned char hp_decide(const float* __restrict__ h, unsigned char* st, int H, int W, int r, int p) {
  const int y = p / W, x = p - y * W;
  const float hp = h[p];
  const int y0 = max(y - r, 0), y1 = min(y + r, H - 1), x0 = max(x - r, 0), x1 = min(x + r, W - 1);
  bool pending = false;
  for (int yy = y0; yy <= y1; ++yy)
    for (int xx = x0; xx <= x1; ++xx) {
      const int q = yy * W + xx;
      if (q == p) continue;
      const unsigned char sq = st_load(st + q);
      if (sq == ST_NONE || sq == ST_SUPPRESSED) continue;
      const float hq = h[q];
      if (!(hq > hp || (hq == hp && q < p))) continue;
      if (sq == ST_KEPT) { st_store(st + p, ST_SUPPRESSED); return ST_SUPPRESSED; }
      pending = true;
    }
  if (pending) return ST_UNDECIDED;
  st_store(st + p, ST_KEPT);
  return ST_KEPT;
}

// ctr[k] = pixels still undecided after round k; round k > 0 returns at once when round k-1 left none
__global__ void __launch_bounds__(256) hp_round_kernel(const float* __restrict__ h, unsigned char* st, int H, int W, int r, int k, int* ctr) {
  if (k > 0 && ctr[k - 1] == 0) return;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= H * W) return;
  if (st_load(st + p) != ST_UNDECIDED) return;
  if (hp_decide(h, st, H, W, r, p) == ST_UNDECIDED) atomicAdd(ctr + k, 1);
}

// what the bounded rounds left undecided, as a list (any order)
__global__ void __launch_bounds__(256) hp_undecided_kernel(const unsigned char* __restrict__ st, int n, const int* last_ctr, int* und_count,
                                                           int* __restrict__ und) {
  if (*last_ctr == 0) return;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p < n && st[p] == ST_UNDECIDED) und[atomicAdd(und_count, 1)] = p;
}

// COST, worst case: this pass is serial in the number of rounds and runs on one CU.  On detector maps the list is a few hundred
// pixels and the rounds a few dozen (49 us at 480 x 640).  On a PLATEAU (a constant or saturated map, conf_thresh <= 0 on a flat
// image: ties go by index) the dependency front needs about 2 (W + H) / (r + 1) rounds -- ~450 at 480 x 640 -- over up to H W
// entries each: one launch of the order of 0.1 - 1 s.  Correct and terminating, but slow; likewise hp_emit_kernel ranks in
// O(K^2) of the K survivors (nms_dist 0 on a map that is all candidates: K = H W).
// the path without a bound: ONE workgroup repeats rounds over that list until nothing is undecided.  Every round decides at
// least the highest-ranked undecided pixel, so the loop ends; a workgroup barrier separates the rounds.
__global__ void __launch_bounds__(1024) hp_finish_kernel(const float* __restrict__ h, unsigned char* st, int H, int W, int r,
                                                         const int* und_count, const int* __restrict__ und) {
  __shared__ int remaining;
  const int n = *und_count;
  if (n == 0) return;
  for (;;) {
    if (threadIdx.x == 0) remaining = 0;
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += 1024) {
      const int p = und[j];
      if (st_load(st + p) == ST_UNDECIDED && hp_decide(h, st, H, W, r, p) == ST_UNDECIDED) atomicAdd(&remaining, 1);
    }
    __threadfence();
    __syncthreads();
    const int left = remaining;
    __syncthreads();
    if (left == 0) break;
  }
}

// survivors inside the border (removed AFTER the NMS, utils/utils.py:265-270), any order
__global__ void __launch_bounds__(256) hp_kept_kernel(const float* __restrict__ h, const unsigned char* __restrict__ st, int H, int W, int border,
                                                      int* kept_count, int* __restrict__ kept_idx, float* __restrict__ kept_score) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int y = p / W, x = p - y * W;
  const bool keep = p < H * W && st[p] == ST_KEPT && !(x < border || x >= W - border || y < border || y >= H - border);
  // one atomic per wave: the lanes that keep a point take consecutive slots after the leader's base
  const unsigned long long m = __ballot(keep);
  if (!m) return;
  const int lane = threadIdx.x & 63, leader = __ffsll((long long)m) - 1;
  int base = 0;
  if (lane == leader) base = atomicAdd(kept_count, __popcll(m));
  base = __shfl(base, leader);
  if (!keep) return;
  const int j = base + __popcll(m & ((1ull << lane) - 1ull));
  kept_idx[j] = p;
  kept_score[j] = h[p];
}

// rank of every survivor by counting (exact, independent of the order of the list), then its row (x, y, conf); optional 5 x 5
// centroid (soft_argmax_points, model_wrap.py:146-176: softmax(log(p / (sum p + 1e-6))) = p / sum p on the zero-padded map)
__global__ void __launch_bounds__(256) hp_emit_kernel(const float* __restrict__ h, int H, int W, const int* kept_count, const int* __restrict__ kept_idx,
                                                      const float* __restrict__ kept_score, int top_k, int subpixel, float* __restrict__ pts, int cap,
                                                      int* __restrict__ count_out) {
  // a workgroup ranks 64 survivors at a time: the list passes through LDS in tiles of 256, wave w counts against quarter w of every
  // tile (all its lanes read the same entry: an LDS broadcast), the four partial ranks are added at the end
  __shared__ float ts[256];
  __shared__ int ti[256];
  __shared__ int part_rank[4][64];
  const int K = *kept_count;
  const int limit = top_k > 0 ? min(top_k, cap) : cap;
  if (blockIdx.x == 0 && threadIdx.x == 0 && count_out) *count_out = top_k > 0 ? min(K, top_k) : K;
  const int lane = threadIdx.x & 63, part = threadIdx.x >> 6;
  for (int j0 = blockIdx.x * 64; j0 < K; j0 += gridDim.x * 64) {
    const int j = j0 + lane;
    const bool valid = j < K;
    const int p = valid ? kept_idx[j] : 0;
    const float s = valid ? kept_score[j] : 0.0f;
    int rank = 0;
    for (int t0 = 0; t0 < K; t0 += 256) {
      __syncthreads();
      const int k = t0 + threadIdx.x;
      ts[threadIdx.x] = k < K ? kept_score[k] : 0.0f;
      ti[threadIdx.x] = k < K ? kept_idx[k] : 0;
      __syncthreads();
      const int e = min(64, K - (t0 + part * 64));
      for (int q = 0; q < e; ++q) {
        const float sk = ts[part * 64 + q];
        rank += (sk > s || (sk == s && ti[part * 64 + q] < p)) ? 1 : 0;
      }
    }
    part_rank[part][lane] = rank;
    __syncthreads();
    rank = part_rank[0][lane] + part_rank[1][lane] + part_rank[2][lane] + part_rank[3][lane];
    if (part == 0 && valid && rank < limit) {
      const int y = p / W, x = p - y * W;
      float fx = (float)x, fy = (float)y;
      if (subpixel) {
        float sp = 0.0f, sx = 0.0f, sy = 0.0f;
        for (int dy = 0; dy < 5; ++dy)
          for (int dx = 0; dx < 5; ++dx) {
            const int yy = y + dy - 2, xx = x + dx - 2;
            const float v = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? h[yy * W + xx] : 0.0f;
            sp += v; sx += v * (float)dx; sy += v * (float)dy;
          }
        fx += sx / sp - 2.0f;
        fy += sy / sp - 2.0f;
      }
      pts[(size_t)rank * 3 + 0] = fx;
      pts[(size_t)rank * 3 + 1] = fy;
      pts[(size_t)rank * 3 + 2] = s;
    }
  }
}

}  // namespace

hipError_t launch_ha_warp(const float* src, long src_stride, const float* mats, int N, int H, int W, int nearest, float* dst,
                          float* mask_out, hipStream_t s) {
  if (N < 1 || N > 65535 || H < 2 || W < 2 || (H + 3) / 4 > 65535) return hipErrorInvalidValue;
  ha_warp_kernel<<<dim3((W + 63) / 64, (H + 3) / 4, N), dim3(64, 4), 0, s>>>(src, src_stride, mats, H, W, nearest, dst, mask_out);
  return hipGetLastError();
}

hipError_t launch_ha_combine(const float* heat, const float* mask, const float* warp, const float* unwarp, int N, int H, int W, float* out,
                             float* count, hipStream_t s) {
  if (N < 1 || H < 2 || W < 2 || (H + 7) / 8 > 65535 || (!mask && !warp)) return hipErrorInvalidValue;
  const dim3 grid((W + 31) / 32, (H + 7) / 8), block(32, 8);
  last_form = mask ? "ha_combine:stored-masks" : "ha_combine:recomputed-masks";
  if (mask) ha_combine_kernel<false><<<grid, block, 0, s>>>(heat, mask, nullptr, unwarp, N, H, W, out, count);
  else ha_combine_kernel<true><<<grid, block, 0, s>>>(heat, nullptr, warp, unwarp, N, H, W, out, count);
  return hipGetLastError();
}

size_t heatmap_points_scratch_bytes(int H, int W) {
  const size_t n = (size_t)H * W;
  return 256 + (n + 255) / 256 * 256 + 3 * n * 4;
}

hipError_t launch_heatmap_points(const HeatmapPointsArgs& a, hipStream_t s) {
  const long n = (long)a.H * a.W;
  if (a.H < 1 || a.W < 1 || n > (1l << 30) || a.nms_dist < 0 || a.cap < 0) return hipErrorInvalidValue;
  // scratch: [64 ints: round counters 0 .. kHeatmapPointsRounds-1, then undecided count, kept count][state bytes][und][kept_idx][kept_score]
  char* base = static_cast<char*>(a.scratch);
  int* ctr = reinterpret_cast<int*>(base);
  unsigned char* st = reinterpret_cast<unsigned char*>(base + 256);
  const size_t stb = ((size_t)n + 255) / 256 * 256;
  int* und = reinterpret_cast<int*>(base + 256 + stb);
  int* kept_idx = und + n;
  float* kept_score = reinterpret_cast<float*>(kept_idx + n);
  int* und_count = ctr + kHeatmapPointsRounds;
  int* kept_count = und_count + 1;
  hipError_t e = hipMemsetAsync(ctr, 0, 256, s);
  if (e != hipSuccess) return e;
  const int blocks = (int)((n + 255) / 256);
  hp_init_kernel<<<blocks, 256, 0, s>>>(a.heatmap, (int)n, a.conf_thresh, st);
  for (int k = 0; k < kHeatmapPointsRounds; ++k) hp_round_kernel<<<blocks, 256, 0, s>>>(a.heatmap, st, a.H, a.W, a.nms_dist, k, ctr);
  hp_undecided_kernel<<<blocks, 256, 0, s>>>(st, (int)n, ctr + kHeatmapPointsRounds - 1, und_count, und);
  hp_finish_kernel<<<1, 1024, 0, s>>>(a.heatmap, st, a.H, a.W, a.nms_dist, und_count, und);
  hp_kept_kernel<<<blocks, 256, 0, s>>>(a.heatmap, st, a.H, a.W, a.border, kept_count, kept_idx, kept_score);
  const int eblocks = (int)((n + 63) / 64);
  hp_emit_kernel<<<eblocks < 1024 ? eblocks : 1024, 256, 0, s>>>(a.heatmap, a.H, a.W, kept_count, kept_idx, kept_score, a.top_k, a.subpixel, a.pts, a.cap,
                                                           a.count);
  return hipGetLastError();
}

}  // namespace imx
