// speval.hip -- kernels of libimx_speval.so (include/imx_speval.h): the mutual nearest-neighbour descriptor matcher
// and the pair metrics of SuperPoint's validation under a known warp.
//
// mnn_search: one direction of the search.  A workgroup of 256 threads owns 64 query rows of one pair and walks all key tiles of 64;
// four waves on 2 x 2 sub-tiles of 32 keys x 32 queries, products on v_mfma_f32_32x32x2_f32 in the structure of score_train.hip's
// score_da: per step one [64 keys][32 channels] and one [64 queries][32 channels] tile go through LDS as [row][33] images, two buffers,
// one barrier per step, the next step's global loads issued before this step's products.  The loads are predicated single dwords with
// 64-bit offsets, and the threads run along whichever index is contiguous in memory, so both the (B,D,N) layout and a transposed view
// of (B,K,D) are read in whole cache lines (with the key on the lane, as score_fwd reads, the second layout cost a cache line per lane
// and load: measured 0.23 ms per search at N = 1024, D = 128 whatever B).  The KEYS are the A operand and the QUERIES the B operand, so
// the query index lies on the accumulator's lane (train_dev.h: a lane holds column lane & 31, rows crow(r, hi)): every lane keeps a running (maximum, index)
// over the 16 keys it holds per tile, keys ascending, and nothing crosses lanes until the end, where the two half-waves and the two key
// waves of a query are combined through LDS -- the larger maximum first, then the lower index.  The similarity matrix is never stored.
//
// The sum over the channels is score_fwd's: chunks of 32 (16 MFMA steps, step s takes the channels 2 s and 2 s + 1), four chunks or
// what is left form one chain from a zero accumulator, chains added to the running sum in ascending order.  That order is a function
// of D alone, a product a b has the bits of b a, and both directions run this one kernel with the sides swapped: sim(i, j) has the
// same bits whichever side searches.  A NaN similarity never wins (every comparison with it is false).
//
// pair_metrics: one workgroup of 1024 threads per pair, every operation after the fp32 loads in float64 (as homog.hip).  H^-1 by the
// adjugate; both sides' positions IN IMAGE 1 are staged in LDS as float64 (side 0 warped by H, side 1 as it is), a point outside the
// shared view as NaN so that no comparison with it holds; then one pass over the rows and one over the columns of the implied distance
// matrix.  within_eps() is the only place that decides "within eps".  Sums: each thread adds its own points in ascending order, then a
// fixed tree over the 1024 threads; counts are integer LDS atomics.  No floating-point atomics, no workgroup waits on another.
#include "speval.h"
#include "imx_kernels.h"
#include "train_dev.h"

namespace imx {

namespace {

constexpr int kThreads = 256;                // 4 waves: 2 query halves x 2 key halves of a 64 x 64 tile
constexpr int TS = 33;                       // row stride of an LDS tile image [row][32 channels]: reads with the row on the lane spread over the banks
constexpr int kTileRegs = kSpevalTile * 32 / kThreads;   // floats per thread of one [64][32] tile

__device__ __forceinline__ bool closes_block(int chunk, int nchunks) { return (chunk & 3) == 3 || chunk == nchunks - 1; }

// Which (row, channel) of a [64 rows][32 channels] tile thread `tid` moves as its i-th element.  The index that is contiguous in memory
// runs along the threads: the channel where the channel stride is 1 (a (B,K,D) tensor seen through a transposed view: 128 contiguous
// bytes per 32 threads), else the row (a (B,D,N) tensor: 256 contiguous bytes per wave).  Either way the LDS image is [row][TS] and its
// writes are free of bank conflicts (33 row mod 64 is a permutation of the rows).
__device__ __forceinline__ void tile_slot(int tid, int i, bool channel_fast, int& row, int& col) {
  const int e = tid + i * kThreads;
  if (channel_fast) { row = e >> 5; col = e & 31; } else { row = e & 63; col = e >> 6; }
}

// rows [r0, r0 + 64) x channels [32 ch, 32 ch + 32) of one side of one pair into registers; nothing past the count or past D is read
__device__ __forceinline__ void load_tile(float (&r)[kTileRegs], const float* base, long long sc, long long sn, int r0, int count, int ch, int D,
                                          bool channel_fast, int tid) {
#pragma unroll
  for (int i = 0; i < kTileRegs; ++i) {
    int row, col;
    tile_slot(tid, i, channel_fast, row, col);
    const int n = r0 + row, d = ch * 32 + col;
    r[i] = (n < count && d < D) ? base[(long long)d * sc + (long long)n * sn] : 0.f;
  }
}

__device__ __forceinline__ void store_tile(float* dst, const float (&r)[kTileRegs], bool channel_fast, int tid) {
#pragma unroll
  for (int i = 0; i < kTileRegs; ++i) {
    int row, col;
    tile_slot(tid, i, channel_fast, row, col);
    dst[row * TS + col] = r[i];
  }
}

__global__ __launch_bounds__(kThreads) void mnn_search_kernel(MnnSearchArgs a, int nqb) {
  __shared__ float Kt[2][kSpevalTile * TS], Qt[2][kSpevalTile * TS];   // [64 keys][32 channels], [64 queries][32 channels]; two buffers
  __shared__ float cv[4][kSpevalTile];
  __shared__ int ci[4][kSpevalTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5, l31 = lane & 31, wq = wave >> 1, wk = wave & 1;
  const int b = blockIdx.x / nqb, q0 = (blockIdx.x % nqb) * kSpevalTile;
  const int cq = clampi(a.nq ? a.nq[b] : a.Nq, a.Nq), ck = clampi(a.nk ? a.nk[b] : a.Nk, a.Nk);
  if (q0 >= cq || ck == 0) {                 // block-uniform: no query row of this block is valid, or there is no key
    if (tid < kSpevalTile && q0 + tid < a.Nq) {
      a.nn[(size_t)b * a.Nq + q0 + tid] = -1;
      a.sim[(size_t)b * a.Nq + q0 + tid] = 0.f;
    }
    return;
  }
  const float* Q = a.q + (long long)b * a.qb;
  const float* K = a.k + (long long)b * a.kb;
  const bool qfast = a.qc == 1, kfast = a.kc == 1;      // block-uniform
  const int nch = (a.D + 31) / 32, total = ((ck + kSpevalTile - 1) / kSpevalTile) * nch;
  const bool q_live = q0 + 32 * wq < cq;     // wave-uniform: the wave's 32 queries hold a valid one
  float best = 0.f;
  int idx = -1;
  float kr[kTileRegs], qr[kTileRegs];        // the next step's tiles, on their way
  load_tile(kr, K, a.kc, a.kn, 0, ck, 0, a.D, kfast, tid);
  load_tile(qr, Q, a.qc, a.qn, q0, cq, 0, a.D, qfast, tid);
  f32x16 acc = zero16(), T = zero16();
  int t = 0, ch = 0;                         // the step's key tile and channel chunk: chunks inside tiles, both ascending
  for (int it = 0; it < total; ++it) {
    float* Ks = Kt[it & 1];
    float* Qs = Qt[it & 1];
    store_tile(Ks, kr, kfast, tid);          // (this buffer was last read two steps ago: every wave has passed a barrier since)
    store_tile(Qs, qr, qfast, tid);
    __syncthreads();
    if (it + 1 < total) {
      const int tn = ch + 1 < nch ? t : t + 1, cn = ch + 1 < nch ? ch + 1 : 0;
      load_tile(kr, K, a.kc, a.kn, tn * kSpevalTile, ck, cn, a.D, kfast, tid);
      load_tile(qr, Q, a.qc, a.qn, q0, cq, cn, a.D, qfast, tid);
    }
    const int kb = t * kSpevalTile + 32 * wk;            // the wave's 32 keys of this tile
    if (q_live && kb < ck) {                 // wave-uniform
      const float* krow = Ks + (32 * wk + l31) * TS + hi;
      const float* qrow = Qs + (32 * wq + l31) * TS + hi;
#pragma unroll
      for (int s = 0; s < 16; ++s) T = mma(krow[2 * s], qrow[2 * s], T);
      if (closes_block(ch, nch)) {
        acc += T;
        T = zero16();
      }
      if (ch == nch - 1) {                   // the tile's similarities are complete
#pragma unroll
        for (int r = 0; r < 16; ++r) {       // crow ascends with r: within a lane the keys come in ascending order, so > keeps the lowest
          const int key = kb + crow(r, hi);
          const float v = acc[r];
          if (key < ck && (v > best || (idx < 0 && v == v))) {
            best = v;
            idx = key;
          }
        }
        acc = zero16();
      }
    }
    if (++ch == nch) {
      ch = 0;
      ++t;
    }
  }
  cv[wk * 2 + hi][32 * wq + l31] = best;
  ci[wk * 2 + hi][32 * wq + l31] = idx;
  __syncthreads();
  if (tid >= kSpevalTile) return;
  const int q = q0 + tid;
  if (q >= a.Nq) return;
  float bvv = 0.f;
  int bi = -1;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float v = cv[c][tid];
    const int i = ci[c][tid];
    if (i >= 0 && (bi < 0 || v > bvv || (v == bvv && i < bi))) {
      bvv = v;
      bi = i;
    }
  }
  const bool ok = q < cq && bi >= 0;
  a.nn[(size_t)b * a.Nq + q] = ok ? bi : -1;
  a.sim[(size_t)b * a.Nq + q] = ok ? bvv : 0.f;
}

__global__ __launch_bounds__(256) void mnn_mutual_kernel(const int* __restrict__ nn0, const int* __restrict__ nn1, int B, int N0, int N1,
                                                         long long* __restrict__ m0, long long* __restrict__ m1) {
  const long long per = (long long)N0 + N1, e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= per * B) return;
  const int b = (int)(e / per), r = (int)(e % per);
  const int* a0 = nn0 + (size_t)b * N0;
  const int* a1 = nn1 + (size_t)b * N1;
  if (r < N0) {
    const int j = a0[r];
    m0[(size_t)b * N0 + r] = (j >= 0 && j < N1 && a1[j] == r) ? j : -1;
  } else {
    const int c = r - N0, i = a1[c];
    m1[(size_t)b * N1 + c] = (i >= 0 && i < N0 && a0[i] == c) ? i : -1;
  }
}

// ------------------------------------------------------------------------------------------------ the pair metrics
__device__ __forceinline__ double dist2(double dx, double dy) { return dx * dx + dy * dy; }
// THE within-eps decision of every count (r0, r1, c), on a squared distance
__device__ __forceinline__ bool within_eps(double d2, double eps) { return sqrt(d2) <= eps; }

// the sum of v over the workgroup in a fixed tree; every thread calls it
__device__ __forceinline__ double block_sum(double v, double* red, int tid) {
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int s = kSpevalMetricThreads / 2; s >= 1; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(kSpevalMetricThreads) void pair_metrics_kernel(PairMetricArgs a) {
  extern __shared__ double stage[];
  __shared__ double red[kSpevalMetricThreads];
  __shared__ double Hs[18];
  __shared__ int cnt[8];
  __shared__ int s_bad;
  constexpr int T = kSpevalMetricThreads;
  double* wx = stage;                        // side 0 in image 1 (warped), NaN = outside the shared view
  double* wy = wx + a.K0;
  double* px = wy + a.K0;                    // side 1 in image 1 (as it is), NaN = outside the shared view
  double* py = px + a.K1;
  const int tid = threadIdx.x, b = blockIdx.x;
  int* counts = a.counts + (size_t)b * 8;
  double* sums = a.sums + (size_t)b * 2;
  if (tid < 8) cnt[tid] = 0;
  if (tid == 0) {
    const double* H = a.H + (size_t)b * 9;
    double h[9], adj[9];
    for (int i = 0; i < 9; ++i) h[i] = H[i];
    adj[0] = h[4] * h[8] - h[5] * h[7]; adj[1] = h[2] * h[7] - h[1] * h[8]; adj[2] = h[1] * h[5] - h[2] * h[4];
    adj[3] = h[5] * h[6] - h[3] * h[8]; adj[4] = h[0] * h[8] - h[2] * h[6]; adj[5] = h[2] * h[3] - h[0] * h[5];
    adj[6] = h[3] * h[7] - h[4] * h[6]; adj[7] = h[1] * h[6] - h[0] * h[7]; adj[8] = h[0] * h[4] - h[1] * h[3];
    const double det = h[0] * adj[0] + h[1] * adj[3] + h[2] * adj[6];
    s_bad = !(det != 0.0 && fabs(det) < 1e300) ? 1 : 0;
    for (int i = 0; i < 9; ++i) {
      Hs[i] = h[i];
      Hs[9 + i] = adj[i] / det;
    }
  }
  __syncthreads();
  if (s_bad) {                               // block-uniform
    if (tid < 8) counts[tid] = tid == 6 ? 1 : 0;
    if (tid < 2) sums[tid] = 0.0;
    return;
  }
  const int n0 = clampi(a.n0 ? a.n0[b] : a.K0, a.K0), n1 = clampi(a.n1 ? a.n1[b] : a.K1, a.K1);
  const double xmax = (double)(a.width - 1), ymax = (double)(a.height - 1), eps = a.eps;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const float* k0 = a.kpts0 + (size_t)b * a.K0 * 2;
  const float* k1 = a.kpts1 + (size_t)b * a.K1 * 2;
  const long long* mt = a.matches0 ? a.matches0 + (size_t)b * a.K0 : nullptr;
  int lv = 0, lm = 0, lc = 0;
  for (int i = tid; i < n0; i += T) {
    const double x = (double)k0[2 * i], y = (double)k0[2 * i + 1];
    const double X = Hs[0] * x + Hs[1] * y + Hs[2], Y = Hs[3] * x + Hs[4] * y + Hs[5], W = Hs[6] * x + Hs[7] * y + Hs[8];
    const bool wpos = W > 0.0;
    const double u = X / W, v = Y / W;
    const bool vis = wpos && u >= 0.0 && u <= xmax && v >= 0.0 && v <= ymax;
    wx[i] = vis ? u : nan;
    wy[i] = vis ? v : nan;
    lv += vis ? 1 : 0;
    if (mt) {
      const long long j = mt[i];
      if (j >= 0 && j < n1) {
        ++lm;
        const double qx = (double)k1[2 * j], qy = (double)k1[2 * j + 1];
        if (wpos && within_eps(dist2(u - qx, v - qy), eps)) ++lc;
      }
    }
  }
  if (lv) atomicAdd(&cnt[0], lv);
  if (lm) atomicAdd(&cnt[4], lm);
  if (lc) atomicAdd(&cnt[5], lc);
  lv = 0;
  for (int j = tid; j < n1; j += T) {
    const double x = (double)k1[2 * j], y = (double)k1[2 * j + 1];
    const double X = Hs[9] * x + Hs[10] * y + Hs[11], Y = Hs[12] * x + Hs[13] * y + Hs[14], W = Hs[15] * x + Hs[16] * y + Hs[17];
    const double u = X / W, v = Y / W;
    const bool vis = W > 0.0 && u >= 0.0 && u <= xmax && v >= 0.0 && v <= ymax;
    px[j] = vis ? x : nan;
    py[j] = vis ? y : nan;
    lv += vis ? 1 : 0;
  }
  if (lv) atomicAdd(&cnt[1], lv);
  __syncthreads();
  // rows: every visible point of side 0 against the visible points of side 1 (a NaN position makes d2 NaN: never below best)
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  int lr = 0;
  double ls = 0.0;
  for (int i = tid; i < n0; i += T) {
    const double ux = wx[i], uy = wy[i];
    if (ux != ux) continue;
    double bd = inf;
    for (int j = 0; j < n1; ++j) {
      const double d2 = dist2(ux - px[j], uy - py[j]);
      if (d2 < bd) bd = d2;
    }
    if (within_eps(bd, eps)) {
      ++lr;
      ls += sqrt(bd);
    }
  }
  if (lr) atomicAdd(&cnt[2], lr);
  const double sum0 = block_sum(ls, red, tid);
  lr = 0;
  ls = 0.0;
  for (int j = tid; j < n1; j += T) {
    const double ux = px[j], uy = py[j];
    if (ux != ux) continue;
    double bd = inf;
    for (int i = 0; i < n0; ++i) {
      const double d2 = dist2(ux - wx[i], uy - wy[i]);
      if (d2 < bd) bd = d2;
    }
    if (within_eps(bd, eps)) {
      ++lr;
      ls += sqrt(bd);
    }
  }
  if (lr) atomicAdd(&cnt[3], lr);
  const double sum1 = block_sum(ls, red, tid);      // (its barriers also order the atomics above before the reads below)
  if (tid < 8) counts[tid] = tid < 6 ? cnt[tid] : 0;
  if (tid == 0) {
    sums[0] = sum0;
    sums[1] = sum1;
  }
}

}  // namespace

hipError_t launch_mnn_search(const MnnSearchArgs& a, hipStream_t s) {
  if (a.B <= 0 || a.Nq <= 0 || a.Nk <= 0 || a.D <= 0 || a.D > kSpevalMaxDim) return hipErrorInvalidValue;
  const int nqb = cdiv(a.Nq, kSpevalTile);
  if ((long long)nqb * a.B > 0x7fffffffll) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mnn_search_kernel, dim3((unsigned)(nqb * a.B)), dim3(kThreads), 0, s, a, nqb);
  return hipGetLastError();
}

hipError_t launch_mnn_mutual(const int* nn0, const int* nn1, int B, int N0, int N1, long long* matches0, long long* matches1, hipStream_t s) {
  if (B <= 0 || N0 <= 0 || N1 <= 0) return hipErrorInvalidValue;
  const long long blocks = (((long long)N0 + N1) * B + 255) / 256;
  if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mnn_mutual_kernel, dim3((unsigned)blocks), dim3(256), 0, s, nn0, nn1, B, N0, N1, matches0, matches1);
  return hipGetLastError();
}

hipError_t launch_pair_metrics(const PairMetricArgs& a, hipStream_t s) {
  if (a.B <= 0 || a.K0 <= 0 || a.K1 <= 0 || a.K0 > kSpevalMaxK || a.K1 > kSpevalMaxK) return hipErrorInvalidValue;
  static unsigned long long attr = 0;
  raise_lds_limit(reinterpret_cast<const void*>(pair_metrics_kernel), 2 * kSpevalMaxK * 2 * (int)sizeof(double), attr);
  hipLaunchKernelGGL(pair_metrics_kernel, dim3((unsigned)a.B), dim3(kSpevalMetricThreads), ((size_t)a.K0 + a.K1) * 2 * sizeof(double), s, a);
  return hipGetLastError();
}

}  // namespace imx
