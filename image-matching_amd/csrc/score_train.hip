// score_train.hip -- the score product of SuperGlue's training step, einsum('bdn,bdm->bnm', mdesc0, mdesc1) * scale, forward and backward on
// the fp32 matrix cores (include/imx_sgtrain.h).  Per pair b, with A = a[b] (D, N0), Bm = b[b] (D, N1), n0 and n1
// the pair's counts:
//
//   score_fwd   S[n][m]   = scale sum_d A[d][n] Bm[d][m]        workgroup: 64 rows n x 64 columns m        (i = n, j = m, k = d)
//   score_db    dBm[d][m] = scale sum_n dS[n][m] A[d][n]        workgroup: 64 channels d x 64 columns m    (i = d, j = m, k = n)
//   score_da    dA[d][n]  = scale sum_m dS[n][m] Bm[d][m]       workgroup: 64 channels d x 64 rows n       (i = d, j = n, k = m)
//
// The operand and accumulator lane layouts of v_mfma_f32_32x32x2_f32 are those at the top of lin_train.hip, and so is the structure: a
// 64 x 64 tile per workgroup of 256 threads, four waves on 2 x 2 sub-tiles of 32 x 32.  score_fwd reads both operands straight from
// global memory with the output index on the lane (128 contiguous bytes per half-wave) and uses no LDS and no barrier (lin_dx).  In
// score_db the A operand (A[d][n], d on the lane) is strided: a [64 d][32 n] tile goes through LDS as a [row][33] image, the B operand
// (dS[n][m], m on the lane) comes from global memory (lin_fwd).  In score_da the summation index m is the contiguous one of both
// operands: Bm[d][m] and dS[n][m] go through LDS as [64 d][33] and [64 n][33] images read by columns (lin_dw).  Where LDS is used: two
// buffers, one barrier per tile, the next tile's global loads issued before this tile's products.  Loads are single dwords (a row of
// N0 or N1 floats is not 16-byte aligned when the frame is no multiple of 4) and predicated: nothing past a count, past D or past the
// frame is ever loaded.  All offsets are 64-bit.
//
// Summation orders, fixed at compile time and a function of the pair's own counts only.  The summation index is cut into chunks of 32
// (16 MFMA steps, step s takes the indices 2 s and 2 s + 1); four chunks, or what is left of the last block, form one chain from a zero
// accumulator (a block of 128), which is then added to the running sum, blocks ascending; the running sum starts at +0.  score_fwd:
// the channel 0 .. D-1.  score_db: the row 0 .. n0-1.  score_da: the column 0 .. n1-1.  Blocks past the count are skipped, not added as
// zeros; the one multiply by scale is applied to the finished sum.  One workgroup forms the whole sum of its tile: no partial sums in
// memory, no scratch, no floating-point atomics, no workgroup waits on another.
#include "score_train.h"
#include "train_dev.h"

namespace imx {

namespace {

constexpr int TS = 33;                       // row stride of an LDS tile image [row][32]: reads with the row on the lane spread over the banks
constexpr int kThreads = 256;                // 4 waves, 2 x 2 sub-tiles of 32 x 32
constexpr int kTileRegs = kScoreTile * 32 / kThreads;   // floats per thread of one [64][32] tile

// a chunk closes its block of 128 when it is the block's fourth or the last of all
__device__ __forceinline__ bool closes_block(int chunk, int nchunks) { return (chunk & 3) == 3 || chunk == nchunks - 1; }

__device__ __forceinline__ void store_tile(float* dst, const float (&r)[kTileRegs], int tid) {
#pragma unroll
  for (int i = 0; i < kTileRegs; ++i) {
    const int e = tid + i * kThreads;
    dst[(e >> 5) * TS + (e & 31)] = r[i];
  }
}

// zeros over the part of a 64 x 64 tile at (r0, c0) that lies inside a (rows, cols) matrix of row stride cols
__device__ __forceinline__ void zero_tile(float* out, int r0, int c0, int rows, int cols, int tid) {
  for (int e = tid; e < kScoreTile * kScoreTile; e += kThreads) {
    const int r = r0 + e / kScoreTile, c = c0 + e % kScoreTile;
    if (r < rows && c < cols) out[(size_t)r * cols + c] = 0.f;
  }
}

// ------------------------------------------------------------------------------------------------ forward: no LDS, no barrier
__global__ __launch_bounds__(kThreads) void score_fwd_kernel(ScoreTrainArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5, l31 = lane & 31, wn = wave >> 1, wm = wave & 1;
  const int b = blockIdx.z;
  const int c0 = clampi(a.n0 ? a.n0[b] : a.N0, a.N0), c1 = clampi(a.n1 ? a.n1[b] : a.N1, a.N1);
  float* S = a.s + (size_t)b * a.N0 * a.N1;
  if ((int)blockIdx.y * kScoreTile >= c0 || (int)blockIdx.x * kScoreTile >= c1) {   // block-uniform: no element of this tile is valid
    zero_tile(S, blockIdx.y * kScoreTile, blockIdx.x * kScoreTile, a.N0, a.N1, tid);
    return;
  }
  const int nb = blockIdx.y * kScoreTile + 32 * wn, mb = blockIdx.x * kScoreTile + 32 * wm;     // the wave's 32 x 32 sub-tile
  const int n = nb + l31, m = mb + l31;      // the lane's row as an A operand, its column as a B operand and in the accumulator
  const bool nv = n < c0, mv = m < c1;
  f32x16 acc = zero16();
  if (nb < c0 && mb < c1) {                  // wave-uniform
    const int nch = (a.D + 31) / 32;
    const float* A = a.a + (size_t)b * a.D * a.N0;
    const float* Bm = a.b + (size_t)b * a.D * a.N1;
    float av[16], bv[16], an[16] = {}, bn[16] = {};   // this chunk's operands and the next chunk's, on their way
    auto load = [&](float (&va)[16], float (&vb)[16], int ch) {
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const int d = ch * 32 + 2 * s + hi;
        va[s] = (nv && d < a.D) ? A[(size_t)d * a.N0 + n] : 0.f;
        vb[s] = (mv && d < a.D) ? Bm[(size_t)d * a.N1 + m] : 0.f;
      }
    };
    load(av, bv, 0);
    f32x16 T = zero16();
    for (int ch = 0; ch < nch; ++ch) {
      if (ch + 1 < nch) load(an, bn, ch + 1);
#pragma unroll
      for (int s = 0; s < 16; ++s) T = mma(av[s], bv[s], T);
      if (closes_block(ch, nch)) {
        acc += T;
        T = zero16();
      }
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        av[s] = an[s];
        bv[s] = bn[s];
      }
    }
  }
  if (m >= a.N1) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = nb + crow(r, hi);
    if (row < a.N0) S[(size_t)row * a.N1 + m] = (mv && row < c0) ? a.scale * acc[r] : 0.f;
  }
}

// ------------------------------------------------------------------------------------------------ db: A[d][n] through LDS, dS[n][m] from global memory
__global__ __launch_bounds__(kThreads) void score_db_kernel(ScoreTrainArgs a) {
  __shared__ float At[2][kScoreTile * TS];                  // [64 d][32 n] of A, two buffers: one barrier per chunk
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5, l31 = lane & 31, wd = wave >> 1, wm = wave & 1;
  const int b = blockIdx.z, d0 = blockIdx.y * kScoreTile, m0 = blockIdx.x * kScoreTile;
  const int c0 = clampi(a.n0 ? a.n0[b] : a.N0, a.N0), c1 = clampi(a.n1 ? a.n1[b] : a.N1, a.N1);
  float* dB = a.db + (size_t)b * a.D * a.N1;
  if (m0 >= c1 || c0 == 0) {                 // block-uniform: no column of this tile is valid, or the sum is empty
    zero_tile(dB, d0, m0, a.D, a.N1, tid);
    return;
  }
  const float* A = a.a + (size_t)b * a.D * a.N0;
  const float* dS = a.ds + (size_t)b * a.N0 * a.N1;
  const int m = m0 + 32 * wm + l31;
  const bool mv = m < c1;
  const int nch = (c0 + 31) / 32;
  float ar[kTileRegs], bv[16], bn[16] = {};  // the next A tile and this / the next chunk's rows of dS, on their way
  auto load_a = [&](int ch) {
#pragma unroll
    for (int i = 0; i < kTileRegs; ++i) {
      const int e = tid + i * kThreads, d = d0 + (e >> 5), n = ch * 32 + (e & 31);
      ar[i] = (d < a.D && n < c0) ? A[(size_t)d * a.N0 + n] : 0.f;
    }
  };
  auto load_b = [&](float (&v)[16], int ch) {
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const int n = ch * 32 + 2 * s + hi;
      v[s] = (mv && n < c0) ? dS[(size_t)n * a.N1 + m] : 0.f;
    }
  };
  load_a(0);
  load_b(bv, 0);
  f32x16 acc = zero16(), T = zero16();
  for (int ch = 0; ch < nch; ++ch) {
    float* As = At[ch & 1];
    store_tile(As, ar, tid);                 // (this buffer was last read two chunks ago: every wave has passed a barrier since)
    __syncthreads();
    if (ch + 1 < nch) {
      load_a(ch + 1);
      load_b(bn, ch + 1);
    }
    const float* arow = As + (32 * wd + l31) * TS + hi;
#pragma unroll
    for (int s = 0; s < 16; ++s) T = mma(arow[2 * s], bv[s], T);
    if (closes_block(ch, nch)) {
      acc += T;
      T = zero16();
    }
#pragma unroll
    for (int s = 0; s < 16; ++s) bv[s] = bn[s];
  }
  if (m >= a.N1) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int d = d0 + 32 * wd + crow(r, hi);
    if (d < a.D) dB[(size_t)d * a.N1 + m] = mv ? a.scale * acc[r] : 0.f;
  }
}

// ------------------------------------------------------------------------------------------------ da: Bm[d][m] and dS[n][m] through LDS
__global__ __launch_bounds__(kThreads) void score_da_kernel(ScoreTrainArgs a) {
  __shared__ float Bt[2][kScoreTile * TS], St[2][kScoreTile * TS];   // [64 d][32 m] of Bm, [64 n][32 m] of dS; two buffers
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5, l31 = lane & 31, wd = wave >> 1, wn = wave & 1;
  const int b = blockIdx.z, d0 = blockIdx.y * kScoreTile, r0 = blockIdx.x * kScoreTile;
  const int c0 = clampi(a.n0 ? a.n0[b] : a.N0, a.N0), c1 = clampi(a.n1 ? a.n1[b] : a.N1, a.N1);
  float* dA = a.da + (size_t)b * a.D * a.N0;
  if (r0 >= c0 || c1 == 0) {                 // block-uniform: no row of this tile is valid, or the sum is empty
    zero_tile(dA, d0, r0, a.D, a.N0, tid);
    return;
  }
  const float* Bm = a.b + (size_t)b * a.D * a.N1;
  const float* dS = a.ds + (size_t)b * a.N0 * a.N1;
  const int nt = (c1 + 31) / 32;
  float br[kTileRegs], sr[kTileRegs];        // the next tile, on its way
  auto load = [&](int t) {
#pragma unroll
    for (int i = 0; i < kTileRegs; ++i) {
      const int e = tid + i * kThreads, row = e >> 5, m = t * 32 + (e & 31), d = d0 + row, n = r0 + row;
      const bool mv = m < c1;
      br[i] = (mv && d < a.D) ? Bm[(size_t)d * a.N1 + m] : 0.f;
      sr[i] = (mv && n < c0) ? dS[(size_t)n * a.N1 + m] : 0.f;
    }
  };
  load(0);
  f32x16 acc = zero16(), T = zero16();
  for (int t = 0; t < nt; ++t) {
    float* Bs = Bt[t & 1];
    float* Ss = St[t & 1];
    store_tile(Bs, br, tid);                 // (this buffer was last read two tiles ago: every wave has passed a barrier since)
    store_tile(Ss, sr, tid);
    __syncthreads();
    if (t + 1 < nt) load(t + 1);
    const float* brow = Bs + (32 * wd + l31) * TS + hi;
    const float* srow = Ss + (32 * wn + l31) * TS + hi;
#pragma unroll
    for (int s = 0; s < 16; ++s) T = mma(brow[2 * s], srow[2 * s], T);
    if (closes_block(t, nt)) {
      acc += T;
      T = zero16();
    }
  }
  const int n = r0 + 32 * wn + l31;
  if (n >= a.N0) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int d = d0 + 32 * wd + crow(r, hi);
    if (d < a.D) dA[(size_t)d * a.N0 + n] = n < c0 ? a.scale * acc[r] : 0.f;
  }
}

}  // namespace

hipError_t launch_score_fwd(const ScoreTrainArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(score_fwd_kernel, dim3(cdiv(a.N1, kScoreTile), cdiv(a.N0, kScoreTile), a.B), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_score_da(const ScoreTrainArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(score_da_kernel, dim3(cdiv(a.N0, kScoreTile), cdiv(a.D, kScoreTile), a.B), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_score_db(const ScoreTrainArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(score_db_kernel, dim3(cdiv(a.N1, kScoreTile), cdiv(a.D, kScoreTile), a.B), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace imx
