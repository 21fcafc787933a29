// mha_train.hip -- the attention of SuperGlue's GNN (superglue/models/superglue_train.py:82-86: einsum, softmax, einsum) in its training
// form, flash style on the fp32 matrix cores (include/imx_train.h).  Per (pair b, head h), scale = 1 / sqrt(D):
//
//   forward    S = scale Q^T K,  P = softmax_rows(S),  O = P V,  lse_i = log sum_j exp(S_ij)                      (one launch)
//   backward   delta_i = sum_c dO_ic O_ic                                                                       (one small launch)
//              P = exp(S - lse) recomputed,  dV = P^T dO,  dP = dO V^T,  dS = P o (dP - delta) scale,
//              dK = dS^T Q   per KEY block, query tiles ascending                                                (one launch, dK and dV)
//              dQ = dS K     per QUERY block, key tiles ascending                                                (one launch)
//
// The N x M matrices are never stored.  Tensors are read in place in the reference's own (B, D, H, n) layout: 32 consecutive keypoints
// of one channel are 128 contiguous bytes, which is what one half-wave of an operand of v_mfma_f32_32x32x2_f32 holds (A: lane l has
// [i = l & 31][k = l >> 5], B: [k = l >> 5][j = l & 31]); the accumulator has its column on the lane (l & 31) and row
// (r & 3) + 8 (r >> 2) + 4 (l >> 5) in register r.  Every product below is oriented so that the accumulator of one product is the B operand
// of the next with no lane movement (the summation index of a 32x32x2 step is then the row pair (r, hi = 0 | 1) of register r):
//
//   forward, dQ   query on the lane:  S^T = K^T.Q (A = K tile row, B = Q registers),  O^T += V.P^T,  dQ^T += K.dS^T (A = tile column)
//   dK, dV        key on the lane:    S = Q^T.K (A = Q tile row, B = K registers),    dV^T += dO.P,  dK^T += Q.dS   (A = tile column)
//
// A workgroup is 4 waves; a wave owns 32 queries (keys) and the workgroup walks the other side in tiles of 32, staged through LDS as
// [channel][33] images (row reads for the first products, column reads for the second ones), two buffers and one barrier per tile; the
// next tile's global loads are issued before this tile's products and wait in registers.  Loads are single dwords: a row of N
// floats is not 16-byte aligned when N % 4 != 0.
//
// Summation orders, all fixed at compile time and a function of the pair's own counts only: a 32-term MFMA chain per tile in the order
// of the registers, started from a zero accumulator, then one add into the running sum, tiles ascending (two levels: one running
// accumulator over a thousand non-negative P V terms sits twice as far from float64, attention.hip); the softmax denominator 16 in-lane
// adds, one cross-half add, then the running sum.  No floating-point atomics, no workgroup waits on another: equal inputs give equal bits
// whatever the batch, the padding, the grid or what the workspace held before.
//
// Ragged batches: queries past nq[b] and keys past nk[b] are never loaded (they are staged as zeros and their probabilities are selected
// to zero, so NaN there cannot leak); every output is written in full, with 0 there.
#include "mha_train.h"
#include "train_dev.h"

#include <math.h>

namespace imx {

namespace {

constexpr int TS = 33;                       // row stride of an LDS tile image [channel][32 keypoints]: column reads spread over the banks
constexpr int kWaves = 4, kBlock = 32 * kWaves;   // keypoints per workgroup on the side that owns the accumulators
constexpr float kLog2e = 1.4426950408889634f;

__device__ __forceinline__ float xhalf_max(float x) { return fmaxf(x, __shfl_xor(x, 32)); }
__device__ __forceinline__ float xhalf_sum(float x) { return x + __shfl_xor(x, 32); }

// One [D][32] tile, 128 contiguous bytes per channel, in two steps so that the next tile's loads fly during this tile's products:
// r[i] = src[c][n0 + j] for n0 + j < nvalid, else 0 (never loaded); then dst[c][j] = r[i]
template <int D>
__device__ __forceinline__ void load_tile(float (&r)[D / (2 * kWaves)], const float* src, size_t cs, int n0, int nvalid, int tid) {
#pragma unroll
  for (int i = 0; i < D / (2 * kWaves); ++i) {
    const int e = tid + i * 64 * kWaves, c = e >> 5, n = n0 + (e & 31);
    r[i] = n < nvalid ? src[(size_t)c * cs + n] : 0.f;
  }
}
template <int D>
__device__ __forceinline__ void store_tile(float* dst, const float (&r)[D / (2 * kWaves)], int tid) {
#pragma unroll
  for (int i = 0; i < D / (2 * kWaves); ++i) {
    const int e = tid + i * 64 * kWaves;
    dst[(e >> 5) * TS + (e & 31)] = r[i];
  }
}
// the operand of a product that sums over the tile's keypoints: lane holds tile[c = l31 + 32 cb][keypoint crow(r, hi)]; channels past D
// (head dimension 16: half of the 32-wide output block is padding) are zeros
template <int D>
__device__ __forceinline__ float tile_col(const float* t, int cb, int l31, int r, int hi) {
  const int c = l31 + 32 * cb;
  if (D % 32 == 0) return t[c * TS + crow(r, hi)];
  return c < D ? t[c * TS + crow(r, hi)] : 0.f;
}
// out[c][n0 .. n0 + kBlock) = 0 inside the frame, all channels: a workgroup whose whole block lies past the count
template <int D>
__device__ __forceinline__ void zero_block(float* out, size_t cs, int n0, int frame, int tid) {
  for (int e = tid; e < D * kBlock; e += 64 * kWaves) {
    const int c = e / kBlock, n = n0 + e % kBlock;
    if (n < frame) out[(size_t)c * cs + n] = 0.f;
  }
}
// acc[cb][r] is X^T[c = crow(r, hi) + 32 cb][n] of the lane's keypoint n: stores of one register are 128 contiguous bytes per half-wave
template <int D, int CB>
__device__ __forceinline__ void store_acc(float* out, size_t cs, int n, int frame, bool valid, const f32x16 (&acc)[CB], float f, int hi) {
  if (n >= frame) return;
#pragma unroll
  for (int cb = 0; cb < CB; ++cb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = crow(r, hi) + 32 * cb;
      if (c < D) out[(size_t)c * cs + n] = valid ? acc[cb][r] * f : 0.f;
    }
}

// ------------------------------------------------------------------------------------------------ forward
template <int D>
__global__ __launch_bounds__(64 * kWaves) void mha_fwd_kernel(MhaArgs a) {
  constexpr int CB = (D + 31) / 32;
  __shared__ float Kt[2][D * TS], Vt[2][D * TS];          // two buffers: one barrier per tile
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5, l31 = lane & 31;
  const int bh = blockIdx.y, b = bh / a.H, h = bh - b * a.H;
  const int nq = clampi(a.nq ? a.nq[b] : a.N, a.N), nk = clampi(a.nk ? a.nk[b] : a.M, a.M);
  const size_t csq = (size_t)a.H * a.N, csk = (size_t)a.H * a.M;
  const size_t qoff = ((size_t)b * D * a.H + h) * a.N, koff = ((size_t)b * D * a.H + h) * a.M;
  const int qb = blockIdx.x * kBlock, qi = qb + 32 * wave + l31;
  float* out = a.out + qoff;
  float* lse = a.lse ? a.lse + (size_t)bh * a.N : nullptr;
  if (nk == 0 || qb >= nq) {                 // block-uniform: nothing to attend to, or no query of this block is valid
    zero_block<D>(out, csq, qb, a.N, tid);
    if (lse && tid < kBlock && qb + tid < a.N) lse[qb + tid] = 0.f;
    return;
  }
  const bool qv = qi < nq;
  float qr[D / 2];
#pragma unroll
  for (int s = 0; s < D / 2; ++s) qr[s] = qv ? a.q[qoff + (size_t)(2 * s + hi) * csq + qi] : 0.f;
  f32x16 O[CB];
#pragma unroll
  for (int cb = 0; cb < CB; ++cb) O[cb] = zero16();
  float m = -INFINITY, l = 0.f;
  const int nt = (nk + 31) / 32;
  float kn[D / (2 * kWaves)], vn[D / (2 * kWaves)];          // the next tile, on its way
  load_tile<D>(kn, a.k + koff, csk, 0, nk, tid);
  load_tile<D>(vn, a.v + koff, csk, 0, nk, tid);
  for (int kt = 0; kt < nt; ++kt) {
    const int k0 = kt * 32;
    float* Ks = Kt[kt & 1];
    float* Vs = Vt[kt & 1];
    store_tile<D>(Ks, kn, tid);              // (this buffer was last read two tiles ago: every wave has passed a barrier since)
    store_tile<D>(Vs, vn, tid);
    __syncthreads();
    if (kt + 1 < nt) {
      load_tile<D>(kn, a.k + koff, csk, k0 + 32, nk, tid);
      load_tile<D>(vn, a.v + koff, csk, k0 + 32, nk, tid);
    }
    f32x16 S = zero16();
#pragma unroll
    for (int s = 0; s < D / 2; ++s) S = mma(Ks[(2 * s + hi) * TS + l31], qr[s], S);      // S[r] = Q_q . K_key, key = k0 + crow(r, hi)
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float x = k0 + crow(r, hi) < nk ? S[r] * a.scale : -INFINITY;
      S[r] = x;
      mx = fmaxf(mx, x);
    }
    mx = xhalf_max(mx);                      // finite: key k0 is valid
    const float mn = fmaxf(m, mx);
    const float alpha = __builtin_amdgcn_exp2f((m - mn) * kLog2e);                       // m = -inf on the first tile -> 0
    float rs = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float p = __builtin_amdgcn_exp2f((S[r] - mn) * kLog2e);                      // -inf -> 0
      S[r] = p;
      rs += p;
    }
    l = l * alpha + xhalf_sum(rs);
    m = mn;
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
      f32x16 T = zero16();
#pragma unroll
      for (int r = 0; r < 16; ++r) T = mma(tile_col<D>(Vs, cb, l31, r, hi), S[r], T);
#pragma unroll
      for (int r = 0; r < 16; ++r) O[cb][r] = O[cb][r] * alpha + T[r];
    }
  }
  store_acc<D, CB>(out, csq, qi, a.N, qv, O, 1.f / l, hi);
  if (lse && hi == 0 && qi < a.N) lse[qi] = qv ? m + logf(l) : 0.f;
}

// ------------------------------------------------------------------------------------------------ delta = rowsum(dO o O)
__global__ __launch_bounds__(256) void mha_delta_kernel(MhaArgs a) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= a.N) return;
  const int bh = blockIdx.y, b = bh / a.H, h = bh - b * a.H;
  const int nq = clampi(a.nq ? a.nq[b] : a.N, a.N);
  float d = 0.f;
  if (n < nq) {
    const size_t cs = (size_t)a.H * a.N, off = ((size_t)b * a.D * a.H + h) * a.N + n;
    for (int c = 0; c < a.D; ++c) d = fmaf(a.dout[off + c * cs], a.o_in[off + c * cs], d);      // channels ascending
  }
  a.delta[(size_t)bh * a.N + n] = d;
}

// ------------------------------------------------------------------------------------------------ dQ: per query block
template <int D>
__global__ __launch_bounds__(64 * kWaves) void mha_dq_kernel(MhaArgs a) {
  constexpr int CB = (D + 31) / 32;
  __shared__ float Kt[2][D * TS], Vt[2][D * TS];          // two buffers: one barrier per tile
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5, l31 = lane & 31;
  const int bh = blockIdx.y, b = bh / a.H, h = bh - b * a.H;
  const int nq = clampi(a.nq ? a.nq[b] : a.N, a.N), nk = clampi(a.nk ? a.nk[b] : a.M, a.M);
  const size_t csq = (size_t)a.H * a.N, csk = (size_t)a.H * a.M;
  const size_t qoff = ((size_t)b * D * a.H + h) * a.N, koff = ((size_t)b * D * a.H + h) * a.M;
  const int qb = blockIdx.x * kBlock, qi = qb + 32 * wave + l31;
  float* dq = a.dq + qoff;
  if (nk == 0 || qb >= nq) {
    zero_block<D>(dq, csq, qb, a.N, tid);
    return;
  }
  const bool qv = qi < nq;
  float qr[D / 2], gr[D / 2];                // Q and dO of the lane's query, channels 2 s + hi
#pragma unroll
  for (int s = 0; s < D / 2; ++s) {
    const size_t o = qoff + (size_t)(2 * s + hi) * csq + qi;
    qr[s] = qv ? a.q[o] : 0.f;
    gr[s] = qv ? a.dout[o] : 0.f;
  }
  const float lse = qv ? a.lse_in[(size_t)bh * a.N + qi] : 0.f, dl = qv ? a.delta[(size_t)bh * a.N + qi] : 0.f;
  f32x16 G[CB];
#pragma unroll
  for (int cb = 0; cb < CB; ++cb) G[cb] = zero16();
  const int nt = (nk + 31) / 32;
  float kn[D / (2 * kWaves)], vn[D / (2 * kWaves)];          // the next tile, on its way
  load_tile<D>(kn, a.k + koff, csk, 0, nk, tid);
  load_tile<D>(vn, a.v + koff, csk, 0, nk, tid);
  for (int kt = 0; kt < nt; ++kt) {
    const int k0 = kt * 32;
    float* Ks = Kt[kt & 1];
    float* Vs = Vt[kt & 1];
    store_tile<D>(Ks, kn, tid);              // (this buffer was last read two tiles ago: every wave has passed a barrier since)
    store_tile<D>(Vs, vn, tid);
    __syncthreads();
    if (kt + 1 < nt) {
      load_tile<D>(kn, a.k + koff, csk, k0 + 32, nk, tid);
      load_tile<D>(vn, a.v + koff, csk, k0 + 32, nk, tid);
    }
    f32x16 S = zero16(), P = zero16();
#pragma unroll
    for (int s = 0; s < D / 2; ++s) S = mma(Ks[(2 * s + hi) * TS + l31], qr[s], S);      // Q_q . K_key
#pragma unroll
    for (int s = 0; s < D / 2; ++s) P = mma(Vs[(2 * s + hi) * TS + l31], gr[s], P);      // dP = dO_q . V_key
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float p = k0 + crow(r, hi) < nk ? __builtin_amdgcn_exp2f(fmaf(S[r], a.scale, -lse) * kLog2e) : 0.f;
      S[r] = p * (P[r] - dl) * a.scale;      // dS
    }
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
      f32x16 T = zero16();
#pragma unroll
      for (int r = 0; r < 16; ++r) T = mma(tile_col<D>(Ks, cb, l31, r, hi), S[r], T);
      G[cb] += T;
    }
  }
  store_acc<D, CB>(dq, csq, qi, a.N, qv, G, 1.f, hi);
}

// ------------------------------------------------------------------------------------------------ dK, dV: per key block
template <int D>
__global__ __launch_bounds__(64 * kWaves) void mha_dkdv_kernel(MhaArgs a) {
  constexpr int CB = (D + 31) / 32;
  __shared__ float Qt[2][D * TS], Gt[2][D * TS], Lt[2][64];   // Q, dO, and lse | delta of the tile's 32 queries; two buffers
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5, l31 = lane & 31;
  const int bh = blockIdx.y, b = bh / a.H, h = bh - b * a.H;
  const int nq = clampi(a.nq ? a.nq[b] : a.N, a.N), nk = clampi(a.nk ? a.nk[b] : a.M, a.M);
  const size_t csq = (size_t)a.H * a.N, csk = (size_t)a.H * a.M;
  const size_t qoff = ((size_t)b * D * a.H + h) * a.N, koff = ((size_t)b * D * a.H + h) * a.M;
  const int kb = blockIdx.x * kBlock, ki = kb + 32 * wave + l31;
  const bool want_k = a.dk != nullptr, want_v = a.dv != nullptr;
  if (nq == 0 || kb >= nk) {
    if (want_k) zero_block<D>(a.dk + koff, csk, kb, a.M, tid);
    if (want_v) zero_block<D>(a.dv + koff, csk, kb, a.M, tid);
    return;
  }
  const bool kv = ki < nk;
  float kr[D / 2], vr[D / 2];                // K and V of the lane's key, channels 2 s + hi
#pragma unroll
  for (int s = 0; s < D / 2; ++s) {
    const size_t o = koff + (size_t)(2 * s + hi) * csk + ki;
    kr[s] = kv ? a.k[o] : 0.f;
    vr[s] = kv ? a.v[o] : 0.f;
  }
  f32x16 GK[CB], GV[CB];
#pragma unroll
  for (int cb = 0; cb < CB; ++cb) { GK[cb] = zero16(); GV[cb] = zero16(); }
  const float* lse = a.lse_in + (size_t)bh * a.N;
  const float* delta = a.delta + (size_t)bh * a.N;
  const int nt = (nq + 31) / 32;
  float qn[D / (2 * kWaves)], gn[D / (2 * kWaves)], ln = 0.f;   // the next tile, on its way (ln: lse on threads 0..31, delta on 32..63)
  const float* rowc = tid < 32 ? lse : delta;
  load_tile<D>(qn, a.q + qoff, csq, 0, nq, tid);
  load_tile<D>(gn, a.dout + qoff, csq, 0, nq, tid);
  if (tid < 64) ln = (tid & 31) < nq ? rowc[tid & 31] : 0.f;
  for (int qt = 0; qt < nt; ++qt) {
    const int q0 = qt * 32;
    float* Qs = Qt[qt & 1];
    float* Gs = Gt[qt & 1];
    const float* Ls = Lt[qt & 1];
    const float* Ds = Lt[qt & 1] + 32;
    store_tile<D>(Qs, qn, tid);
    store_tile<D>(Gs, gn, tid);
    if (tid < 64) Lt[qt & 1][tid] = ln;
    __syncthreads();
    if (qt + 1 < nt) {
      load_tile<D>(qn, a.q + qoff, csq, q0 + 32, nq, tid);
      load_tile<D>(gn, a.dout + qoff, csq, q0 + 32, nq, tid);
      if (tid < 64) ln = q0 + 32 + (tid & 31) < nq ? rowc[q0 + 32 + (tid & 31)] : 0.f;
    }
    f32x16 S = zero16(), P = zero16();
#pragma unroll
    for (int s = 0; s < D / 2; ++s) S = mma(Qs[(2 * s + hi) * TS + l31], kr[s], S);      // S[r] = Q_q . K_key, q = q0 + crow(r, hi)
#pragma unroll
    for (int s = 0; s < D / 2; ++s) P = mma(Gs[(2 * s + hi) * TS + l31], vr[s], P);      // dP = dO_q . V_key
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int qq = crow(r, hi);
      const float p = (kv && q0 + qq < nq) ? __builtin_amdgcn_exp2f(fmaf(S[r], a.scale, -Ls[qq]) * kLog2e) : 0.f;
      S[r] = p;
      P[r] = p * (P[r] - Ds[qq]) * a.scale;  // dS
    }
    if (want_v) {
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
        f32x16 T = zero16();
#pragma unroll
        for (int r = 0; r < 16; ++r) T = mma(tile_col<D>(Gs, cb, l31, r, hi), S[r], T);
        GV[cb] += T;
      }
    }
    if (want_k) {
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
        f32x16 T = zero16();
#pragma unroll
        for (int r = 0; r < 16; ++r) T = mma(tile_col<D>(Qs, cb, l31, r, hi), P[r], T);
        GK[cb] += T;
      }
    }
  }
  if (want_k) store_acc<D, CB>(a.dk + koff, csk, ki, a.M, kv, GK, 1.f, hi);
  if (want_v) store_acc<D, CB>(a.dv + koff, csk, ki, a.M, kv, GV, 1.f, hi);
}

}  // namespace

bool mha_head_dim_ok(int D) { return D == 16 || D == 32 || D == 64; }

#define IMX_MHA_DISPATCH(kernel, grid)                                                                        \
  switch (a.D) {                                                                                              \
    case 16: hipLaunchKernelGGL(kernel<16>, grid, dim3(64 * kWaves), 0, s, a); break;                         \
    case 32: hipLaunchKernelGGL(kernel<32>, grid, dim3(64 * kWaves), 0, s, a); break;                         \
    case 64: hipLaunchKernelGGL(kernel<64>, grid, dim3(64 * kWaves), 0, s, a); break;                         \
    default: return hipErrorInvalidValue;                                                                     \
  }                                                                                                           \
  return hipGetLastError();

hipError_t launch_mha_fwd(const MhaArgs& a, hipStream_t s) { IMX_MHA_DISPATCH(mha_fwd_kernel, dim3(cdiv(a.N, kBlock), a.B * a.H)) }
hipError_t launch_mha_dq(const MhaArgs& a, hipStream_t s) { IMX_MHA_DISPATCH(mha_dq_kernel, dim3(cdiv(a.N, kBlock), a.B * a.H)) }
hipError_t launch_mha_dkdv(const MhaArgs& a, hipStream_t s) { IMX_MHA_DISPATCH(mha_dkdv_kernel, dim3(cdiv(a.M, kBlock), a.B * a.H)) }
hipError_t launch_mha_delta(const MhaArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(mha_delta_kernel, dim3(cdiv(a.N, 256), a.B * a.H), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace imx
