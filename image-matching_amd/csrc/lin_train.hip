// lin_train.hip -- nn.Conv1d(kernel_size=1) on torch.cat([x0, x1], 1) in its training form on the fp32 matrix cores
// (include/imx_train.h).  Per pair b, with xcat the concatenation of x0 and x1 over channels, Cin = C0 + C1:
//
//   lin_fwd         y[o][n]  = bias[o] + sum_c w[o][c] xcat[c][n]          workgroup: 64 output channels x 64 columns
//   lin_dx          dx[c][n] = sum_o w[o][c] dy[o][n]                      workgroup: 64 input channels x 64 columns
//   lin_dw          part[b][slab][o][c] = sum_{n in slab} dy[o][n] xcat[c][n],  c = Cin: the ones row, which gives db
//                                                                          workgroup: 64 x 64 channels, one pair, one slab of 256 columns
//   lin_dw_reduce   dw[o][c] = sum_b (sum_slab part), db[o] likewise       one thread per element, slabs then pairs ascending
//
// Operands of v_mfma_f32_32x32x2_f32: A lane l holds [i = l & 31][k = l >> 5], B [k = l >> 5][j = l & 31]; the accumulator has its column
// on the lane (l & 31) and row (r & 3) + 8 (r >> 2) + 4 (l >> 5) in register r.  With the column n on the lane, the B operands of lin_fwd
// (xcat[c][n]) and lin_dx (dy[o][n]) are 128 contiguous bytes per half-wave straight from global memory, and so is the A operand of
// lin_dx (i = c, k = o: w[o][c]).  The A operand of lin_fwd (w[o][c], o on the lane) is strided: a [64 o][32 c] tile goes through LDS
// as a [row][33] image.  In lin_dw the summation index is the column, so both operands are [channel][33] images of 32 columns read
// by columns.  Two LDS buffers and one barrier per tile; the next tile's global loads are issued before this tile's products and wait
// in registers.  Loads are single dwords (a row of N floats is not 16-byte aligned when N % 4 != 0, a row of w not when Cin % 4 != 0)
// and predicated: nothing past a count, a channel count or the frame is ever loaded.
//
// Summation orders, fixed at compile time and a function of the counts only.  The summation index is cut into chunks of 32 (16 MFMA
// steps, step s takes the indices 2 s and 2 s + 1); four chunks, or what is left of the last block, form one chain from a zero
// accumulator (a block of 128), which is then added to the running sum, blocks ascending; the running sum starts at +0.  lin_fwd: the
// concatenated input channel, then the bias.  lin_dx: the output channel.  lin_dw: the columns of one slab (two blocks), chunks past
// the pair's count skipped; lin_dw_reduce adds a pair's slabs ascending from +0 (slabs past the count skipped), then the pairs ascending
// from +0 (pairs of count 0 skipped).  No floating-point atomics, no workgroup waits on another.
#include "lin_train.h"
#include "train_dev.h"

namespace imx {

namespace {

constexpr int TS = 33;                       // row stride of an LDS tile image [row][32]: reads with the row on the lane spread over the banks
constexpr int kThreads = 256;                // 4 waves, 2 x 2 sub-tiles of 32 x 32
constexpr int kTileRegs = kLinTile * 32 / kThreads;   // floats per thread of one [64][32] tile

// a chunk closes its block of 128 when it is the block's fourth or the last of all
__device__ __forceinline__ bool closes_block(int chunk, int nchunks) { return (chunk & 3) == 3 || chunk == nchunks - 1; }

// row c of the concatenation of pair b, or null past it
__device__ __forceinline__ const float* xcat_row(const LinArgs& a, int b, int c) {
  if (c < a.C0) return a.x0 + ((size_t)b * a.C0 + c) * a.N;
  if (c < a.C0 + a.C1) return a.x1 + ((size_t)b * a.C1 + (c - a.C0)) * a.N;
  return nullptr;
}

__device__ __forceinline__ void store_tile(float* dst, const float (&r)[kTileRegs], int tid) {
#pragma unroll
  for (int i = 0; i < kTileRegs; ++i) {
    const int e = tid + i * kThreads;
    dst[(e >> 5) * TS + (e & 31)] = r[i];
  }
}

// ------------------------------------------------------------------------------------------------ forward
__global__ __launch_bounds__(kThreads) void lin_fwd_kernel(LinArgs a) {
  __shared__ float Wt[2][kLinTile * TS];                    // [64 o][32 c] of w, two buffers: one barrier per chunk
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5, l31 = lane & 31, wo = wave >> 1, wn = wave & 1;
  const int b = blockIdx.z, o0 = blockIdx.y * kLinTile, n0 = blockIdx.x * kLinTile, Cin = a.C0 + a.C1;
  const int cnt = clampi(a.n ? a.n[b] : a.N, a.N);
  float* y = a.y + (size_t)b * a.Cout * a.N;
  if (n0 >= cnt) {                           // block-uniform: no column of this tile is valid
    for (int e = tid; e < kLinTile * kLinTile; e += kThreads) {
      const int o = o0 + e / kLinTile, n = n0 + e % kLinTile;
      if (o < a.Cout && n < a.N) y[(size_t)o * a.N + n] = 0.f;
    }
    return;
  }
  const int n = n0 + 32 * wn + l31;
  const bool nv = n < cnt;
  const int nch = (Cin + 31) / 32;
  float wr[kTileRegs], bv[16], bn[16] = {};  // the next w tile and this / the next chunk's columns, on their way
  auto load_w = [&](int ch) {
#pragma unroll
    for (int i = 0; i < kTileRegs; ++i) {
      const int e = tid + i * kThreads, o = o0 + (e >> 5), c = ch * 32 + (e & 31);
      wr[i] = (o < a.Cout && c < Cin) ? a.w[(size_t)o * Cin + c] : 0.f;
    }
  };
  auto load_b = [&](float (&v)[16], int ch) {
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const float* row = xcat_row(a, b, ch * 32 + 2 * s + hi);
      v[s] = (nv && row) ? row[n] : 0.f;
    }
  };
  load_w(0);
  load_b(bv, 0);
  f32x16 acc = zero16(), T = zero16();
  for (int ch = 0; ch < nch; ++ch) {
    float* Ws = Wt[ch & 1];
    store_tile(Ws, wr, tid);                 // (this buffer was last read two chunks ago: every wave has passed a barrier since)
    __syncthreads();
    if (ch + 1 < nch) {
      load_w(ch + 1);
      load_b(bn, ch + 1);
    }
    const float* wrow = Ws + (32 * wo + l31) * TS + hi;
#pragma unroll
    for (int s = 0; s < 16; ++s) T = mma(wrow[2 * s], bv[s], T);
    if (closes_block(ch, nch)) {
      acc += T;
      T = zero16();
    }
#pragma unroll
    for (int s = 0; s < 16; ++s) bv[s] = bn[s];
  }
  if (n >= a.N) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int o = o0 + 32 * wo + crow(r, hi);
    if (o < a.Cout) y[(size_t)o * a.N + n] = nv ? acc[r] + (a.bias ? a.bias[o] : 0.f) : 0.f;
  }
}

// ------------------------------------------------------------------------------------------------ dx: no LDS, no barrier
__global__ __launch_bounds__(kThreads) void lin_dx_kernel(LinArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5, l31 = lane & 31, wc = wave >> 1, wn = wave & 1;
  const int b = blockIdx.z, Cin = a.C0 + a.C1;
  const int c0 = blockIdx.y * kLinTile + 32 * wc, n0 = blockIdx.x * kLinTile + 32 * wn;     // the wave's 32 x 32 sub-tile
  // wave-uniform: the sub-tile holds no channel of a wanted output
  if (c0 >= Cin || !((a.dx0 && c0 < a.C0) || (a.dx1 && c0 + 32 > a.C0))) return;
  const int cnt = clampi(a.n ? a.n[b] : a.N, a.N);
  const int n = n0 + l31, ci = c0 + l31;
  const bool nv = n < cnt, cv = ci < Cin;
  f32x16 acc = zero16();
  if (n0 < cnt) {                            // wave-uniform
    const int nch = (a.Cout + 31) / 32;
    const float* dy = a.dy + (size_t)b * a.Cout * a.N;
    float av[16], bv[16], an[16] = {}, bn[16] = {};   // this chunk's operands and the next chunk's, on their way
    auto load = [&](float (&va)[16], float (&vb)[16], int ch) {
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const int o = ch * 32 + 2 * s + hi;
        va[s] = (cv && o < a.Cout) ? a.w[(size_t)o * Cin + ci] : 0.f;
        vb[s] = (nv && o < a.Cout) ? dy[(size_t)o * a.N + n] : 0.f;
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
  if (n >= a.N) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int c = c0 + crow(r, hi);
    float* row = nullptr;
    if (c < a.C0) row = a.dx0 ? a.dx0 + ((size_t)b * a.C0 + c) * a.N : nullptr;
    else if (c < Cin) row = a.dx1 ? a.dx1 + ((size_t)b * a.C1 + (c - a.C0)) * a.N : nullptr;
    if (row) row[n] = nv ? acc[r] : 0.f;
  }
}

// ------------------------------------------------------------------------------------------------ dw, db: per (pair, slab) partials
__global__ __launch_bounds__(kThreads) void lin_dw_kernel(LinArgs a, int ct0, int nct) {
  __shared__ float Dt[2][kLinTile * TS], Xt[2][kLinTile * TS];   // [64 o][32 n] of dy, [64 c][32 n] of xcat and the ones row; two buffers
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5, l31 = lane & 31, wo = wave >> 1, wc = wave & 1;
  const int b = blockIdx.z, slab = blockIdx.y, Cin = a.C0 + a.C1, P = Cin + 1;
  const int o0 = (blockIdx.x / nct) * kLinTile, c0 = (ct0 + blockIdx.x % nct) * kLinTile;
  const int cnt = clampi(a.n ? a.n[b] : a.N, a.N);
  const int s0 = slab * kLinSlab;
  float* part = a.part + ((size_t)b * gridDim.y + slab) * a.Cout * P;
  if (s0 >= cnt) {                           // block-uniform: the slab lies past the count; lin_dw_reduce skips it, the scratch is still written
    for (int e = tid; e < kLinTile * kLinTile; e += kThreads) {
      const int o = o0 + e / kLinTile, c = c0 + e % kLinTile;
      if (o < a.Cout && c < P) part[(size_t)o * P + c] = 0.f;
    }
    return;
  }
  const int send = min(cnt, s0 + kLinSlab), nt = (send - s0 + 31) / 32;
  const bool active = c0 + 32 * wc < P;      // wave-uniform: the sub-tile holds a channel or the ones row
  const float* dy = a.dy + (size_t)b * a.Cout * a.N;
  float dr[kTileRegs], xr[kTileRegs];        // the next tile, on its way
  auto load = [&](int t) {
#pragma unroll
    for (int i = 0; i < kTileRegs; ++i) {
      const int e = tid + i * kThreads, ch = e >> 5, n = s0 + t * 32 + (e & 31), o = o0 + ch, c = c0 + ch;
      const bool nv = n < send;
      dr[i] = (nv && o < a.Cout) ? dy[(size_t)o * a.N + n] : 0.f;
      const float* row = xcat_row(a, b, c);
      xr[i] = !nv ? 0.f : row ? row[n] : (c == Cin && a.db) ? 1.f : 0.f;
    }
  };
  load(0);
  f32x16 acc = zero16(), T = zero16();
  for (int t = 0; t < nt; ++t) {
    float* Ds = Dt[t & 1];
    float* Xs = Xt[t & 1];
    store_tile(Ds, dr, tid);                 // (this buffer was last read two tiles ago: every wave has passed a barrier since)
    store_tile(Xs, xr, tid);
    __syncthreads();
    if (t + 1 < nt) load(t + 1);
    if (active) {
      const float* drow = Ds + (32 * wo + l31) * TS + hi;
      const float* xrow = Xs + (32 * wc + l31) * TS + hi;
#pragma unroll
      for (int s = 0; s < 16; ++s) T = mma(drow[2 * s], xrow[2 * s], T);
      if (closes_block(t, nt)) {
        acc += T;
        T = zero16();
      }
    }
  }
  const int c = c0 + 32 * wc + l31;
  if (c >= P) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int o = o0 + 32 * wo + crow(r, hi);
    if (o < a.Cout) part[(size_t)o * P + c] = acc[r];
  }
}

__global__ __launch_bounds__(kThreads) void lin_dw_reduce_kernel(LinArgs a, int c_first, int slabs) {
  const int Cin = a.C0 + a.C1, P = Cin + 1, c = c_first + blockIdx.x * kThreads + threadIdx.x, o = blockIdx.y;
  if (c >= P || (c < Cin ? a.dw == nullptr : a.db == nullptr)) return;
  float total = 0.f;
  for (int b = 0; b < a.B; ++b) {
    const int cnt = clampi(a.n ? a.n[b] : a.N, a.N), ns = (cnt + kLinSlab - 1) / kLinSlab;
    if (ns == 0) continue;                   // an empty pair adds nothing, not even a zero
    const float* p = a.part + ((size_t)b * slabs * a.Cout + o) * P + c;
    float pair = 0.f;
    for (int s = 0; s < ns; ++s) pair += p[(size_t)s * a.Cout * P];
    total += pair;
  }
  if (c < Cin) a.dw[(size_t)o * Cin + c] = total;
  else a.db[o] = total;
}

}  // namespace

hipError_t launch_lin_fwd(const LinArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(lin_fwd_kernel, dim3(cdiv(a.N, kLinTile), cdiv(a.Cout, kLinTile), a.B), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_lin_dx(const LinArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(lin_dx_kernel, dim3(cdiv(a.N, kLinTile), cdiv(a.C0 + a.C1, kLinTile), a.B), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

// with dw unwanted only the channel tile that holds the ones row (index Cin) runs
hipError_t launch_lin_dw(const LinArgs& a, hipStream_t s) {
  const int Cin = a.C0 + a.C1, ct0 = a.dw ? 0 : Cin / kLinTile, nct = (a.dw ? cdiv(Cin + (a.db ? 1 : 0), kLinTile) : Cin / kLinTile + 1) - ct0;
  hipLaunchKernelGGL(lin_dw_kernel, dim3(nct * cdiv(a.Cout, kLinTile), lin_slabs(a.N), a.B), dim3(kThreads), 0, s, a, ct0, nct);
  return hipGetLastError();
}

hipError_t launch_lin_dw_reduce(const LinArgs& a, hipStream_t s) {
  const int Cin = a.C0 + a.C1, c_first = a.dw ? 0 : Cin, c_end = a.db ? Cin + 1 : Cin;
  hipLaunchKernelGGL(lin_dw_reduce_kernel, dim3(cdiv(c_end - c_first, kThreads), a.Cout), dim3(kThreads), 0, s, a, c_first, lin_slabs(a.N));
  return hipGetLastError();
}

}  // namespace imx
