// conv3_train.hip -- nn.Conv2d(Cin, Cout, 3, padding=1) (stride 1, no dilation, no groups) in its training form on the fp32 matrix cores
// (include/imx_spnet.h), on the reference's own NCHW tensors: x (B,Cin,H,W), w (Cout,Cin,3,3), y and dy (B,Cout,H,W).
//
//   conv3<false>    y[b][o][i][j]  = bias[o] + sum_c sum_uv w[o][c][u][v] x[b][c][i+u-1][j+v-1]      workgroup: 64 channels x 8 rows x 32 columns
//   conv3<true>     dx[b][c][i][j] = sum_o sum_uv w[o][c][2-u][2-v] dy[b][o][i+u-1][j+v-1]           the same kernel: flipped taps, o and c exchanged
//   conv3_dw        part[b][slab][o][9 c + 3 u + v] = sum_{(i,j) in slab} dy[b][o][i][j] x[b][c][i+u-1][j+v-1];  column 9 Cin: the ones
//                   column, which gives db                                workgroup: 64 x 64 of (o, column), one image, one slab of 16 rows
//   conv3_dw_reduce dw[o][c][u][v] = sum_b (sum_slab part), db[o] likewise                           one thread per element
//
// Operands of v_mfma_f32_32x32x2_f32: A lane l holds [i = l & 31][k = l >> 5], B [k = l >> 5][j = l & 31]; the accumulator has its column
// on the lane (l & 31) and row crow(r, l >> 5) in register r (train_dev.h).
//
// conv3<>: the output channel is the accumulator's row, the image column its column, so lanes walk W: the pixel operand of a (tap, row) is
// 32 consecutive floats of one halo row, the weight operand 32 consecutive output channels of one (tap, summation channel).  The two
// summation indices of an MFMA step are two channels (2 s and 2 s + 1 of the chunk) at the same tap.  A chunk of 8 summation channels goes
// through LDS: its halo tile [8][10][34] and its weights [9 taps][4 pairs][2 blocks of 32 channels][2][32], laid out so that every LDS read
// has consecutive lanes on consecutive words.  Two buffers, one barrier per chunk; the next chunk's global loads are issued before this
// chunk's products and wait in registers.  A wave owns 2 image rows x 64 output channels: 2 x 2 accumulators of 32 x 32, so every weight
// operand read from LDS feeds two MFMAs (two rows) and every pixel operand two to four (two channel blocks, and the one or two (row, u)
// pairs that meet on one halo row).  Loads are single dwords and predicated on the image, the tile and the channel count: W % 4 != 0 leaves rows
// unaligned, and nothing outside a tensor is ever addressed.  Every offset is 64-bit.
//
// conv3_dw: the pixel is the summation index, so both operands are [channel][33] LDS images of 32 pixels read by columns, as in
// lin_train.hip's lin_dw; the x image is gathered tap by tap (im2col on the fly, predicated at the image border).  A slab's pixels are
// walked in row-major order as one flat run of min(16, H - 16 slab) W pixels.
//
// Summation orders, fixed at compile time and a function of (B, Cin, Cout, H, W) only.  conv3<>: the summation channels are cut into
// chunks of 8; inside a chunk the pairs s = 0..3 ascend, inside a pair the taps (u, v) in row-major order; two chunks, or the last one
// alone, form one MFMA chain of 72 steps (36) from a zero accumulator, which is then added to the running sum, chains ascending; the
// running sum starts at +0; conv3<false> adds the bias (or +0) last.  (This is not lin_train.hip's order: its chains are 64 steps, blocks
// of 128 summation indices, which no whole number of channels times nine taps gives.)  conv3_dw: a slab's pixels in chunks of 32
// (16 MFMA steps, step s takes the pixels 2 s and 2 s + 1); four chunks, or what is left, form one chain of 64 steps, added to the running sum from +0.
// conv3_dw_reduce adds an image's slabs ascending from +0, then the images ascending from +0.  No floating-point atomics, no workgroup
// waits on another.
#include "conv3_train.h"
#include "train_dev.h"

#include <algorithm>

namespace imx {

namespace {

constexpr int kThreads = 256;                                  // 4 waves
constexpr int HR = kC3Rows + 2, XS = kC3Cols + 2;              // halo rows and columns of the pixel tile
constexpr int kXFloats = kC3Chunk * HR * XS;                   // 2720: one chunk's halo tile [8][10][34]
constexpr int kWFloats = 9 * kC3Chunk * kC3Chan;               // 4608: one chunk's weights
constexpr int kXRegs = HR + 1;                                 // 11: ten rows of one column, and one value of the last two columns
constexpr int kWRegs = kWFloats / kThreads;                    // 18: two channels x nine taps
static_assert(kWRegs == 18 && kThreads == 32 * kC3Chunk && kThreads == 4 * kC3Chan && kC3Rows == 8 && kC3Cols == 32 && kC3Chan == 64 && kC3Chunk == 8, "the index arithmetic below assumes these");

// ------------------------------------------------------------------------------------------------ forward (FLIP = false), dx (FLIP = true)
template <bool FLIP>
__global__ __launch_bounds__(kThreads) void conv3_kernel(Conv3Args a) {
  __shared__ float Xs[2][kXFloats];
  __shared__ float Ws[2][kWFloats];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5, l31 = lane & 31;
  const int H = a.H, W = a.W;
  const int Cp = FLIP ? a.Cin : a.Cout, Cq = FLIP ? a.Cout : a.Cin;        // the output's channels, the summation's channels
  const int wtiles = (W + kC3Cols - 1) / kC3Cols;
  const int j0 = (blockIdx.x % wtiles) * kC3Cols, i0 = (blockIdx.x / wtiles) * kC3Rows, p0 = blockIdx.y * kC3Chan, b = blockIdx.z;
  const size_t HW = (size_t)H * W;
  const float* in = (FLIP ? a.dy : a.x) + (size_t)b * Cq * HW;
  float* out = (FLIP ? a.dx : a.y) + (size_t)b * Cp * HW;
  const bool ob1 = p0 + 32 < Cp;               // block-uniform: the second block of 32 output channels holds a channel
  const int nch = (Cq + kC3Chunk - 1) / kC3Chunk;
  float xr[kXRegs], wr[kWRegs];                // the next chunk, on its way
  // the halo tile [8 q][10 rows][34 columns]: thread (q = tid >> 5, column tid & 31) walks the ten rows of the first 32 columns; the
  // 160 values of the last two columns go one each to the threads below 160
  const int xq = tid >> 5, xc = tid & 31, gjx = j0 - 1 + xc;
  const bool xcv = gjx >= 0 && gjx < W;
  const int eq = tid / (2 * HR), ehr = (tid % (2 * HR)) >> 1, ec = kC3Cols + (tid & 1), egi = i0 - 1 + ehr, egj = j0 - 1 + ec;
  const bool ev = tid < 2 * HR * kC3Chunk && egi >= 0 && egi < H && egj < W;
  // the weights [64 p][8 q][9 taps]: thread (p = tid >> 2, sub = tid & 3) takes the 18 values of the channels 2 sub and 2 sub + 1
  const int wp = tid >> 2, wsub = tid & 3, gp = p0 + wp;
  auto load = [&](int ch) {
    const int gq = ch * kC3Chunk + xq;
    const long long xoff = (long long)gq * (long long)HW + (long long)(i0 - 1) * W + gjx;
#pragma unroll
    for (int hr = 0; hr < HR; ++hr) {
      const int gi = i0 - 1 + hr;
      xr[hr] = (xcv && gq < Cq && gi >= 0 && gi < H) ? in[xoff + (long long)hr * W] : 0.f;
    }
    xr[HR] = (ev && ch * kC3Chunk + eq < Cq) ? in[(size_t)(ch * kC3Chunk + eq) * HW + (size_t)egi * W + egj] : 0.f;
#pragma unroll
    for (int k = 0; k < kWRegs; ++k) {
      const int gq2 = ch * kC3Chunk + 2 * wsub + k / 9;
      const size_t row = FLIP ? (size_t)gq2 * Cp + gp : (size_t)gp * Cq + gq2;
      wr[k] = (gq2 < Cq && gp < Cp) ? a.w[row * 9 + k % 9] : 0.f;
    }
  };
  auto store = [&](float* Xb, float* Wb) {
#pragma unroll
    for (int hr = 0; hr < HR; ++hr) Xb[(xq * HR + hr) * XS + xc] = xr[hr];
    if (tid < 2 * HR * kC3Chunk) Xb[(eq * HR + ehr) * XS + ec] = xr[HR];
#pragma unroll
    for (int k = 0; k < kWRegs; ++k) {
      const int t = FLIP ? 8 - k % 9 : k % 9;        // dx reads the weight as w[o][c][2-u][2-v]
      Wb[((t * (kC3Chunk / 2) + wsub) * 2 + (wp >> 5)) * 64 + (k / 9) * 32 + (wp & 31)] = wr[k];
    }
  };
  load(0);
  f32x16 acc[2][2], T[2][2];
#pragma unroll
  for (int ob = 0; ob < 2; ++ob)
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) acc[ob][rr] = T[ob][rr] = zero16();
  for (int ch = 0; ch < nch; ++ch) {
    float* Xb = Xs[ch & 1];
    float* Wb = Ws[ch & 1];
    store(Xb, Wb);                             // (this buffer was last read two chunks ago: every wave has passed a barrier since)
    __syncthreads();
    if (ch + 1 < nch) load(ch + 1);
#pragma unroll
    for (int s = 0; s < kC3Chunk / 2; ++s) {
      // the wave's rows 2 wave and 2 wave + 1 of the tile read the halo rows 2 wave .. 2 wave + 3
      const float* xb = Xb + ((2 * s + hi) * HR + 2 * wave) * XS + l31;
      float bv[4][3];
#pragma unroll
      for (int hr = 0; hr < 4; ++hr)
#pragma unroll
        for (int v = 0; v < 3; ++v) bv[hr][v] = xb[hr * XS + v];
#pragma unroll
      for (int u = 0; u < 3; ++u)
#pragma unroll
        for (int v = 0; v < 3; ++v) {
          const float* wp = Wb + (((u * 3 + v) * (kC3Chunk / 2) + s) * 2) * 64 + lane;
          const float a0 = wp[0];
          T[0][0] = mma(a0, bv[u][v], T[0][0]);
          T[0][1] = mma(a0, bv[u + 1][v], T[0][1]);
          if (ob1) {
            const float a1 = wp[64];
            T[1][0] = mma(a1, bv[u][v], T[1][0]);
            T[1][1] = mma(a1, bv[u + 1][v], T[1][1]);
          }
        }
    }
    if ((ch & 1) == 1 || ch == nch - 1) {      // the chain closes: two chunks, or the last one alone
#pragma unroll
      for (int ob = 0; ob < 2; ++ob)
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
          acc[ob][rr] += T[ob][rr];
          T[ob][rr] = zero16();
        }
    }
  }
  const int j = j0 + l31;
  if (j >= W) return;
#pragma unroll
  for (int ob = 0; ob < 2; ++ob)
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
      const int i = i0 + 2 * wave + rr;
      if (i >= H) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int p = p0 + 32 * ob + crow(r, hi);
        if (p >= Cp) continue;
        float v = acc[ob][rr][r];
        if (!FLIP) v += a.bias ? a.bias[p] : 0.f;
        out[(size_t)p * HW + (size_t)i * W + j] = v;
      }
    }
}

// ------------------------------------------------------------------------------------------------ dw, db: per (image, slab) partials
constexpr int TS = 33;                       // row stride of an LDS tile image [row][32]: reads with the row on the lane spread over the banks
constexpr int kTileRegs = kC3Tile * 32 / kThreads;   // floats per thread of one [64][32] tile

__device__ __forceinline__ void store_tile(float* dst, const float (&r)[kTileRegs], int tid) {
#pragma unroll
  for (int i = 0; i < kTileRegs; ++i) {
    const int e = tid + i * kThreads;
    dst[(e >> 5) * TS + (e & 31)] = r[i];
  }
}

__global__ __launch_bounds__(kThreads) void conv3_dw_kernel(Conv3Args a, int ct0, int nct) {
  __shared__ float Dt[2][kC3Tile * TS], Xt[2][kC3Tile * TS];   // [64 o][32 pixels] of dy, [64 columns][32 pixels] of shifted x and the ones; two buffers
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5, l31 = lane & 31, wo = wave >> 1, wc = wave & 1;
  const int b = blockIdx.z, slab = blockIdx.y, H = a.H, W = a.W, K9 = 9 * a.Cin, P = K9 + 1;
  const int o0 = (blockIdx.x / nct) * kC3Tile, c0 = (ct0 + blockIdx.x % nct) * kC3Tile;
  const int r0 = slab * kC3Slab, cnt = min(kC3Slab, H - r0) * W, nt = (cnt + 31) / 32;     // the slab's pixels, row-major: at least one
  const size_t HW = (size_t)H * W;
  float* part = a.part + ((size_t)b * gridDim.y + slab) * a.Cout * P;
  const bool active = c0 + 32 * wc < P;      // wave-uniform: the sub-tile holds a column of dw or the ones column
  const float* dy = a.dy + (size_t)b * a.Cout * HW + (size_t)r0 * W;
  const float* x = a.x + (size_t)b * a.Cin * HW;
  const int n = tid & 31, chb = tid >> 5;    // the thread's pixel of a chunk and its first channel of the tile images (then every 8th)
  float dr[kTileRegs], xr[kTileRegs];        // the next tile, on its way
  auto load = [&](int t) {
    const int pix = t * 32 + n, row = pix / W, gi = r0 + row, gj = pix - row * W;
    const bool nv = pix < cnt;
#pragma unroll
    for (int i = 0; i < kTileRegs; ++i) {
      const int ch = chb + 8 * i, o = o0 + ch, ck = c0 + ch, c = ck / 9, tap = ck - 9 * c;
      dr[i] = (nv && o < a.Cout) ? dy[(size_t)o * HW + pix] : 0.f;
      const int si = gi + tap / 3 - 1, sj = gj + tap % 3 - 1;
      float v = 0.f;
      if (nv && ck < K9 && a.dw) {            // (with dw unwanted the tile of the ones column gathers nothing)
        if (si >= 0 && si < H && sj >= 0 && sj < W) v = x[(size_t)c * HW + (size_t)si * W + sj];
      } else if (nv && ck == K9 && a.db) {
        v = 1.f;
      }
      xr[i] = v;
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
      if ((t & 3) == 3 || t == nt - 1) {     // the chain closes: four chunks (128 pixels), or what is left
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
    if (o < a.Cout && (a.dw || c == K9)) part[(size_t)o * P + c] = acc[r];
  }
}

__global__ __launch_bounds__(kThreads) void conv3_dw_reduce_kernel(Conv3Args a, int c_first, int slabs) {
  const int K9 = 9 * a.Cin, P = K9 + 1, c = c_first + blockIdx.x * kThreads + threadIdx.x, o = blockIdx.y;
  if (c >= P || (c < K9 ? a.dw == nullptr : a.db == nullptr)) return;
  float total = 0.f;
  for (int b = 0; b < a.B; ++b) {
    const float* p = a.part + ((size_t)b * slabs * a.Cout + o) * P + c;
    float image = 0.f;
    for (int s = 0; s < slabs; ++s) image += p[(size_t)s * a.Cout * P];
    total += image;
  }
  if (c < K9) a.dw[(size_t)o * K9 + c] = total;
  else a.db[o] = total;
}

// with dw unwanted only the column tile that holds the ones column (index 9 Cin) runs
inline void dw_tiles(const Conv3Args& a, int& ct0, int& nct) {
  const int K9 = 9 * a.Cin;
  ct0 = a.dw ? 0 : K9 / kC3Tile;
  nct = (a.dw ? cdiv(K9 + (a.db ? 1 : 0), kC3Tile) : K9 / kC3Tile + 1) - ct0;
}

}  // namespace

long long conv3_max_grid(int B, int Cout, int Cin, int H, int W) {
  const long long tiles = (long long)cdiv(W, kC3Cols) * cdiv(H, kC3Rows) * B;
  const long long fwd = tiles * cdiv(Cout, kC3Chan), dx = tiles * cdiv(Cin, kC3Chan);
  const long long dw = (long long)cdiv(9 * Cin + 1, kC3Tile) * cdiv(Cout, kC3Tile) * conv3_slabs(H) * B;
  return std::max(fwd, std::max(dx, dw));
}

hipError_t launch_conv3_fwd(const Conv3Args& a, hipStream_t s) {
  hipLaunchKernelGGL(conv3_kernel<false>, dim3(cdiv(a.W, kC3Cols) * cdiv(a.H, kC3Rows), cdiv(a.Cout, kC3Chan), a.B), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_conv3_dx(const Conv3Args& a, hipStream_t s) {
  hipLaunchKernelGGL(conv3_kernel<true>, dim3(cdiv(a.W, kC3Cols) * cdiv(a.H, kC3Rows), cdiv(a.Cin, kC3Chan), a.B), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_conv3_dw(const Conv3Args& a, hipStream_t s) {
  int ct0, nct;
  dw_tiles(a, ct0, nct);
  hipLaunchKernelGGL(conv3_dw_kernel, dim3(nct * cdiv(a.Cout, kC3Tile), conv3_slabs(a.H), a.B), dim3(kThreads), 0, s, a, ct0, nct);
  return hipGetLastError();
}

hipError_t launch_conv3_dw_reduce(const Conv3Args& a, hipStream_t s) {
  const int K9 = 9 * a.Cin, c_first = a.dw ? 0 : K9, c_end = a.db ? K9 + 1 : K9;
  hipLaunchKernelGGL(conv3_dw_reduce_kernel, dim3(cdiv(c_end - c_first, kThreads), a.Cout), dim3(kThreads), 0, s, a, c_first, conv3_slabs(a.H));
  return hipGetLastError();
}

}  // namespace imx
