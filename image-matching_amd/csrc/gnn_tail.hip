// gnn_tail.hip -- the tail of one GNN layer of the THROUGHPUT path in one launch (round 4; superglue_test.py:110-119,134-137 and
// the next layer's projections :99-100, or final_proj :256):
//     hidden = relu([x | att] W1' + b1)      (mlp.0 with BatchNorm and attn.merge folded, 2d -> 2d)
//     x     += hidden W2 + b2                 (mlp.3, 2d -> d, residual)
//     out    = x W3 + b3                      (the NEXT layer's q|k|v, d -> 3d, or final_proj, d -> d)
// ONE kernel body, templated on the operand format (planes.h): FmtX3 carries every fp32 product as six bf16 plane products of
// three-plane operands (gnn_tail_x3_kernel, the arithmetic of gemm_x3.hip), FmtH2 as THREE fp16 plane products of two-plane operands
// (gnn_tail_h2_kernel; the format of attention_x3.hip's FmtH2 and of conv3x3_wino24h.hip): 864 instead of 1728 MFMAs per wave and 32
// rows, 16-KB instead of 24-KB weight images.
//
// Why one kernel: the three gemm_x3 launches it replaces run at 0.32-0.39 of the bf16 pipe -- K is 128 / 256, so a 128 x 128 tile is
// 4-8 chunks long and its prologue (first loads), its LDS staging of the split activations (a barrier per chunk) and its epilogue
// (64 KB of stores per tile) weigh as much as its MFMAs; between the launches 268 MB of hidden activations and 67 MB of x' go to HBM
// and come back.  Here a WAVE owns 32 rows from the first product to the last store:
//   * every product is TRANSPOSED, D[channel][row] = W^T . act^T: the weights are the MFMA's A operand, the wave's activations its B
//     operand.  A lane of the result holds sixteen channels of ITS row -- which is a B operand of the next product when that
//     product's k index is mapped onto those channels (gnn_tail_pack.h permutes the weights accordingly).  The hidden activations
//     and x' stay in the registers of the wave: no LDS staging, no barrier, no HBM round trip for them;
//   * the first product's B operand is loaded straight from global memory (a lane reads 64 contiguous bytes of its row per 32-k
//     chunk) and split in registers (planes.h);
//   * the only thing in LDS is the weight stream: images of 2 k-steps x 4 output blocks x NP planes (24 / 16 KB; gnn_tail_pack.h writes
//     them in consumption order) in a ring of two / three, copied by LDS-DMA one / two images ahead (global_load_lds: no staging
//     registers, no ds_write pass), ONE barrier per image (48 / 24 MFMAs per wave) behind a COUNTED vmcnt; the four waves of a
//     workgroup share every image;
//   * mlp.0's 256 hidden channels are produced in two halves (64 accumulator registers each), each half consumed by mlp.3 right away
//     (the first product's activations are read and split twice: +7 % VALU work, -64 registers);
//   * results and the residual go through a per-wave 32 x 32 transpose tile in LDS, so that every global access is a full 128-byte
//     row segment.
// Work per wave and 32 rows (FmtX3): 768 + 384 + 576 MFMAs (q|k|v) against ~1700 VALU instructions.
//
// FmtH2's scales.  fp16 has five exponent bits, so every operand is multiplied by a power of two.  The weights' are fixed on the host
// (gnn_tail_pack_h2: each matrix's largest |value| to [2^13, 2^14)).  The activations' come from BOUNDS that are uniform over a wave (its
// 32 rows belong to one (side, pair)):
//     |[x | att]| <= bound_in = max(amax_x, amax_v)      amax_x: the (side, pair)'s largest |x| over its valid rows, written by the kernel that
//                                                        produced x (this kernel's epilogue for the previous layer; rows_amax (gemm_h2.hip) for layer 0);
//                                                        amax_v: the key side's largest |v| (att is a convex combination of v rows)
//     |hidden|    <= bound_h  = bound_in L1(W1') + max|b1|           (largest column L1 norm of the folded mlp.0)
//     |x'|        <= bound_x  = amax_x + bound_h L1(W2) + max|b2|
// A bound that is loose by 2^k costs nothing while the typical value stays above 2^-3 after scaling (its low plane is then a normal
// fp16 number): these are loose by ~2^6 and ~2^11 of 2^17.  Rows past the valid count are not covered by the maxima: their inputs are
// zeroed before the split (they are never read by the attention's softmax or by the score matrix).
// The powers of two are undone where a result leaves its accumulator: one multiply per value that was a conversion's input anyway.
#include "imx_kernels.h"
#include "planes.h"
#include "gnn_tail_pack.h"

namespace imx {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int GT_STAGE_RS = 36;
#ifndef GT_RING
#define GT_RING 3      // FmtH2's weight images resident per workgroup: the stream runs two images ahead (round 6: with two, one ahead, 2.69 -> 2.63 ms
                       // per C3 step on one box; 70 KB of LDS per workgroup, two workgroups per CU)
#endif

// What the format decides about the weight stream (in 16-byte elements).  Four waves per workgroup, two k-steps per image.
template <class Fmt>
struct Stream {
  static constexpr int RING = Fmt::SCALED ? GT_RING : 2;       // images resident per workgroup (FmtX3: 2 x 24 KB)
  static constexpr int STEP = 4 * Fmt::NP * 64;                // one k-step: 4 output blocks x NP planes x 1 KB
  static constexpr int SLOT = 2 * STEP;                        // one image
  static constexpr int PIECES = SLOT / 256;                    // LDS-DMA pieces per thread and image: 6 / 4
  static __device__ __forceinline__ const u32x4* base(const GnnTailArgs& p) {
    return reinterpret_cast<const u32x4*>(Fmt::SCALED ? p.stream_h2 : p.stream);
  }
};

// eight fp32 values (FmtH2: already scaled) -> the planes of one B operand
template <class Fmt>
__device__ __forceinline__ void split8(const float (&v)[8], typename Fmt::x8 (&pl)[Fmt::NP]) {
#pragma unroll
  for (int j = 0; j < 8; j += 2) {
    typename Fmt::x2 t[Fmt::NP];
    Fmt::split(v[j], v[j + 1], t);
#pragma unroll
    for (int q = 0; q < Fmt::NP; ++q) { pl[q][j] = t[q][0]; pl[q][j + 1] = t[q][1]; }
  }
}

// The workgroup barrier between weight images.  __syncthreads() is a fence: hipcc puts s_waitcnt vmcnt(0) lgkmcnt(0) in front of the
// s_barrier, which would drain the wave's activation prefetch (an HBM latency) at EVERY image.  Only this wave's LDS stores of the
// next image have to be complete before the others may read them: lgkmcnt(0).
// The weight images arrive by LDS-DMA (global_load_lds: no staging registers, no ds_write pass); such data is ordered for the readers
// only by the ISSUING wave's counted vmcnt followed by a barrier.  VMEM operations retire in order, so vmcnt(N) with N = the operations
// this wave issued AFTER the DMA pieces of the image that is due and that may still be in flight retires that image without draining
// them.  With a ring of R images the stream runs AHEAD = R - 1 images ahead, so these are
//     YOUNGER = PIECES x (AHEAD - 1)   DMA pieces of the images requested after the one that is due (none at R = 2, four at R = 3), and
//     pend                             the wave's own operations since its newest request that it has not consumed (the activation
//                                      prefetch: two chunks = 8 loads; the stores and atomics of a result: 16 or 17);
// lgkmcnt(0) retires this wave's LDS reads of the slot that is about to be refilled.
// n is a compile-time constant after unrolling and is rounded DOWN to 0, 4, 8 or 16 (waiting for more is always safe); exactly one
// s_barrier is executed whatever n is
__device__ __forceinline__ void image_barrier(int n) {
  if (n >= 16) asm volatile("s_waitcnt vmcnt(16) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  else if (n >= 8) asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  else if (n >= 4) asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// Four waves per workgroup: TWO workgroups of 128 rows per CU, weight images of two k-steps.  Eight waves (one workgroup of 256 rows per
// CU, images of four k-steps, half the weight stream per row; two waves share a SIMD either way) were measured and dropped
// (docs/HISTORY.md).  FmtX3: the same at 131072 rows (255 vs 256 us: a SIMD's time is the sum of its waves' MFMA and VALU issue whichever
// way they are grouped), four waves ahead where workgroups are scarce (8224 rows: 40 vs 60 us; three gemm_x3 launches: 50).
// FmtH2 (round 6): 2.86 with eight against 2.70 ms per C3 step with four, same box.
template <class Fmt, int NPASS>
__device__ __forceinline__ void gnn_tail_body(const GnnTailArgs& p) {
  typedef typename Fmt::x8 x8;
  typedef Stream<Fmt> St;
  constexpr int D = 128, NP = Fmt::NP;
  constexpr int NW = 4, NT = 64 * NW;
  constexpr int SPI = 2;                                   // k-steps per weight image
  constexpr int RING = St::RING, SLOT = St::SLOT;
  constexpr int NSTEP = 2 * (16 + 8) + 8 * NPASS;          // k-steps of the whole tail
  constexpr int NIMG = NSTEP / SPI;
  extern __shared__ __attribute__((aligned(16))) u32x4 ring[];       // [RING][SLOT] weight images, the biases (2 D + D + NPASS D floats), the transpose tiles
  float* lbias = reinterpret_cast<float*>(ring + RING * SLOT);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5, l31 = lane & 31;
  const int row0 = blockIdx.x * (32 * NW) + 32 * wave;
  float* stage = lbias + (3 + NPASS) * D + wave * (32 * GT_STAGE_RS);      // this wave's 32 x 32 transpose tile (row stride 36 floats: conflict-free 16-byte accesses)
  const bool active = row0 < p.M;                                    // waves past M (a multiple of 32) compute on a clamped row and store nothing
  const int row = min(row0 + l31, p.M - 1);
  const u32x4* stream = St::base(p);
  // this wave's (side, pair) -- its 32 rows belong to one: the padded counts are multiples of 32, the division is wave-uniform -- and
  // the valid part of its rows.  FmtH2 scales by it; either format needs it for the next layer's maxima (amax)
  int sp = 0, ksp = 0, i0 = 0, nvalid = 0;
  if ((Fmt::SCALED || (NPASS == 3 && p.amax)) && active) {
    const int r0 = __builtin_amdgcn_readfirstlane(row0), s1 = p.B * p.N0p;
    const int side = r0 >= s1 ? 1 : 0, Np = side ? p.N1p : p.N0p, rr = r0 - (side ? s1 : 0);
    const int b = rr / Np;
    i0 = rr - b * Np;
    nvalid = side ? (p.n1 ? p.n1[b] : p.N1) : (p.n0 ? p.n0[b] : p.N0);
    sp = side * p.B + b;
    ksp = (p.cross ? 1 - side : side) * p.B + b;
  }
  const bool row_valid = i0 + l31 < nvalid;
  unsigned* amax_slot = (NPASS == 3 && p.amax && active) ? p.amax + (size_t)sp * 4 : nullptr;      // the next layer's q | k | v maxima of this (side, pair)
  // FmtH2: the powers of two of its operands (header), what the three accumulators carry (k1, k2, k3) and what undoes it; FmtX3: all 1
  float s_x = 1.f, k1 = 1.f, k2 = 1.f, k3 = 1.f, c1 = 1.f, c2inv = 1.f, c3inv = 1.f, sin_lane = 1.f;
  if constexpr (Fmt::SCALED) {
    const float ax = __builtin_bit_cast(float, p.amax_x_in[sp]), av = __builtin_bit_cast(float, p.amax_v[(size_t)ksp * 4 + 2]);
    const float bound_in = fmaxf(fmaxf(ax, av), 1e-30f);
    const float bound_h = fmaf(bound_in, p.l1_1, p.bmax_1);
    const float bound_x = ax + fmaf(bound_h, p.l1_2, p.bmax_2);
    const float s_in = pow2_scale(bound_in), s_h = pow2_scale(bound_h);
    s_x = pow2_scale(bound_x);
    k1 = s_in / p.w1_inv; k2 = s_h / p.w2_inv; k3 = s_x / p.w3_inv;
    c1 = s_h / k1; c2inv = 1.0f / k2; c3inv = 1.0f / k3;
    sin_lane = row_valid ? s_in : 0.f;                                            // rows past the count: inputs zeroed (the maxima do not cover them)
  }

  // ---- the weight stream: image i -> ring slot i % RING by LDS-DMA, RING - 1 images ahead (PIECES per thread: 16-byte elements j * NT + tid)
  typedef __attribute__((address_space(3))) void lds_void;
  typedef const __attribute__((address_space(1))) void glb_void;
  int pend = 0;      // VMEM operations issued after the newest image's DMA pieces that may still be in flight at the next barrier
  auto fetch = [&](int i) __attribute__((always_inline)) {
    __builtin_amdgcn_sched_barrier(0);            // the order of VMEM operations around the DMA pieces is what image_barrier counts on
#pragma unroll
    for (int j = 0; j < St::PIECES; ++j)
      __builtin_amdgcn_global_load_lds((glb_void*)(stream + (size_t)i * SLOT + j * NT + tid),
                                       (lds_void*)(ring + (i % RING) * SLOT + j * NT + 64 * wave), 16, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    pend = 0;
  };
  // global k-step gs: at the first step of an image the workgroup meets (image gs / SPI is in its slot: its DMA was issued RING - 1
  // images ago; the slot of the image just finished is free) and the image RING - 1 ahead is requested
  auto enter_step = [&](int gs) __attribute__((always_inline)) {
    if (gs % SPI) return;
    const int img = gs / SPI;
    constexpr int AHEAD = RING - 1, YOUNGER = St::PIECES * (AHEAD - 1);
    if (img > 0) image_barrier((active ? pend : 0) + (img + 1 < NIMG ? YOUNGER : 0));
    if (img + AHEAD < NIMG) fetch(img + AHEAD);
  };
  // one k-step: 4 NT MFMAs (24 / 12).  The A operands (four output blocks x NP planes from the image) are read two blocks at a time --
  // half the registers -- and the two blocks' MFMAs alternate, so consecutive MFMAs never share an accumulator.
  auto step24 = [&](int gs, const x8 (&b)[NP], f32x16 (&acc)[4]) __attribute__((always_inline)) {
    const int i = gs / SPI, t = gs % SPI;
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
      x8 a[2][NP];
#pragma unroll
      for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int q = 0; q < NP; ++q) a[e][q] = __builtin_bit_cast(x8, ring[(i % RING) * SLOT + ((t * 4 + 2 * pr + e) * NP + q) * 64 + lane]);
#pragma unroll
      for (int q = 0; q < Fmt::NT; ++q)
#pragma unroll
        for (int e = 0; e < 2; ++e)
          acc[2 * pr + e] = Fmt::mfma(a[e][Fmt::pa(q)], b[Fmt::pb(q)], acc[2 * pr + e]);
    }
  };
  // accumulators of four 32-channel blocks start from the bias of their channels: register 4 g + e <-> channel 32 blk + 8 g + 4 hi + e.
  // The biases sit in LDS: a global load here would queue behind the stores of the previous pass (VMEM returns in order).
  // (`k`: the power of two the product's accumulators carry)
  auto bias_init = [&](f32x16 (&acc)[4], int off, float k) __attribute__((always_inline)) {
#pragma unroll
    for (int blk = 0; blk < 4; ++blk)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(lbias + off + 32 * blk + 8 * g + 4 * hi) * k;
        acc[blk][4 * g] = v[0]; acc[blk][4 * g + 1] = v[1]; acc[blk][4 * g + 2] = v[2]; acc[blk][4 * g + 3] = v[3];
      }
  };
  // the first product's activations: chunk c (32 k) of [x | att], sixteen contiguous floats of the lane's row
  const float* xrow = p.x + (size_t)row * D;
  const float* arow = p.att + (size_t)row * D;
  auto act_load = [&](int c, f32x4 (&a)[4]) __attribute__((always_inline)) {
    const float* src = (c < 4 ? xrow : arow) + 32 * (c & 3) + 16 * hi;
#pragma unroll
    for (int q = 0; q < 4; ++q) a[q] = *reinterpret_cast<const f32x4*>(src + 4 * q);
    pend += 4;
  };

  // A 32-channel block of a transposed result -> 32 rows x 128 bytes of a row-major tensor, through this wave's LDS tile: a lane's
  // direct stores would put 32 bytes into each of 32 different rows per instruction (partial lines: measured 10-18 k cycles per
  // 128-channel burst); from the tile every store instruction writes eight full 128-byte row segments.
  auto store_block = [&](const f32x16& acc, float* dst, int ld, int col) __attribute__((always_inline)) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 v = (f32x4){acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]} * c3inv;
      *reinterpret_cast<f32x4*>(stage + l31 * GT_STAGE_RS + 8 * g + 4 * hi) = v;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int r = 8 * k + (lane >> 3);
      const f32x4 v = *reinterpret_cast<const f32x4*>(stage + r * GT_STAGE_RS + 4 * (lane & 7));
      *reinterpret_cast<f32x4*>(dst + (size_t)(row0 + r) * ld + col + 4 * (lane & 7)) = v;
    }
  };

  fetch(0);
  if constexpr (RING > 2) { if (NIMG > 1) fetch(1); }
  for (int e = tid; e < (3 + NPASS) * D; e += NT) lbias[e] = e < 2 * D ? p.b1[e] : e < 3 * D ? p.b2[e - 2 * D] : p.b3[e - 3 * D];
  __syncthreads();                     // (a full fence: the biases, and image 0)
  f32x16 acc2[4];                      // x' (mlp.3's output, transposed)
  bias_init(acc2, 2 * D, k2);
  int gs = 0;                          // global k-step (a compile-time constant at every use: all loops are unrolled)
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    // ---- mlp.0', hidden channels 128 half .. +127: 16 k-steps = 8 chunks of 32 k
    f32x16 acc1[4];
    bias_init(acc1, D * half, k1);
    f32x4 act[3][4];                                       // ring of three chunks: loaded TWO chunks (four k-steps) ahead
    act_load(0, act[0]);
    act_load(1, act[1]);
#pragma unroll
    for (int s = 0; s < 16; ++s, ++gs) {
      enter_step(gs);
      const int c = s >> 1;
      if ((s & 1) == 0 && c + 2 < 8) act_load(c + 2, act[(c + 2) % 3]);
      const f32x4 (&cur)[4] = act[c % 3];
      const f32x4 lo = cur[2 * (s & 1)], hi4 = cur[2 * (s & 1) + 1];
      const float v[8] = {lo[0] * sin_lane, lo[1] * sin_lane, lo[2] * sin_lane, lo[3] * sin_lane, hi4[0] * sin_lane, hi4[1] * sin_lane, hi4[2] * sin_lane, hi4[3] * sin_lane};
      x8 bp[NP];
      split8<Fmt>(v, bp);
      step24(gs, bp, acc1);
    }
    // ---- mlp.3 over this half's hidden channels: k-steps (b, h2) with the B operand straight from acc1 (ReLU here)
#pragma unroll
    for (int s = 0; s < 8; ++s, ++gs) {
      enter_step(gs);
      const int b = s / 2, h2 = s & 1;
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = fmaxf(acc1[b][8 * h2 + j], 0.f) * c1;      // (FmtH2: hidden s_h)
      x8 bp[NP];
      split8<Fmt>(v, bp);
      step24(gs, bp, acc2);
    }
  }
  float xmax = 0.f;
  // ---- x' = x + (hidden W2 + b2): through the transpose tile, where a lane sees 16 contiguous bytes of a row -- the residual is read
  //      and x' written as full 128-byte row segments (16 loads + 16 stores; the next image_barrier counts the stores), and the sum
  //      comes back from the tile in the transposed layout for the next product
#pragma unroll
  for (int blk = 0; blk < 4; ++blk) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 v = {acc2[blk][4 * g], acc2[blk][4 * g + 1], acc2[blk][4 * g + 2], acc2[blk][4 * g + 3]};
      *reinterpret_cast<f32x4*>(stage + l31 * GT_STAGE_RS + 8 * g + 4 * hi) = v;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int r = 8 * k + (lane >> 3);
      float* xa = p.x + (size_t)min(row0 + r, p.M - 1) * D + 32 * blk + 4 * (lane & 7);
      const f32x4 v = *reinterpret_cast<const f32x4*>(stage + r * GT_STAGE_RS + 4 * (lane & 7)) * c2inv + *reinterpret_cast<const f32x4*>(xa);
      if (active) *reinterpret_cast<f32x4*>(xa) = v;
      *reinterpret_cast<f32x4*>(stage + r * GT_STAGE_RS + 4 * (lane & 7)) = v;
      if constexpr (Fmt::SCALED) {
        if (i0 + r < nvalid) xmax = fmaxf(xmax, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));      // x' of the valid rows
      }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(stage + l31 * GT_STAGE_RS + 8 * g + 4 * hi);
      acc2[blk][4 * g] = v[0]; acc2[blk][4 * g + 1] = v[1]; acc2[blk][4 * g + 2] = v[2]; acc2[blk][4 * g + 3] = v[3];
    }
  }
  pend = 16;                           // the sixteen stores of x' (their loads are older and were consumed)
  if constexpr (Fmt::SCALED) {
    if (p.amax_x_out && active) {      // the largest |x'| of this (side, pair): the NEXT layer's amax_x (one atomic without return per wave)
      unsigned mb = __builtin_bit_cast(unsigned, xmax);
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) mb = max(mb, (unsigned)__shfl_xor((int)mb, o));
      if (lane == 0 && mb) atomicMax(p.amax_x_out + sp, mb);
      pend += 1;
    }
  }
  x8 xp[8][NP];                        // x' (FmtH2: x' s_x) as the B operands of the next product's k-steps (ob, h2): split once, used by every pass
#pragma unroll
  for (int ob = 0; ob < 4; ++ob)
#pragma unroll
    for (int h2 = 0; h2 < 2; ++h2) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = acc2[ob][8 * h2 + j] * s_x;
      split8<Fmt>(v, xp[2 * ob + h2]);
    }
  // ---- the next product: NPASS passes of 128 output channels, 8 k-steps each
#pragma unroll
  for (int pass = 0; pass < NPASS; ++pass) {
    __builtin_amdgcn_sched_barrier(0);           // (keeps the next pass's accumulators from being initialised before this pass's are stored: registers)
    f32x16 acc3[4];
    bias_init(acc3, 3 * D + D * pass, k3);
#pragma unroll
    for (int s = 0; s < 8; ++s, ++gs) {
      enter_step(gs);
      step24(gs, xp[s], acc3);
    }
    if (active) {
#pragma unroll
      for (int blk = 0; blk < 4; ++blk) store_block(acc3[blk], p.out, p.n3, D * pass + 32 * blk);
    }
    pend = 16;
    if constexpr (NPASS == 3) {
      // max |q| / |k| / |v| (pass 0 / 1 / 2) over the valid rows of this wave's (side, pair), for the next layer's attention
      // (GnnTailArgs::amax): a lane holds 64 values of ITS row -- 32 v_max3 with |.| modifiers, one select, a wave reduction, one
      // atomic without return per wave and pass (32 waves share a word: the atomics sit in the wave's in-order VMEM queue like a store;
      // three words per LAUNCH instead of per (side, pair): +27 us)
      if (amax_slot) {
        float mx = 0.f;
#pragma unroll
        for (int blk = 0; blk < 4; ++blk)
#pragma unroll
          for (int r = 0; r < 16; r += 2) mx = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(acc3[blk][r]), __builtin_fabsf(acc3[blk][r + 1])), mx);
        unsigned mb = row_valid ? __builtin_bit_cast(unsigned, mx * c3inv) : 0u;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) mb = max(mb, (unsigned)__shfl_xor((int)mb, o));
        if (lane == 0 && mb) atomicMax(amax_slot + pass, mb);
        pend += 1;
      }
    }
  }
}

// (two names, so that a profile tells the formats apart: gnn_tail_x3_kernel<3>, gnn_tail_h2_kernel<3>, and <1> for final_proj)
template <int NPASS>
__global__ __launch_bounds__(256, 2) void gnn_tail_x3_kernel(GnnTailArgs p) { gnn_tail_body<FmtX3, NPASS>(p); }
template <int NPASS>
__global__ __launch_bounds__(256, 2) void gnn_tail_h2_kernel(GnnTailArgs p) { gnn_tail_body<FmtH2, NPASS>(p); }

// dynamic LDS of a workgroup: the ring, the biases, four transpose tiles
template <class Fmt>
size_t tail_lds_bytes(const GnnTailArgs& a) {
  return (size_t)Stream<Fmt>::RING * Stream<Fmt>::SLOT * 16 + (size_t)(3 * a.d + a.n3 + 4 * 32 * GT_STAGE_RS) * sizeof(float);
}

}  // namespace

bool gnn_tail_x3_supported(const GnnTailArgs& a) {
  if (a.amax && (a.n3 != 384 || a.B <= 0 || a.N0p % 32 || a.N1p % 32 || a.M != a.B * (a.N0p + a.N1p))) return false;
  return a.d == 128 && (a.n3 == 384 || a.n3 == 128) && a.M > 0 && a.M % 32 == 0 && a.stream && a.b1 && a.b2 && a.b3;
}

hipError_t launch_gnn_tail_x3(const GnnTailArgs& a, hipStream_t s) {
  if (!gnn_tail_x3_supported(a)) return hipErrorInvalidValue;
  last_form = "gnn_tail_x3:bf16x3";
  static unsigned long long attr[2] = {0, 0};
  auto go = [&](auto kern, int which) {
    const size_t lds = tail_lds_bytes<FmtX3>(a);
    raise_lds_limit(reinterpret_cast<const void*>(kern), (int)lds, attr[which]);
    hipLaunchKernelGGL(kern, dim3((unsigned)((a.M + 127) / 128)), dim3(256), lds, s, a);
  };
  if (a.n3 == 384) go(gnn_tail_x3_kernel<3>, 0); else go(gnn_tail_x3_kernel<1>, 1);
  return hipGetLastError();
}

bool gnn_tail_h2_supported(const GnnTailArgs& a) {
  if (!a.stream_h2 || !a.amax_x_in || !a.amax_v || !(a.w1_inv > 0.f) || !(a.w2_inv > 0.f) || !(a.w3_inv > 0.f)) return false;
  if (a.B <= 0 || a.N0p % 32 || a.N1p % 32 || a.M != a.B * (a.N0p + a.N1p)) return false;
  if (a.amax && a.n3 != 384) return false;
  return a.d == 128 && (a.n3 == 384 || a.n3 == 128) && a.M > 0 && a.b1 && a.b2 && a.b3;
}

hipError_t launch_gnn_tail_h2(const GnnTailArgs& a, hipStream_t s) {
  if (!gnn_tail_h2_supported(a)) return hipErrorInvalidValue;
  last_form = "gnn_tail_h2:f16x2";
  static unsigned long long attr[2] = {0, 0};
  auto go = [&](auto kern, int which) {
    const size_t lds = tail_lds_bytes<FmtH2>(a);
    raise_lds_limit(reinterpret_cast<const void*>(kern), (int)lds, attr[which]);
    hipLaunchKernelGGL(kern, dim3((unsigned)((a.M + 127) / 128)), dim3(256), lds, s, a);
  };
  if (a.n3 == 384) go(gnn_tail_h2_kernel<3>, 0); else go(gnn_tail_h2_kernel<1>, 1);
  return hipGetLastError();
}

}  // namespace imx
