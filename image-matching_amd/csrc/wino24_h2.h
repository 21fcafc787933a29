// wino24_h2.h -- what the four fp16 Winograd F(2x4, 3x3) kernels share besides the transforms of wino24_pk.h: the tile and operand
// geometry and the scales of conv3x3_wino24h.hip (tile form) / conv3x3_wino24p.hip (pair form) and of conv1ab_wino24h.hip /
// conv1ab_wino24p.hip, the fused first layer in the same two forms.  The two-plane split is planes.h's FmtH2::split.  The loaders, the
// transform / MFMA phases and the epilogues stay in the kernels: they capture kernel state, and their register allocation was tuned
// per kernel.
#pragma once
#include "planes.h"
#include "wino24_pk.h"

namespace imx {
namespace {

// ---- all four kernels
constexpr int OH = 8, OW = 16;                 // output pixels per tile (4 x 4 wtiles of 2 x 4)
constexpr int RH = OH + 2, RW = OW + 2;        // input patch of the 3x3 convolution (pad-1 halo)
constexpr int NPOS = 24;                       // Winograd positions
constexpr int VPLANE = NPOS * 4 * 16 * 8;      // halves per plane of a tile's V (24576 bytes)
constexpr int UPOS = 2 * 4 * 64 * 8;           // halves of U per ((item block,) chunk, position): [plane][wave / channel block][lane][8]
constexpr int RING = 6;                        // positions of U in flight (pair form: of the wave's twelve, NLP % RING == 0)
// (all but conv1ab_wino24h.hip) image b -> slot b % 256: ConvArgs::amax_in / amax_out hold upper bounds, so sharing a slot is safe
constexpr int AMAX_SLOTS = 256;

template <bool V>
struct BoolC { static constexpr bool value = V; };

// ---- the pair form (conv3x3_wino24p.hip, conv1ab_wino24p.hip)
constexpr int NG = 2;                          // tiles per workgroup
constexpr int NLP = 12;                        // positions per wave: transformed COLUMNS 3 ph .. 3 ph + 2, all four rows = positions 12 ph + lp, lp = jj*4 + i
constexpr int VGRP = 2 * VPLANE;               // halves per tile
constexpr int XCH = 6 * 64 * 16;               // bytes of one wave's exchange block: the row stage's six results for the partner's tile

// the lane index, recomputed where it is called (a volatile asm is not hoisted out of the main loop: values derived from a kept
// lane index are spilled to scratch there, and a scratch reload is a vector-memory operation that waits for the loads in flight)
__device__ __forceinline__ int lane_now() {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}

// ---- the 3x3 layers (conv3x3_wino24h.hip, conv3x3_wino24p.hip)
constexpr int RSC = 10;                        // raw sub-patch: pixel stride (8 channels + 2), as in conv3x3_wino24.hip
constexpr int RAWC = 192 * RSC;                // 180 pixels + pad, floats per 8-channel sub-patch
constexpr int NSUB = 4;                        // 8-channel sub-patches per chunk
constexpr int CKH = 32, NT = 64;               // input channels per chunk, output channels per item
constexpr unsigned OOB = 0x7ffffff0u;          // byte offset beyond any image: buffer loads return 0

// s_v of an image: 32 x its largest |input| (>= the bound 20 max|d| of the transformed patch) goes to 2^13
__device__ __forceinline__ float v_scale(unsigned amax_bits) {
  unsigned e = (amax_bits >> 23) & 0xffu;
  e = e < 60u ? 60u : e > 200u ? 200u : e;
  return __builtin_bit_cast(float, (262u - e) << 23);
}

// ---- the fused first layer (conv1ab_wino24h.hip, conv1ab_wino24p.hip)
constexpr int IMG_H = RH + 2, IMG_W = RW + 2;  // image patch 12 x 20
constexpr int RSH = 34;                        // conv1a half patch: pixel stride (32 channels + 2: wtile columns 4 px apart land 8 banks apart)
constexpr int RAWSZ = 192 * RSH;               // floats per tile: 180 pixels + 12 pad (the conv1a GEMM's twelfth pixel block stores unmasked)

// the power of two that brings 32 x `bound` (>= 20 max|d| >= |V|) to 2^13
__device__ __forceinline__ float v_scale_of_bound(float bound) {
  unsigned e = (__builtin_bit_cast(unsigned, bound) >> 23) & 0xffu;
  e = e < 60u ? 60u : e > 200u ? 200u : e;
  return __builtin_bit_cast(float, (261u - e) << 23);
}

}  // namespace
}  // namespace imx
