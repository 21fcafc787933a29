// planes.h -- the split-plane operand formats: an fp32 product carried on a 16-bit matrix pipe.  A format says how
// a value is cut into 16-bit planes, which plane products are kept and in what order, which MFMA runs them and (FmtH2) how the power of
// two is derived that brings an operand into fp16's range.  Every kernel of that kind (gemm_x3.hip, gemm_h2.hip, gnn_tail.hip,
// attention_x3.hip, the fp16 Winograd convolutions) takes these from here.
//
// The splits.  Round 4: the residuals r = x - float(h) (and r - float(m)) are ONE instruction per value, v_dot2c_f32_bf16 / v_dot2c_f32_f16
// (D += a.lo * b.lo + a.hi * b.hi with the packed pair (h0, h1) as `a` and the constant (-1, 0) / (0, -1) as `b`): the products of a
// 16-bit value with -1 / 0 are exact and the sum x - h is exactly representable (it is the rounding residual of x), so the result is
// the same bits as the unpack (shift / mask) + v_sub_f32 pair it replaces -- 3.5 VALU instructions per value instead of 5.5 for three
// bf16 planes, 2 for two fp16 planes (tools/ubench/split_dot2.hip checks all three bf16 planes bit for bit over 2^24 values incl.
// zeros, subnormal residuals and the largest finite values).
// The constants go through SGPRs behind an (un-foldable, side-effect-free) asm: hipcc 7.2 encodes the packed constant {-1, 0} as the
// INLINE constant -1.0, which these instructions on gfx950 do not read as the 16-bit pair (-1, 0) -- the result is x + 0.0034 instead
// of x - h (tools/ubench/split_dot2.hip's first version; a literal or a register operand is correct).
#pragma once
#include <hip/hip_runtime.h>

namespace imx {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 split_bf16x2 __attribute__((ext_vector_type(2)));

// x = h + m + l, an fp32 value as three bf16 terms (8 significant bits each, round-to-nearest residuals), two values at a time
__device__ __forceinline__ void split3_pair(float x0, float x1, split_bf16x2& h, split_bf16x2& m, split_bf16x2& l) {
  unsigned lo_u, hi_u;
  asm("s_mov_b32 %0, 0x0000bf80" : "=s"(lo_u));
  asm("s_mov_b32 %0, 0xbf800000" : "=s"(hi_u));
  const split_bf16x2 lo = __builtin_bit_cast(split_bf16x2, lo_u), hi = __builtin_bit_cast(split_bf16x2, hi_u);
  h[0] = (__bf16)x0; h[1] = (__bf16)x1;                                    // v_cvt_pk_bf16_f32
  const float r0 = __builtin_amdgcn_fdot2_f32_bf16(h, lo, x0, false);      // x0 - h0
  const float r1 = __builtin_amdgcn_fdot2_f32_bf16(h, hi, x1, false);      // x1 - h1
  m[0] = (__bf16)r0; m[1] = (__bf16)r1;
  l[0] = (__bf16)__builtin_amdgcn_fdot2_f32_bf16(m, lo, r0, false);
  l[1] = (__bf16)__builtin_amdgcn_fdot2_f32_bf16(m, hi, r1, false);
}

// (file-local to each unit that includes this header -- every one is a single device unit -- so that the kernels templated on a
// format keep one name in every profile: attention_x3_kernel<32, FmtH2>)
namespace {

// FmtX3: x = h + m + l in bf16 (8 significant bits each), six of the nine term products -- fp32 products to ~2^-24, any exponent.
struct FmtX3 {
  static constexpr int NP = 3, NT = 6;
  static constexpr bool SCALED = false;
  typedef __bf16 T;
  typedef __bf16 x8 __attribute__((ext_vector_type(8)));
  typedef __bf16 x4 __attribute__((ext_vector_type(4)));
  typedef __bf16 x2 __attribute__((ext_vector_type(2)));
  // term products, smallest first: planes (A, B) = (m,m) (h,l) (l,h) (h,m) (m,h) (h,h)
  static __device__ __forceinline__ constexpr int pa(int i) { constexpr int t[6] = {1, 0, 2, 0, 1, 0}; return t[i]; }
  static __device__ __forceinline__ constexpr int pb(int i) { constexpr int t[6] = {1, 2, 0, 1, 0, 0}; return t[i]; }
  static __device__ __forceinline__ void split(float x0, float x1, x2 (&pl)[3]) { split3_pair(x0, x1, pl[0], pl[1], pl[2]); }
  static __device__ __forceinline__ f32x16 mfma(x8 a, x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};
// FmtH2 (round 4): x s = h + m in fp16 (11 significant bits each: 22 bits, truncation 2^-22 |x|), THREE term products (h,m) (m,h)
// (h,h) -- half the MFMAs of FmtX3 and a split of 2 instead of 3.5 VALU instructions per value (v_cvt_pk_f16_f32 rounds and packs
// two values, the residual x - h is one v_dot2c_f32_f16 per value, exact).  fp16 has five exponent bits, so every operand is
// scaled by a power of two s that brings a bound of its |values| to [2^13, 2^14) (pow2_scale below; the attention takes the q, k, v
// maxima of a (side, pair) over its valid rows, AttnArgs::amax): every value within 2^-17 of the maximum keeps its 22 bits, smaller
// ones are exact to 2^-39 of the maximum; the attention's P (<= 1) is scaled by 2^15 inside its exponential.  The powers of two cancel
// exactly (one fma in the softmax, the final 1 / l).  Against a float64 evaluation the attention's result is as close as the
// six-product bf16 form's on P.V (P's own rounding in fp32 dominates both) and 0.66 x the fp32-MFMA kernel's error on Q.K^T
// (tools/f16_split_emul.py; tools/ubench/attn_x3_bench.cpp measures all three kernels).
struct FmtH2 {
  static constexpr int NP = 2, NT = 3;
  static constexpr bool SCALED = true;
  typedef _Float16 T;
  typedef _Float16 x8 __attribute__((ext_vector_type(8)));
  typedef _Float16 x4 __attribute__((ext_vector_type(4)));
  typedef _Float16 x2 __attribute__((ext_vector_type(2)));
  static __device__ __forceinline__ constexpr int pa(int i) { constexpr int t[3] = {0, 1, 0}; return t[i]; }
  static __device__ __forceinline__ constexpr int pb(int i) { constexpr int t[3] = {1, 0, 0}; return t[i]; }
  // (The residual and its conversion as one mixed-precision fma each -- v_fma_mixlo_f16 / v_fma_mixhi_f16, three instructions instead
  // of four, the same bits -- measured the same in conv3x3_wino24p.hip: 1917 vs 1916 us on conv2a.)
  static __device__ __forceinline__ void split(float x0, float x1, x2 (&pl)[2]) {
    unsigned lo_u, hi_u;
    asm("s_mov_b32 %0, 0x0000bc00" : "=s"(lo_u));
    asm("s_mov_b32 %0, 0xbc000000" : "=s"(hi_u));
    const x2 lo = __builtin_bit_cast(x2, lo_u), hi = __builtin_bit_cast(x2, hi_u);
    pl[0][0] = (_Float16)x0; pl[0][1] = (_Float16)x1;                                  // v_cvt_pk_f16_f32 (round to nearest even)
    const float r0 = __builtin_amdgcn_fdot2(pl[0], lo, x0, false);                     // x0 - h0, exact
    const float r1 = __builtin_amdgcn_fdot2(pl[0], hi, x1, false);
    pl[1][0] = (_Float16)r0; pl[1][1] = (_Float16)r1;
  }
  static __device__ __forceinline__ f32x16 mfma(x8 a, x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};

// FmtH2's scale: the power of two that brings a bound (> 0; as a bit pattern, or as a float) of a tensor's |values| to [2^13, 2^14);
// exponents clamped so that the scale, the product of two scales and their reciprocals stay normal fp32 numbers (bound in
// [2^-37, 2^73]: outside, fp32 arithmetic on such a tensor is itself degenerate)
__device__ __forceinline__ float pow2_scale(unsigned bound_bits) {
  unsigned e = (bound_bits >> 23) & 0xffu;
  e = e < 90u ? 90u : e > 200u ? 200u : e;
  return __builtin_bit_cast(float, (267u - e) << 23);
}
__device__ __forceinline__ float pow2_scale(float bound) { return pow2_scale(__builtin_bit_cast(unsigned, bound)); }

}  // namespace
}  // namespace imx
