// pack_host.h -- host-only helpers shared by the weight packers (wino24_pack.h, gnn_tail_pack.h, imx_weights.cpp): bit-pattern
// conversions to fp16 / bf16, the power-of-two scale of the fp16-plane forms, the spread statistic their guards read, and the
// B-fragment index of the 32x32x16 MFMAs.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace imx {

// fp32 -> fp16 bit pattern, round to nearest even (subnormals and overflow to infinity included)
inline uint16_t f16_rne(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  const uint32_t sign = (u >> 16) & 0x8000u;
  u &= 0x7fffffffu;
  if (u >= 0x7f800000u) return (uint16_t)(sign | (u > 0x7f800000u ? 0x7e00u : 0x7c00u));
  if (u >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                     // rounds to 65536 or more
  if (u < 0x38800000u) {                                                       // below 2^-14: subnormal result
    if (u < 0x33000000u) return (uint16_t)sign;                                // below 2^-25
    const int e = (int)(u >> 23);
    const uint32_t m = (u & 0x7fffffu) | 0x800000u;
    const int sh = 126 - e;                                                    // 14 .. 24
    const uint32_t q = m >> sh, rem = m & ((1u << sh) - 1u), half = 1u << (sh - 1);
    return (uint16_t)(sign | (q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u)));
  }
  const uint32_t r = u + 0xfffu + ((u >> 13) & 1u);
  return (uint16_t)(sign | ((r - 0x38000000u) >> 13));
}
inline float f16_to_f32(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
  uint32_t u;
  if (e == 0) {
    if (m == 0) u = sign;
    else { float f = (float)m * 5.9604644775390625e-8f; memcpy(&u, &f, 4); u |= sign; }
  } else if (e == 31) u = sign | 0x7f800000u | (m << 13);
  else u = sign | ((e + 112u) << 23) | (m << 13);
  float f;
  memcpy(&f, &u, 4);
  return f;
}

// fp32 -> bf16 bit pattern, round to nearest even (Inf / NaN keep their upper half)
inline uint16_t bf16_rne(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  if ((u & 0x7F800000u) == 0x7F800000u) return (uint16_t)(u >> 16);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
inline float bf16_to_f32(uint16_t b) {
  const uint32_t u = (uint32_t)b << 16;
  float x;
  memcpy(&x, &u, 4);
  return x;
}

// The power of two s that brings mx to [2^13, 2^14): mx = f 2^e with f in [0.5, 1), s = 2^(14 - e)  (mx = 0: 2^14)
inline double pow2_scale_for(double mx) {
  int e = 0;
  if (mx > 0) std::frexp(mx, &e);
  return std::ldexp(1.0, 14 - e);
}

// The spread statistic of the fp16-plane guards: mx (the largest value) over the median of v (one value per output channel, element
// size / 2 in sorted order) -- how far the typical channel sits below the one scale its matrix carries.  zero_median: what a zero
// median under a nonzero maximum counts as (each caller's cap; callers that cap the ratio itself do so with the same value).
inline double spread_over_median(std::vector<double> v, double mx, double zero_median) {
  std::nth_element(v.begin(), v.begin() + v.size() / 2, v.end());
  const double med = v[v.size() / 2];
  return med > 0 ? mx / med : (mx > 0 ? zero_median : 1.0);
}

// B operand of v_mfma_f32_32x32x16_{bf16,f16}: W[k][n] of a [K][Npad] matrix held as `planes` 16-bit planes sits at
// [column block of 32][16-k step][plane][lane = (n & 31) + 32 kb][8], lane (n, kb) holding W[16 st + 8 kb + j][32 nb + (n & 31)], j = 0..7
inline size_t b_fragment_index(int k, int n, int K, int planes, int plane) {
  const int nb = n >> 5, st = k >> 4, lane = (n & 31) + 32 * ((k >> 3) & 1), j = k & 7;
  return ((((size_t)nb * (K / 16) + st) * planes + plane) * 64 + lane) * 8 + j;
}

}  // namespace imx
