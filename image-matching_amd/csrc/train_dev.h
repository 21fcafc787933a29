// train_dev.h -- the helpers that more than one training kernel file (libimx_train.so, libimx_sgtrain.so, libimx_spnet.so) uses with the
// same operations in the same order: the operands and accumulator of v_mfma_f32_32x32x2_f32 (lin_train.hip, mha_train.hip,
// score_train.hip, conv3_train.hip), the butterfly sum over a wave (bn_train.hip,
// otgrad.hip) and the host's grid division.  Everything is inlined at its call: no symbol of a code object comes from here.
#pragma once
#include <hip/hip_runtime.h>

namespace imx {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// a count read on the device, clamped to its frame [0, hi]
__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }
// the row of a 32x32 accumulator that register r of a lane in half hi (lane >> 5) holds; its column is lane & 31
__device__ __forceinline__ int crow(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }
__device__ __forceinline__ f32x16 zero16() {
  const f32x16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  return z;
}
__device__ __forceinline__ f32x16 mma(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

// the sum over the 64 lanes of a wave, xor 32, 16, 8, 4, 2, 1: every lane ends with the same bits.  (otgrad.hip's own copy was a plain
// `inline` loop without the unroll pragma: the same six adds in the same order, and with the present compiler the same code bytes --
// the gfx950 .text of otgrad.hip did not change when it moved here.  The order of the adds is the contract, the bytes are not.)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

inline int cdiv(int a, int b) { return (a + b - 1) / b; }

}  // namespace imx
