// sppool_train.h -- launchers of sppool_train.hip, kernels of libimx_sppool.so (include/imx_sppool.h): nn.MaxPool2d(2) and the descriptor
// normalisation desc / ||desc||_2 of SuperPoint's training step on NCHW maps, forward and backward.  DESIGN.md section 20 has the formulas,
// the launch structure and the summation order.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace imx {

constexpr int kPoolThreads = 256;   // a workgroup of the pooling kernels: 256 items of one (image, channel) plane
constexpr int kL2Lanes = 64;        // lanes of an l2norm workgroup along pixels (one wave wide) ...
constexpr int kL2Groups = 4;        // ... times its waves along channels: wave g takes the channels g, g + 4, g + 8, ...

// x, dx (B,C,H,W); y, dy (B,C,H/2,W/2) (floor); idx (B,C,H/2,W/2) bytes, 2 row + col of the window's maximum, null in an evaluation forward
struct PoolArgs {
  const float* x; float* y; uint8_t* idx;                       // forward
  const uint8_t* idx_in; const float* dy; float* dx;            // backward
  int B, C, H, W;
};

// x, y, dy, dx (B,C,HW); norm (B,HW)
struct L2Args {
  const float* x; float* y; float* norm;                        // forward
  const float* y_in; const float* norm_in; const float* dy; float* dx;   // backward
  int B, C, HW;
};

inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
// the 16-byte form of the pooling kernels: every row of x / dx and of y / dy starts on a 16-byte boundary and holds whole quads of outputs
// (W % 8 == 0), and a quad of index bytes is one aligned word.  Both forms scan a window in the same order with the same comparisons, so
// the choice does not reach the bits.
inline bool pool_x4(int W, const void* full, const void* half, const void* idx) {
  return W % 8 == 0 && aligned_to(full, 16) && aligned_to(half, 16) && aligned_to(idx, 4);
}
// the 16-byte form of the normalisation kernels: a lane holds four consecutive pixels.  Taken from 2^16 pixels on only: below that the
// quad grid has fewer workgroups than the device has compute units.  A pixel's operations are the same in both forms.
inline bool l2_x4(int B, int HW, const void* p, const void* q, const void* r = nullptr, const void* s = nullptr) {
  return HW % 4 == 0 && (long long)B * HW >= (1 << 16) && aligned_to(p, 16) && aligned_to(q, 16) && aligned_to(r, 16) && aligned_to(s, 16);
}

hipError_t launch_maxpool2_fwd(const PoolArgs& a, hipStream_t s);    // y, and idx where given
hipError_t launch_maxpool2_bwd(const PoolArgs& a, hipStream_t s);    // dx, every element
hipError_t launch_l2norm_fwd(const L2Args& a, hipStream_t s);        // y, norm
hipError_t launch_l2norm_bwd(const L2Args& a, hipStream_t s);        // dx

}  // namespace imx
