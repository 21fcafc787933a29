// bn2d_train.h -- launchers of bn2d_train.hip, kernels of libimx_spnorm.so (include/imx_spnorm.h): nn.BatchNorm2d, optionally followed by
// nn.ReLU, in its training form on NCHW maps, forward and backward, the work split over pixels.  DESIGN.md section 19 has the formulas,
// the launch structure and the summation orders.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace imx {

constexpr int kBn2dThreads = 256;   // one workgroup of four waves per slab
constexpr int kBn2dSlab = 4096;     // consecutive pixels of one (image, channel) per workgroup: 256 threads x 4 quads x 4 values
constexpr int kBn2dFinal = 64;      // threads of a finalize workgroup: one wave per channel, a lane per image of a group of 64

// x, y, dy, dx (B,C,HW): the flat view of NCHW maps; gamma, beta, mean, rstd, dgamma, dbeta, running_mean, running_var (C).
// train: 1 = batch statistics (and the running statistics are updated where given), 0 = the running statistics.  relu: 1 = y = max(z, 0).
// part: (C, B, slabs, 2) scratch, slabs = bn2d_slabs(HW): (mean, M2) of a slab in the forward, (sum g, sum g xhat) in the backward; the
// backward's finalize leaves the channel's two totals in the channel's first pair, where bn2d_bwd_dx reads them.
struct Bn2dArgs {
  const float* x; const float* gamma; const float* beta; const float* dy;
  int B, C, HW, relu, train;
  float eps, momentum;
  float* running_mean; float* running_var;      // forward: read in evaluation mode, updated in place in training mode; either may be null in training mode
  long long* num_batches_tracked;               // forward, training mode: + 1 by one thread, or null
  float* y; float* mean; float* rstd;           // forward
  const float* mean_in; const float* rstd_in;   // backward: what the forward wrote
  float* dx; float* dgamma; float* dbeta;       // backward; dgamma and dbeta may be null
  float* part;
};

__host__ __device__ inline int bn2d_slabs(int HW) { return (HW + kBn2dSlab - 1) / kBn2dSlab; }
inline size_t bn2d_part_floats(int B, int C, int HW) { return 2 * (size_t)B * C * bn2d_slabs(HW); }
// the 16-byte form of a streaming kernel: every map's run starts on a 16-byte boundary.  Both forms visit the same values in the same
// order with the same operations, so the choice does not reach the bits.
inline bool bn2d_x4(int HW, const void* p, const void* q = nullptr, const void* r = nullptr) {
  return HW % 4 == 0 && ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(r)) & 15) == 0;
}

hipError_t launch_bn2d_stats(const Bn2dArgs& a, hipStream_t s);           // part: (mean, M2) per slab
hipError_t launch_bn2d_finalize(const Bn2dArgs& a, hipStream_t s);        // mean, rstd, the running statistics from part
hipError_t launch_bn2d_apply(const Bn2dArgs& a, hipStream_t s);           // y (evaluation mode: mean and rstd too)
hipError_t launch_bn2d_bwd_sums(const Bn2dArgs& a, hipStream_t s);        // part: (sum g, sum g xhat) per slab
hipError_t launch_bn2d_bwd_finalize(const Bn2dArgs& a, hipStream_t s);    // the totals into part, and dgamma / dbeta where given
hipError_t launch_bn2d_bwd_dx(const Bn2dArgs& a, hipStream_t s);          // dx

}  // namespace imx
