// bn_train.h -- launchers of bn_train.hip, kernels of libimx_train.so (include/imx_train.h): nn.BatchNorm1d followed by nn.ReLU in
// their training form, forward and backward, one launch each.  DESIGN.md section 16 has the formulas, the launch structure and the
// summation orders.
#pragma once
#include <hip/hip_runtime.h>

namespace imx {

constexpr int kBnThreads = 256;     // one workgroup of four waves per channel
constexpr int kBnSlots = 16;        // values a thread holds in registers in the register form

// x, y, dy, dx (B,C,N); gamma, beta, mean, rstd, dgamma, dbeta, running_mean, running_var (C); n: (B) counts or null = N, clamped to the
// frame.  train: 1 = batch statistics (and the running statistics are updated where given), 0 = the running statistics.
struct BnArgs {
  const float* x; const float* gamma; const float* beta; const float* dy;
  const int* n;
  int B, C, N, train;
  float eps, momentum;
  float* running_mean; float* running_var;      // forward: read in evaluation mode, updated in place in training mode; either may be null in training mode
  long long* num_batches_tracked;               // forward, training mode: + 1 by one thread, or null
  float* y; float* mean; float* rstd;           // forward: y written in full (0 past the count)
  const float* mean_in; const float* rstd_in;   // backward: what the forward wrote
  float* dx; float* dgamma; float* dbeta;       // backward: dx written in full (0 past the count); any may be null
};

// a thread's columns of a pair are t, t + 256, ...: ceil(N / 256) slots per pair.  When all B pairs fit in kBnSlots slots the channel's
// values stay in registers between the passes; otherwise the passes read them again.  Both forms visit the valid values in the same
// order, so the choice (a function of the frame) does not reach the bits.
inline bool bn_in_registers(int B, int N) { return (long long)B * ((N + kBnThreads - 1) / kBnThreads) <= kBnSlots; }

hipError_t launch_bn_relu_fwd(const BnArgs& a, hipStream_t s);        // y, mean, rstd, the running statistics
hipError_t launch_bn_relu_bwd(const BnArgs& a, hipStream_t s);        // dx, dgamma, dbeta

}  // namespace imx
