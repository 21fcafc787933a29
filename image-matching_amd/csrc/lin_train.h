// lin_train.h -- launchers of lin_train.hip, kernels of libimx_train.so (include/imx_train.h): nn.Conv1d(kernel_size=1) on
// torch.cat([x0, x1], 1) in its training form, forward and the three gradients.  DESIGN.md section 15 has the formulas, the launch
// structure and the summation orders.
#pragma once
#include <hip/hip_runtime.h>

namespace imx {

constexpr int kLinTile = 64;        // a workgroup's tile: 64 x 64 of (output channel, column), (input channel, column) or (output, input channel)
constexpr int kLinSlab = 256;       // columns of one lin_dw workgroup: two summation blocks of 128

// x0 (B,C0,N), x1 (B,C1,N) or null with C1 = 0, y and dy (B,Cout,N), w (Cout, C0+C1) row-major, bias (Cout) or null; n: (B) counts or
// null = N, clamped to the frame.  part: (B, slabs, Cout, C0+C1+1) scratch of lin_dw, slabs = lin_slabs(N); column C0+C1 carries db.
struct LinArgs {
  const float* x0; const float* x1; const float* w; const float* bias; const float* dy;
  const int* n;
  int B, Cout, C0, C1, N;
  float* y;                           // forward: written in full (0 past the count)
  float* dx0; float* dx1;             // written in full (0 past the count); either may be null
  float* dw; float* db;               // overwritten by launch_lin_dw_reduce; either may be null
  float* part;
};

inline int lin_slabs(int N) { return (N + kLinSlab - 1) / kLinSlab; }
inline size_t lin_part_floats(int B, int Cout, int Cin, int N) { return (size_t)B * lin_slabs(N) * Cout * (Cin + 1); }

hipError_t launch_lin_fwd(const LinArgs& a, hipStream_t s);           // y
hipError_t launch_lin_dx(const LinArgs& a, hipStream_t s);            // dx0 and / or dx1
hipError_t launch_lin_dw(const LinArgs& a, hipStream_t s);            // part: one (Cout, Cin+1) partial per (pair, slab)
hipError_t launch_lin_dw_reduce(const LinArgs& a, hipStream_t s);     // dw and / or db from part: slabs ascending, then pairs ascending

}  // namespace imx
