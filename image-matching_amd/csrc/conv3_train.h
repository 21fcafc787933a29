// conv3_train.h -- launchers of conv3_train.hip, kernels of libimx_spnet.so (include/imx_spnet.h): nn.Conv2d(Cin, Cout, 3, padding=1) in
// its training form, forward and the three gradients.  DESIGN.md section 18 has the formulas, the launch structure and the summation
// orders.
#pragma once
#include <hip/hip_runtime.h>

namespace imx {

constexpr int kC3Chan = 64;         // conv3_fwd / conv3_dx: output channels of a workgroup's tile (two blocks of 32 per wave)
constexpr int kC3Rows = 8;          //   image rows of the tile (two per wave)
constexpr int kC3Cols = 32;         //   image columns of the tile (on the lanes)
constexpr int kC3Chunk = 8;         //   summation channels staged through LDS at a time; two chunks form one MFMA chain of 72 steps
constexpr int kC3Tile = 64;         // conv3_dw: 64 output channels x 64 columns (c, u, v) of the weight gradient per workgroup
constexpr int kC3Slab = 16;         // conv3_dw: image rows of one workgroup's sum

// x (B,Cin,H,W), w (Cout,Cin,3,3), bias (Cout) or null, y and dy (B,Cout,H,W), dx the shape of x, dw the shape of w, db (Cout): NCHW,
// contiguous.  part: (B, slabs, Cout, 9 Cin + 1) scratch of conv3_dw, slabs = conv3_slabs(H); column 9 Cin carries db.
struct Conv3Args {
  const float* x; const float* w; const float* bias; const float* dy;
  int B, Cout, Cin, H, W;
  float* y;                           // forward: written in full
  float* dx;                          // written in full
  float* dw; float* db;               // overwritten by launch_conv3_dw_reduce; either may be null
  float* part;
};

inline int conv3_slabs(int H) { return (H + kC3Slab - 1) / kC3Slab; }
// (the scratch does not depend on W: a slab's pixels are summed inside its workgroup)
inline size_t conv3_part_floats(int B, int Cout, int Cin, int H, int W) { (void)W; return (size_t)B * conv3_slabs(H) * Cout * (9 * (size_t)Cin + 1); }
// workgroups of the largest grid any of the launches below would use for this shape
long long conv3_max_grid(int B, int Cout, int Cin, int H, int W);

hipError_t launch_conv3_fwd(const Conv3Args& a, hipStream_t s);           // y
hipError_t launch_conv3_dx(const Conv3Args& a, hipStream_t s);            // dx
hipError_t launch_conv3_dw(const Conv3Args& a, hipStream_t s);            // part: one (Cout, 9 Cin + 1) partial per (image, slab)
hipError_t launch_conv3_dw_reduce(const Conv3Args& a, hipStream_t s);     // dw and / or db from part: slabs ascending, then images ascending

}  // namespace imx
