// sploop.h -- launchers of sploop.hip, kernels of libimx_sploop.so (include/imx_sploop.h): the bilinear label splat of SuperPoint's
// gaussian_label and the flat Adam step.  DESIGN.md section 22 has the arithmetic, the launch structure and the duplicate rule.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace imx {

struct LabelsBiArgs {
  const float* pts;          // (B,Kcap,2) (x, y)
  const int32_t* counts;     // (B) or null = Kcap
  const float* mats;         // (B,3,3) pixel space
  float* out;                // (B,H,W)
  int32_t* owner;            // (B,H,W) workspace: the highest order index k * count + i that landed on the pixel, -1 = none
  int32_t* flag;             // bit 0: a kept weight outside [0,1]; bit 1: a non-finite warped point; may be null
  int B, Kcap, H, W, levels;
};
hipError_t launch_labels_bi(const LabelsBiArgs& a, hipStream_t s);   // three launches: fill, claim, write

struct AdamArgs {
  float *p, *g, *m, *v;
  int64_t n;
  float step_size, beta1, c1, beta2, c2, inv_sqrt_bc2, eps, weight_decay;   // c1 = 1 - beta1, c2 = 1 - beta2, rounded from double
  int zero_grad;
};
constexpr int kAdamThreads = 256;
inline bool adam_x4(const AdamArgs& a) {
  return ((reinterpret_cast<uintptr_t>(a.p) | reinterpret_cast<uintptr_t>(a.g) | reinterpret_cast<uintptr_t>(a.m) | reinterpret_cast<uintptr_t>(a.v)) & 15) == 0;
}
hipError_t launch_adam_flat(const AdamArgs& a, hipStream_t s);       // one launch; n = 0: none

}  // namespace imx
