// mha_train.h -- launchers of mha_train.hip, kernels of libimx_train.so (include/imx_train.h): the attention of SuperGlue's GNN in
// its training form, a forward that keeps the row log-sum-exp and the backward that recomputes the probabilities from it.  DESIGN.md
// section 14 has the formulas, the launch structure and the summation orders.
#pragma once
#include <hip/hip_runtime.h>

namespace imx {

// Tensors are (B, D, H, n) contiguous fp32, element (b, c, h, n) at ((b D + c) H + h) n_frame + n: q, out, dout, dq over N queries,
// k, v, dk, dv over M keys.  lse and delta are (B, H, N).  nq / nk: (B) counts or null = N / M, clamped to the frame.
struct MhaArgs {
  const float* q; const float* k; const float* v;
  const int* nq; const int* nk;
  int B, H, D, N, M;
  float scale;                        // 1 / sqrt(D)
  float* out; float* lse;             // forward: written in full (0 past the counts); lse may be null
  const float* o_in; const float* lse_in; const float* dout;   // backward inputs
  float* delta;                       // (B, H, N) scratch: written in full by launch_mha_delta, read by the two kernels after it
  float* dq; float* dk; float* dv;    // written in full (0 past the counts); dk or dv may be null in launch_mha_dkdv
};

bool mha_head_dim_ok(int D);                                          // 16, 32 or 64
hipError_t launch_mha_fwd(const MhaArgs& a, hipStream_t s);           // out, lse
hipError_t launch_mha_delta(const MhaArgs& a, hipStream_t s);         // delta = rowsum(dout o out)
hipError_t launch_mha_dkdv(const MhaArgs& a, hipStream_t s);          // per key block, query tiles ascending: dk and / or dv
hipError_t launch_mha_dq(const MhaArgs& a, hipStream_t s);            // per query block, key tiles ascending: dq

}  // namespace imx
