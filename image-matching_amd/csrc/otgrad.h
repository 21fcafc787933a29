// otgrad.h -- launchers of otgrad.hip, kernels of libimx_train.so (include/imx_train.h): the SuperGlue match loss through the
// unrolled log-domain Sinkhorn as a value-and-gradient call.  DESIGN.md section 13 has the derivative rules and the summation orders.
#pragma once
#include <hip/hip_runtime.h>

namespace imx {

// One pair b: m = n0[b], n = n1[b] (clamped to [0,N0] / [0,N1]); the coupling matrix C is (m+1) x (n+1), scores inside and bin_score
// in the last row and column; it is never materialised.  A pair with m = 0 or n = 0 has loss 0 and zero gradients.
struct OtArgs {
  const float* scores;                      // (B,N0,N1); rows past m and columns past n are never read
  const int* n0; const int* n1;             // (B) counts, or null = N0 / N1
  const float* bin;                         // one float: bin_score
  int B, N0, N1, T;
  const long long* all_matches; const int* n_all; int L;   // (B,2,L), (B); entries past n_all are never read
  const float* gout;                        // (B) upstream cotangents, or null = 1
  float* loss; float* grad; float* grad_bin; int* flag;    // (B), (B,N0,N1) or null = the value only, (B), (B)
  // scratch, every element that is read is written by the same call
  float* U; float* V;                       // (B,T+1,N0+1) / (B,T+1,N1+1): the potentials u_t, v_t of every iteration, t = 0 the zeros
  float* UB; float* VB;                     // the same shapes: the cotangents u-bar_t (t = 1..T; slot 0 = the seed G 1) and v-bar_t
  int* cnt_row; int* cnt_col;               // (B,N0+1) / (B,N1+1): listings per row x and per column y of C
  int* cnt_bin;                             // (B,N0+N1+1): listings on the dustbin row (y = 0..n, the corner at n), then on the dustbin column
  float* binv;                              // (B,N0+N1+1): C-bar on the dustbin row, then on the dustbin column, for grad_bin
};
// the normaliser of Z = C + u_T + v_T - norm for a pair with counts m, n: ONE expression, shared by otgrad.hip (the loss reads Z through it)
// and sgloop.hip (the matches are extracted from the same Z), so that both form the same bits
__device__ __forceinline__ float ot_norm(int m, int n) { return -logf((float)(m + n)); }
constexpr int kOtFlagIndex = 1;             // bit 0 of flag: a listed index outside the coupling matrix (the entry contributes nothing)

hipError_t launch_ot_init(const OtArgs& a, hipStream_t s);            // u_0 = v_0 = 0, the counts zeroed (and grad, which first holds counts)
hipError_t launch_ot_row_lse(const OtArgs& a, int t, hipStream_t s);  // u_t from v_{t-1}
hipError_t launch_ot_col_lse(const OtArgs& a, int t, hipStream_t s);  // v_t from u_t
hipError_t launch_ot_gather(const OtArgs& a, hipStream_t s);          // loss, flag, the counts
hipError_t launch_ot_seed(const OtArgs& a, hipStream_t s);            // u-bar = G 1, v-bar_T = G^T 1
hipError_t launch_ot_row_bwd(const OtArgs& a, int t, hipStream_t s);  // u-bar_t from v-bar_t
hipError_t launch_ot_col_bwd(const OtArgs& a, int t, hipStream_t s);  // v-bar_{t-1} from u-bar_t
hipError_t launch_ot_assemble(const OtArgs& a, hipStream_t s);        // C-bar: grad in full, binv
hipError_t launch_ot_bin(const OtArgs& a, hipStream_t s);             // grad_bin = the sum of binv in a fixed order

}  // namespace imx
