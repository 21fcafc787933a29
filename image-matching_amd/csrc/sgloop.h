// sgloop.h -- launchers of sgloop.hip, kernels of libimx_sgloop.so (include/imx_sgloop.h): the mutual-argmax match extraction of
// SuperGlue's training forward (superglue/models/superglue_train.py:276-286) from a score matrix and Sinkhorn's final potentials.
// DESIGN.md section 23 has the launch structure, the tie rule and the byte count.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace imx {

// One pair b: m = n0[b], n = n1[b] (clamped to [0,N0] / [0,N1]); Z[i][j] = ((scores[i][j] + u[i]) + v[j]) - ot_norm(m, n) for i < m,
// j < n, never stored.  The dustbin row and column take no part.
struct SglArgs {
  const float* scores;                      // (B,N0,N1); rows past m and columns past n are never read
  const int* n0; const int* n1;             // (B) counts, or null = N0 / N1
  const float* u; const float* v;           // the potentials of pair b start at u + b * su / v + b * sv (floats); null = zeros
  size_t su, sv;
  int B, N0, N1;
  float threshold;
  const long long* gt0;                     // (B,N0) or null (with stats)
  long long* matches0; long long* matches1; // (B,N0) / (B,N1), -1 = none; written in full
  float* mscores0; float* mscores1;         // (B,N0) / (B,N1); written in full
  int* stats;                               // (B,3) [gt0 >= 0, matches0 > -1, matches0 == gt0 >= 0] over i < m, or null
  // scratch, every element that is read is written by the same call
  float* row_val; int* row_idx;             // (B,N0): the maximum of row i over j < n and its lowest column
  int* col_idx;                             // (B,N1): the lowest row of the maximum of column j over i < m
};

hipError_t launch_sgl_row_max(const SglArgs& a, hipStream_t s);   // row_val, row_idx
hipError_t launch_sgl_col_max(const SglArgs& a, hipStream_t s);   // col_idx
hipError_t launch_sgl_mutual(const SglArgs& a, hipStream_t s);    // the mutual test, expf, the threshold, side 1, the padding, the counts

}  // namespace imx
