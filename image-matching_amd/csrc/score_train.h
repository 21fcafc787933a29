// score_train.h -- launchers of score_train.hip, kernels of libimx_sgtrain.so (include/imx_sgtrain.h): the score product of SuperGlue's
// training step, scores = einsum('bdn,bdm->bnm', mdesc0, mdesc1) * scale, forward and the two gradients.  DESIGN.md section 17 has the
// formulas, the launch structure and the summation orders.
#pragma once
#include <hip/hip_runtime.h>

namespace imx {

constexpr int kScoreTile = 64;      // a workgroup's tile: 64 x 64 of (row n, column m), (channel d, column m) or (channel d, row n)

// a (B,D,N0), b (B,D,N1), s and ds (B,N0,N1), da the shape of a, db the shape of b; n0, n1: (B) counts or null = N0 / N1, clamped to
// the frame.  Every output is written in full, with 0 past the counts.
struct ScoreTrainArgs {
  const float* a; const float* b; const float* ds;
  const int* n0; const int* n1;
  int B, D, N0, N1;
  float scale;
  float* s;                           // forward
  float* da; float* db;               // backward; each launcher needs its own only
};

hipError_t launch_score_fwd(const ScoreTrainArgs& a, hipStream_t s);          // s
hipError_t launch_score_da(const ScoreTrainArgs& a, hipStream_t s);           // da
hipError_t launch_score_db(const ScoreTrainArgs& a, hipStream_t s);           // db

}  // namespace imx
