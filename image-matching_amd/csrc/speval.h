// speval.h -- launchers of speval.hip, kernels of libimx_speval.so (include/imx_speval.h): the mutual nearest-neighbour descriptor
// matcher (a brute-force matcher with cross-check, the similarity matrix never stored) and the pair metrics of SuperPoint's validation
// under a known warp (shared-view filter, repeatability counts, localisation sums, correctness of matches).  DESIGN.md section 25 has
// the definitions, the tie rules, the launch structure and the resource usage.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace imx {

constexpr int kSpevalTile = 64;             // query rows of a workgroup of the search, and keys of one of its tiles
constexpr int kSpevalMaxDim = 1024;         // descriptor channels
constexpr int kSpevalMaxK = 4096;           // keypoints a side of the pair metrics: both sides' positions are staged in LDS as float64
constexpr int kSpevalMetricThreads = 1024;

// one direction of the search: for every query row i < Nq of every pair, the lowest key j < nk attaining max_j sum_c q[i,c] k[j,c]
struct MnnSearchArgs {
  const float* q; long long qb, qc, qn;     // element (b, c, i) of the query side at b*qb + c*qc + i*qn
  const float* k; long long kb, kc, kn;     // the key side likewise
  const int* nq; const int* nk;             // (B) counts or null = the frame; rows past a count are never read
  int B, D, Nq, Nk;
  int* nn;                                  // (B,Nq): the neighbour, -1 = none (past the count, no key, or no comparable similarity)
  float* sim;                               // (B,Nq): its similarity, 0 where nn is -1
};
hipError_t launch_mnn_search(const MnnSearchArgs& a, hipStream_t s);
// matches0[i] = nn0[i] if nn1[nn0[i]] == i else -1, and matches1 likewise
hipError_t launch_mnn_mutual(const int* nn0, const int* nn1, int B, int N0, int N1, long long* matches0, long long* matches1, hipStream_t s);

struct PairMetricArgs {
  const float* kpts0; const int* n0;        // (B,K0,2), (B) or null = K0
  const float* kpts1; const int* n1;        // (B,K1,2), (B) or null = K1
  const long long* matches0;                // (B,K0) or null
  const double* H;                          // (B,9), pixels of image 0 to pixels of image 1
  int B, K0, K1, width, height;
  double eps;
  int* counts;                              // (B,8): v0, v1, r0, r1, m, c, bad, 0
  double* sums;                             // (B,2)
};
hipError_t launch_pair_metrics(const PairMetricArgs& a, hipStream_t s);

}  // namespace imx
