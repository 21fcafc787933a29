// imx_speval.cpp -- the host unit of libimx_speval.so (include/imx_speval.h), on the handle libimx.so made: the argument checks of the
// mutual nearest-neighbour matcher and of the pair metrics, and their launches (speval.hip).  Workspace: "speval.nn" (4 B (N0 + N1)
// bytes, the two directions' neighbours), written by the call before it is read.
#include "imx_host.h"
#include "speval.h"
#include "../../include/imx_speval.h"

extern "C" {

int imx_mutual_nn_match(imx_handle_t h, int B, int D, const float* desc0_dev, int64_t s0_b, int64_t s0_c, int64_t s0_n, const int32_t* n0_dev,
                        int N0, const float* desc1_dev, int64_t s1_b, int64_t s1_c, int64_t s1_n, const int32_t* n1_dev, int N1,
                        int64_t* matches0_dev, int64_t* matches1_dev, float* sim0_dev, float* sim1_dev, void* stream) {
  return on_device(h, "imx_mutual_nn_match", [&]() -> int {
    const char* who = "imx_mutual_nn_match";
    hipStream_t s = as_stream(stream);
    if (B < 1 || B > (1 << 16) || N0 < 1 || N1 < 1 || N0 > (1 << 20) || N1 > (1 << 20))
      return fail(h, "%s: bad shape B=%d N0=%d N1=%d (B in [1,2^16], N0 and N1 in [1,2^20])", who, B, N0, N1);
    if (D < 1 || D > kSpevalMaxDim) return fail(h, "%s: D=%d outside [1,%d]", who, D, kSpevalMaxDim);
    if (!desc0_dev || !desc1_dev || !matches0_dev || !matches1_dev || !sim0_dev || !sim1_dev) return fail(h, "%s: null argument", who);
    WS(nn, int, "speval.nn", (size_t)B * ((size_t)N0 + N1) * sizeof(int));
    int* nn0 = nn;
    int* nn1 = nn + (size_t)B * N0;
    MnnSearchArgs a{};
    a.B = B; a.D = D;
    a.q = desc0_dev; a.qb = s0_b; a.qc = s0_c; a.qn = s0_n; a.nq = n0_dev; a.Nq = N0;
    a.k = desc1_dev; a.kb = s1_b; a.kc = s1_c; a.kn = s1_n; a.nk = n1_dev; a.Nk = N1;
    a.nn = nn0; a.sim = sim0_dev;
    RUN("mnn_search_0", launch_mnn_search(a, s));
    MnnSearchArgs r{};                       // the same kernel with the sides swapped: sim(i, j) has the same bits in both directions
    r.B = B; r.D = D;
    r.q = desc1_dev; r.qb = s1_b; r.qc = s1_c; r.qn = s1_n; r.nq = n1_dev; r.Nq = N1;
    r.k = desc0_dev; r.kb = s0_b; r.kc = s0_c; r.kn = s0_n; r.nk = n0_dev; r.Nk = N0;
    r.nn = nn1; r.sim = sim1_dev;
    RUN("mnn_search_1", launch_mnn_search(r, s));
    RUN("mnn_mutual", launch_mnn_mutual(nn0, nn1, B, N0, N1, reinterpret_cast<long long*>(matches0_dev), reinterpret_cast<long long*>(matches1_dev), s));
    return 0;
  });
}

int imx_keypoint_pair_metrics(imx_handle_t h, const float* kpts0_dev, const int32_t* n0_dev, const float* kpts1_dev, const int32_t* n1_dev,
                              const int64_t* matches0_dev, const double* H_gt_dev, int B, int K0, int K1, int width, int height, double eps,
                              int32_t* counts_dev, double* sums_dev, void* stream) {
  return on_device(h, "imx_keypoint_pair_metrics", [&]() -> int {
    const char* who = "imx_keypoint_pair_metrics";
    hipStream_t s = as_stream(stream);
    if (B < 1 || B > (1 << 20) || K0 < 1 || K1 < 1 || width < 1 || height < 1)
      return fail(h, "%s: bad shape B=%d K0=%d K1=%d width=%d height=%d", who, B, K0, K1, width, height);
    if (K0 > kSpevalMaxK || K1 > kSpevalMaxK)
      return fail(h, "%s: K0=%d K1=%d above the limit of %d keypoints a side (both sides are staged in LDS as float64)", who, K0, K1, kSpevalMaxK);
    if (!(eps >= 0.0) || !(eps < 1e300)) return fail(h, "%s: eps must be non-negative and finite", who);
    if (!kpts0_dev || !kpts1_dev || !H_gt_dev || !counts_dev || !sums_dev) return fail(h, "%s: null argument", who);
    PairMetricArgs a{};
    a.kpts0 = kpts0_dev; a.n0 = n0_dev; a.kpts1 = kpts1_dev; a.n1 = n1_dev; a.matches0 = reinterpret_cast<const long long*>(matches0_dev);
    a.H = H_gt_dev; a.B = B; a.K0 = K0; a.K1 = K1; a.width = width; a.height = height; a.eps = eps;
    a.counts = counts_dev; a.sums = sums_dev;
    RUN("pair_metrics", launch_pair_metrics(a, s));
    return 0;
  });
}

}  // extern "C"
