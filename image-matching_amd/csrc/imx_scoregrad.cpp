// imx_scoregrad.cpp -- the host unit of libimx_sgtrain.so (include/imx_sgtrain.h), on the handle libimx.so made: the score product of
// SuperGlue's training step, einsum('bdn,bdm->bnm', a, b) * scale, forward and the gradients at both inputs.  The kernels are
// score_train.hip's; nothing of libimx.so or libimx_train.so is linked here.  No scratch is drawn from the handle's workspace.
#include "imx_host.h"
#include "score_train.h"
#include "train_dev.h"
#include "../../include/imx_sgtrain.h"

#include <cmath>
#include <cstdint>

namespace {

// the shape rules of both entry points; 0 or the error code with the text set
int check_shape(imx_handle_t h, const char* who, int B, int D, int N0, int N1, float scale) {
  if (B < 1 || B > 65535 || D < 1 || D > 1024 || N0 < 1 || N0 > (1 << 20) || N1 < 1 || N1 > (1 << 20))
    return fail(h, "%s: bad shape B=%d D=%d N0=%d N1=%d (B in [1,65535], D in [1,1024], N0 and N1 in [1,2^20])", who, B, D, N0, N1);
  const long long tiles = (long long)cdiv(N0, kScoreTile) * cdiv(N1, kScoreTile) * B;
  if (tiles > INT32_MAX) return fail(h, "%s: B=%d N0=%d N1=%d is %lld tiles of 64 x 64, more than a grid of 2^31 - 1", who, B, N0, N1, tiles);
  if (!std::isfinite(scale)) return fail(h, "%s: scale must be finite", who);
  return 0;
}

// the byte ranges [p, p + floats) and [q, q + floats) share an address
bool overlap(const float* p, size_t np, const float* q, size_t nq) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return p && q && a < b + nq * sizeof(float) && b < a + np * sizeof(float);
}

ScoreTrainArgs shape_args(int B, int D, int N0, int N1, const float* a_dev, const float* b_dev, const int32_t* n0, const int32_t* n1, float scale) {
  ScoreTrainArgs a{};
  a.a = a_dev; a.b = b_dev; a.n0 = n0; a.n1 = n1; a.B = B; a.D = D; a.N0 = N0; a.N1 = N1; a.scale = scale;
  return a;
}

}  // namespace

extern "C" {

int imx_score_product_forward_train(imx_handle_t h, int B, int D, int N0, int N1, const float* a_dev, const float* b_dev,
                                    const int32_t* n0_dev, const int32_t* n1_dev, float scale, float* scores_dev, void* stream) {
  return on_device(h, "imx_score_product_forward_train", [&]() -> int {
    const char* who = "imx_score_product_forward_train";
    if (check_shape(h, who, B, D, N0, N1, scale)) return -1;
    if (!a_dev || !b_dev || !scores_dev) return fail(h, "%s: null argument", who);
    const size_t na = (size_t)B * D * N0, nb = (size_t)B * D * N1, ns = (size_t)B * N0 * N1;
    if (overlap(scores_dev, ns, a_dev, na) || overlap(scores_dev, ns, b_dev, nb)) return fail(h, "%s: scores aliases an input", who);
    hipStream_t s = as_stream(stream);
    ScoreTrainArgs a = shape_args(B, D, N0, N1, a_dev, b_dev, n0_dev, n1_dev, scale);
    a.s = scores_dev;
    RUN("score_fwd", launch_score_fwd(a, s));
    return 0;
  });
}

int imx_score_product_backward(imx_handle_t h, int B, int D, int N0, int N1, const float* a_dev, const float* b_dev,
                               const float* dscores_dev, const int32_t* n0_dev, const int32_t* n1_dev, float scale, float* da_dev,
                               float* db_dev, void* stream) {
  return on_device(h, "imx_score_product_backward", [&]() -> int {
    const char* who = "imx_score_product_backward";
    if (check_shape(h, who, B, D, N0, N1, scale)) return -1;
    if (!a_dev || !b_dev || !dscores_dev) return fail(h, "%s: null argument", who);
    const size_t na = (size_t)B * D * N0, nb = (size_t)B * D * N1, ns = (size_t)B * N0 * N1;
    if (overlap(da_dev, na, a_dev, na) || overlap(da_dev, na, b_dev, nb) || overlap(da_dev, na, dscores_dev, ns))
      return fail(h, "%s: da aliases an input", who);
    if (overlap(db_dev, nb, a_dev, na) || overlap(db_dev, nb, b_dev, nb) || overlap(db_dev, nb, dscores_dev, ns))
      return fail(h, "%s: db aliases an input", who);
    if (overlap(da_dev, na, db_dev, nb)) return fail(h, "%s: da aliases db", who);
    hipStream_t s = as_stream(stream);
    ScoreTrainArgs a = shape_args(B, D, N0, N1, a_dev, b_dev, n0_dev, n1_dev, scale);
    a.ds = dscores_dev; a.da = da_dev; a.db = db_dev;
    if (da_dev) RUN("score_da", launch_score_da(a, s));
    if (db_dev) RUN("score_db", launch_score_db(a, s));
    return 0;
  });
}

}  // extern "C"
