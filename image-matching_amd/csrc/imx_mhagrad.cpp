// imx_mhagrad.cpp -- a host unit of libimx_train.so (include/imx_train.h), on the handle libimx.so made: the attention of
// SuperGlue's GNN in its training form, a forward that keeps the row log-sum-exp and the backward from it.  The kernels are
// mha_train.hip's; attention.hip and the inference path are not linked here and not touched.  The one scratch buffer ("mha.delta",
// B H N floats) is written in full by the backward call that reads it.
#include "imx_host.h"
#include "mha_train.h"
#include "../../include/imx_train.h"

#include <cmath>

namespace {

// the shape rules of both entry points; 0 or the error code with the text set
int check_shape(imx_handle_t h, const char* who, int B, int H, int D, int N, int M) {
  if (B < 1 || H < 1 || (long long)B * H > 65535 || N < 1 || M < 1 || N > (1 << 20) || M > (1 << 20))
    return fail(h, "%s: bad shape B=%d H=%d N=%d M=%d (B, H >= 1, B H <= 65535, N M in [1,2^20])", who, B, H, N, M);
  if (!mha_head_dim_ok(D)) return fail(h, "%s: head dimension %d is not built (16, 32 or 64)", who, D);
  return 0;
}

MhaArgs shape_args(int B, int H, int D, int N, int M, const float* q, const float* k, const float* v, const int32_t* nq, const int32_t* nk) {
  MhaArgs a{};
  a.q = q; a.k = k; a.v = v; a.nq = nq; a.nk = nk; a.B = B; a.H = H; a.D = D; a.N = N; a.M = M;
  a.scale = 1.f / std::sqrt((float)D);
  return a;
}

}  // namespace

extern "C" {

int imx_mha_forward_train(imx_handle_t h, int B, int H, int D, int N, int M, const float* q_dev, const float* k_dev, const float* v_dev,
                          const int32_t* nq_dev, const int32_t* nk_dev, float* out_dev, float* lse_dev, void* stream) {
  return on_device(h, "imx_mha_forward_train", [&]() -> int {
    if (check_shape(h, "imx_mha_forward_train", B, H, D, N, M)) return -1;
    if (!q_dev || !k_dev || !v_dev || !out_dev) return fail(h, "imx_mha_forward_train: null argument");
    hipStream_t s = as_stream(stream);
    MhaArgs a = shape_args(B, H, D, N, M, q_dev, k_dev, v_dev, nq_dev, nk_dev);
    a.out = out_dev; a.lse = lse_dev;
    RUN("mha_fwd", launch_mha_fwd(a, s));
    return 0;
  });
}

int imx_mha_backward(imx_handle_t h, int B, int H, int D, int N, int M, const float* q_dev, const float* k_dev, const float* v_dev,
                     const float* out_dev, const float* lse_dev, const float* dout_dev, const int32_t* nq_dev, const int32_t* nk_dev,
                     float* dq_dev, float* dk_dev, float* dv_dev, void* stream) {
  return on_device(h, "imx_mha_backward", [&]() -> int {
    if (check_shape(h, "imx_mha_backward", B, H, D, N, M)) return -1;
    if (!q_dev || !k_dev || !v_dev || !out_dev || !lse_dev || !dout_dev) return fail(h, "imx_mha_backward: null argument");
    if (!dq_dev && !dk_dev && !dv_dev) return 0;
    hipStream_t s = as_stream(stream);
    MhaArgs a = shape_args(B, H, D, N, M, q_dev, k_dev, v_dev, nq_dev, nk_dev);
    a.o_in = out_dev; a.lse_in = lse_dev; a.dout = dout_dev; a.dq = dq_dev; a.dk = dk_dev; a.dv = dv_dev;
    WS(delta, float, "mha.delta", (size_t)B * H * N * sizeof(float));
    a.delta = delta;
    RUN("mha_delta", launch_mha_delta(a, s));
    if (dk_dev || dv_dev) RUN("mha_dkdv", launch_mha_dkdv(a, s));
    if (dq_dev) RUN("mha_dq", launch_mha_dq(a, s));
    return 0;
  });
}

}  // extern "C"
