// imx_bngrad.cpp -- a host unit of libimx_train.so (include/imx_train.h), on the handle libimx.so made: nn.BatchNorm1d followed by
// nn.ReLU in their training form, forward and backward.  The kernels are bn_train.hip's, one launch per call; no workspace is drawn.
#include "imx_host.h"
#include "bn_train.h"
#include "../../include/imx_train.h"

namespace {

// the shape rules of both entry points; 0 or the error code with the text set
int check_shape(imx_handle_t h, const char* who, int B, int C, int N) {
  if (B < 1 || B > 65535 || C < 1 || C > 1024 || N < 1 || N > (1 << 20))
    return fail(h, "%s: bad shape B=%d C=%d N=%d (B in [1,65535], C in [1,1024], N in [1,2^20])", who, B, C, N);
  return 0;
}

const char* form_of(int B, int N) { return bn_in_registers(B, N) ? "regs" : "reread"; }

}  // namespace

extern "C" {

int imx_bn_relu_forward_train(imx_handle_t h, int B, int C, int N, int use_batch_stats, float eps, float momentum, const float* x_dev,
                              const float* gamma_dev, const float* beta_dev, const int32_t* n_dev, float* running_mean_dev,
                              float* running_var_dev, int64_t* num_batches_tracked_dev, float* y_dev, float* mean_dev, float* rstd_dev,
                              void* stream) {
  return on_device(h, "imx_bn_relu_forward_train", [&]() -> int {
    const char* who = "imx_bn_relu_forward_train";
    if (check_shape(h, who, B, C, N)) return -1;
    if (!(eps > 0.f) || !(momentum >= 0.f && momentum <= 1.f)) return fail(h, "%s: bad eps=%g or momentum=%g (eps > 0, 0 <= momentum <= 1)", who, eps, momentum);
    if (!x_dev || !gamma_dev || !beta_dev || !y_dev || !mean_dev || !rstd_dev) return fail(h, "%s: null argument", who);
    if (!use_batch_stats && (!running_mean_dev || !running_var_dev)) return fail(h, "%s: the running statistics are required with use_batch_stats = 0", who);
    if (use_batch_stats && !n_dev && (long long)B * N == 1) return fail(h, "%s: one value per channel in training mode (B N = 1)", who);
    if (y_dev == x_dev) return fail(h, "%s: y aliases x", who);
    hipStream_t s = as_stream(stream);
    BnArgs a{};
    a.x = x_dev; a.gamma = gamma_dev; a.beta = beta_dev; a.n = n_dev; a.B = B; a.C = C; a.N = N; a.train = use_batch_stats ? 1 : 0;
    a.eps = eps; a.momentum = momentum; a.running_mean = running_mean_dev; a.running_var = running_var_dev;
    a.num_batches_tracked = reinterpret_cast<long long*>(num_batches_tracked_dev);
    a.y = y_dev; a.mean = mean_dev; a.rstd = rstd_dev;
    RUN("bn_relu_fwd", (last_form = form_of(B, N), launch_bn_relu_fwd(a, s)));
    return 0;
  });
}

int imx_bn_relu_backward(imx_handle_t h, int B, int C, int N, int use_batch_stats, const float* x_dev, const float* gamma_dev,
                         const float* beta_dev, const float* mean_dev, const float* rstd_dev, const float* dy_dev, const int32_t* n_dev,
                         float* dx_dev, float* dgamma_dev, float* dbeta_dev, void* stream) {
  return on_device(h, "imx_bn_relu_backward", [&]() -> int {
    const char* who = "imx_bn_relu_backward";
    if (check_shape(h, who, B, C, N)) return -1;
    if (!x_dev || !gamma_dev || !beta_dev || !mean_dev || !rstd_dev || !dy_dev) return fail(h, "%s: null argument", who);
    if (dx_dev && (dx_dev == x_dev || dx_dev == dy_dev)) return fail(h, "%s: dx aliases an input", who);
    if (!dx_dev && !dgamma_dev && !dbeta_dev) return 0;        // nothing wanted: nothing launched
    hipStream_t s = as_stream(stream);
    BnArgs a{};
    a.x = x_dev; a.gamma = gamma_dev; a.beta = beta_dev; a.dy = dy_dev; a.n = n_dev; a.B = B; a.C = C; a.N = N; a.train = use_batch_stats ? 1 : 0;
    a.mean_in = mean_dev; a.rstd_in = rstd_dev; a.dx = dx_dev; a.dgamma = dgamma_dev; a.dbeta = dbeta_dev;
    RUN("bn_relu_bwd", (last_form = form_of(B, N), launch_bn_relu_bwd(a, s)));
    return 0;
  });
}

}  // extern "C"
