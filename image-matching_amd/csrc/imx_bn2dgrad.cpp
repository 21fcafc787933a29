// imx_bn2dgrad.cpp -- the host unit of libimx_spnorm.so (include/imx_spnorm.h), on the handle libimx.so made: nn.BatchNorm2d, optionally
// followed by nn.ReLU, in its training form on NCHW maps, forward and backward.  The kernels are bn2d_train.hip's; nothing of the other
// four libraries is linked here.  The one scratch buffer ("bn2d.part", 2 B C ceil(HW / 4096) floats) is written by the call that reads it.
#include "imx_host.h"
#include "bn2d_train.h"
#include "../../include/imx_spnorm.h"

#include <cstdint>

namespace {

// the shape rules of both entry points; 0 or the error code with the text set
int check_shape(imx_handle_t h, const char* who, int B, int C, int HW) {
  if (B < 1 || B > 65535 || C < 1 || C > 1024 || HW < 1 || HW > (1 << 24) || (long long)B * HW > INT32_MAX)
    return fail(h, "%s: bad shape B=%d C=%d HW=%d (B in [1,65535], C in [1,1024], HW in [1,2^24], B HW <= 2^31 - 1)", who, B, C, HW);
  return 0;
}

struct Range {
  const void* p;
  size_t bytes;
  const char* name;
};
// the byte ranges share an address
bool overlap(const Range& a, const Range& b) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a.p), pb = reinterpret_cast<uintptr_t>(b.p);
  return a.p && b.p && pa < pb + b.bytes && pb < pa + a.bytes;
}
// every output against every input and every other output; 0 or the error code with the text set
int check_alias(imx_handle_t h, const char* who, const Range* outs, int n_out, const Range* ins, int n_in) {
  for (int i = 0; i < n_out; ++i) {
    for (int j = 0; j < n_in; ++j)
      if (overlap(outs[i], ins[j])) return fail(h, "%s: %s aliases %s", who, outs[i].name, ins[j].name);
    for (int j = i + 1; j < n_out; ++j)
      if (overlap(outs[i], outs[j])) return fail(h, "%s: %s aliases %s", who, outs[i].name, outs[j].name);
  }
  return 0;
}

const char* form_of(bool x4) { return x4 ? "x4" : "x1"; }

}  // namespace

extern "C" {

int imx_bn2d_forward_train(imx_handle_t h, int B, int C, int HW, int relu, int use_batch_stats, float eps, float momentum, const float* x_dev,
                           const float* gamma_dev, const float* beta_dev, float* running_mean_dev, float* running_var_dev,
                           int64_t* num_batches_tracked_dev, float* y_dev, float* mean_dev, float* rstd_dev, void* stream) {
  return on_device(h, "imx_bn2d_forward_train", [&]() -> int {
    const char* who = "imx_bn2d_forward_train";
    if (check_shape(h, who, B, C, HW)) return -1;
    if (!(eps > 0.f) || !(momentum >= 0.f && momentum <= 1.f)) return fail(h, "%s: bad eps=%g or momentum=%g (eps > 0, 0 <= momentum <= 1)", who, eps, momentum);
    if (!x_dev || !gamma_dev || !beta_dev || !y_dev || !mean_dev || !rstd_dev) return fail(h, "%s: null argument", who);
    if (!use_batch_stats && (!running_mean_dev || !running_var_dev)) return fail(h, "%s: the running statistics are required with use_batch_stats = 0", who);
    if (use_batch_stats && (long long)B * HW == 1) return fail(h, "%s: one value per channel in training mode (B HW = 1)", who);
    const size_t full = (size_t)B * C * HW * sizeof(float), chan = (size_t)C * sizeof(float);
    const Range ins[3] = {{x_dev, full, "x"}, {gamma_dev, chan, "gamma"}, {beta_dev, chan, "beta"}};
    const Range outs[6] = {{y_dev, full, "y"}, {mean_dev, chan, "mean"}, {rstd_dev, chan, "rstd"}, {running_mean_dev, chan, "running_mean"},
                           {running_var_dev, chan, "running_var"}, {num_batches_tracked_dev, sizeof(int64_t), "num_batches_tracked"}};
    if (check_alias(h, who, outs, 6, ins, 3)) return -1;
    hipStream_t s = as_stream(stream);
    Bn2dArgs a{};
    a.x = x_dev; a.gamma = gamma_dev; a.beta = beta_dev; a.B = B; a.C = C; a.HW = HW; a.relu = relu ? 1 : 0; a.train = use_batch_stats ? 1 : 0;
    a.eps = eps; a.momentum = momentum; a.running_mean = running_mean_dev; a.running_var = running_var_dev;
    a.num_batches_tracked = reinterpret_cast<long long*>(num_batches_tracked_dev);
    a.y = y_dev; a.mean = mean_dev; a.rstd = rstd_dev;
    if (a.train) {
      WS(part, float, "bn2d.part", bn2d_part_floats(B, C, HW) * sizeof(float));
      a.part = part;
      RUN("bn2d_stats", (last_form = form_of(bn2d_x4(HW, x_dev)), launch_bn2d_stats(a, s)));
      RUN("bn2d_finalize", launch_bn2d_finalize(a, s));
    }
    RUN("bn2d_apply", (last_form = form_of(bn2d_x4(HW, x_dev, y_dev)), launch_bn2d_apply(a, s)));
    return 0;
  });
}

int imx_bn2d_backward(imx_handle_t h, int B, int C, int HW, int relu, int use_batch_stats, const float* x_dev, const float* gamma_dev,
                      const float* beta_dev, const float* mean_dev, const float* rstd_dev, const float* dy_dev, float* dx_dev,
                      float* dgamma_dev, float* dbeta_dev, void* stream) {
  return on_device(h, "imx_bn2d_backward", [&]() -> int {
    const char* who = "imx_bn2d_backward";
    if (check_shape(h, who, B, C, HW)) return -1;
    if (!x_dev || !gamma_dev || !beta_dev || !mean_dev || !rstd_dev || !dy_dev) return fail(h, "%s: null argument", who);
    if (use_batch_stats && (long long)B * HW == 1) return fail(h, "%s: one value per channel in training mode (B HW = 1)", who);
    const size_t full = (size_t)B * C * HW * sizeof(float), chan = (size_t)C * sizeof(float);
    const Range ins[6] = {{x_dev, full, "x"}, {gamma_dev, chan, "gamma"}, {beta_dev, chan, "beta"}, {mean_dev, chan, "mean"},
                          {rstd_dev, chan, "rstd"}, {dy_dev, full, "dy"}};
    const Range outs[3] = {{dx_dev, full, "dx"}, {dgamma_dev, chan, "dgamma"}, {dbeta_dev, chan, "dbeta"}};
    if (check_alias(h, who, outs, 3, ins, 6)) return -1;
    if (!dx_dev && !dgamma_dev && !dbeta_dev) return 0;        // nothing wanted: nothing launched
    hipStream_t s = as_stream(stream);
    Bn2dArgs a{};
    a.x = x_dev; a.gamma = gamma_dev; a.beta = beta_dev; a.dy = dy_dev; a.B = B; a.C = C; a.HW = HW; a.relu = relu ? 1 : 0;
    a.train = use_batch_stats ? 1 : 0; a.mean_in = mean_dev; a.rstd_in = rstd_dev; a.dx = dx_dev; a.dgamma = dgamma_dev; a.dbeta = dbeta_dev;
    // the sums: for dgamma and dbeta, and in training mode for dx too (then they stay in the scratch)
    if (dgamma_dev || dbeta_dev || a.train) {
      WS(part, float, "bn2d.part", bn2d_part_floats(B, C, HW) * sizeof(float));
      a.part = part;
      RUN("bn2d_bwd_sums", (last_form = form_of(bn2d_x4(HW, x_dev, dy_dev)), launch_bn2d_bwd_sums(a, s)));
      RUN("bn2d_bwd_finalize", launch_bn2d_bwd_finalize(a, s));
    }
    if (dx_dev) RUN("bn2d_bwd_dx", (last_form = form_of(bn2d_x4(HW, x_dev, dy_dev, dx_dev)), launch_bn2d_bwd_dx(a, s)));
    return 0;
  });
}

}  // extern "C"
