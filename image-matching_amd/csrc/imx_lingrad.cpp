// imx_lingrad.cpp -- a host unit of libimx_train.so (include/imx_train.h), on the handle libimx.so made: nn.Conv1d(kernel_size=1)
// on torch.cat([x0, x1], 1) in its training form, forward and the gradients at the inputs, the weight and the bias.  The kernels are
// lin_train.hip's; gemm*.hip, gnn_tail.hip and the inference path are not linked here and not touched.  The one scratch buffer
// ("lin.part", B ceil(N / 256) Cout (C0 + C1 + 1) floats) is written by the backward call that reads it.
#include "imx_host.h"
#include "lin_train.h"
#include "../../include/imx_train.h"

namespace {

// the shape rules of both entry points; 0 or the error code with the text set
int check_shape(imx_handle_t h, const char* who, int B, int Cout, int C0, int C1, int N, const float* x1) {
  if (B < 1 || B > 65535 || Cout < 1 || Cout > 1024 || C0 < 1 || C1 < 0 || (long long)C0 + C1 > 1024 || N < 1 || N > (1 << 20))
    return fail(h, "%s: bad shape B=%d Cout=%d C0=%d C1=%d N=%d (B in [1,65535], Cout in [1,1024], C0 >= 1, C1 >= 0, C0 + C1 <= 1024, N in [1,2^20])",
                who, B, Cout, C0, C1, N);
  if (C1 == 0 && x1) return fail(h, "%s: x1 given with C1 = 0", who);
  if (C1 > 0 && !x1) return fail(h, "%s: x1 is null with C1 = %d", who, C1);
  return 0;
}

LinArgs shape_args(int B, int Cout, int C0, int C1, int N, const float* x0, const float* x1, const float* w, const int32_t* n) {
  LinArgs a{};
  a.x0 = x0; a.x1 = x1; a.w = w; a.n = n; a.B = B; a.Cout = Cout; a.C0 = C0; a.C1 = C1; a.N = N;
  return a;
}

}  // namespace

extern "C" {

int imx_conv1x1_forward_train(imx_handle_t h, int B, int Cout, int C0, int C1, int N, const float* x0_dev, const float* x1_dev,
                              const float* w_dev, const float* bias_dev, const int32_t* n_dev, float* y_dev, void* stream) {
  return on_device(h, "imx_conv1x1_forward_train", [&]() -> int {
    if (check_shape(h, "imx_conv1x1_forward_train", B, Cout, C0, C1, N, x1_dev)) return -1;
    if (!x0_dev || !w_dev || !y_dev) return fail(h, "imx_conv1x1_forward_train: null argument");
    hipStream_t s = as_stream(stream);
    LinArgs a = shape_args(B, Cout, C0, C1, N, x0_dev, x1_dev, w_dev, n_dev);
    a.bias = bias_dev; a.y = y_dev;
    RUN("lin_fwd", launch_lin_fwd(a, s));
    return 0;
  });
}

int imx_conv1x1_backward(imx_handle_t h, int B, int Cout, int C0, int C1, int N, const float* x0_dev, const float* x1_dev,
                         const float* w_dev, const float* dy_dev, const int32_t* n_dev, float* dx0_dev, float* dx1_dev, float* dw_dev,
                         float* db_dev, void* stream) {
  return on_device(h, "imx_conv1x1_backward", [&]() -> int {
    if (check_shape(h, "imx_conv1x1_backward", B, Cout, C0, C1, N, x1_dev)) return -1;
    if (!x0_dev || !w_dev || !dy_dev) return fail(h, "imx_conv1x1_backward: null argument");
    if (C1 == 0 && dx1_dev) return fail(h, "imx_conv1x1_backward: dx1 given with C1 = 0");
    hipStream_t s = as_stream(stream);
    LinArgs a = shape_args(B, Cout, C0, C1, N, x0_dev, x1_dev, w_dev, n_dev);
    a.dy = dy_dev; a.dx0 = dx0_dev; a.dx1 = dx1_dev; a.dw = dw_dev; a.db = db_dev;
    if (dx0_dev || dx1_dev) RUN("lin_dx", launch_lin_dx(a, s));
    if (dw_dev || db_dev) {
      WS(part, float, "lin.part", lin_part_floats(B, Cout, C0 + C1, N) * sizeof(float));
      a.part = part;
      RUN("lin_dw", launch_lin_dw(a, s));
      RUN("lin_dw_reduce", launch_lin_dw_reduce(a, s));
    }
    return 0;
  });
}

}  // extern "C"
