// imx_conv3grad.cpp -- the host unit of libimx_spnet.so (include/imx_spnet.h), on the handle libimx.so made: nn.Conv2d(Cin, Cout, 3,
// padding=1) in its training form, forward and the gradients at the input, the weight and the bias.  The kernels are conv3_train.hip's;
// nothing of the other three libraries is linked here and the inference convolutions are not touched.  The one scratch buffer
// ("conv3.part", B ceil(H / 16) Cout (9 Cin + 1) floats) is written by the backward call that reads it.
#include "imx_host.h"
#include "conv3_train.h"
#include "../../include/imx_spnet.h"

#include <cstdint>

namespace {

// the shape rules of both entry points; 0 or the error code with the text set
int check_shape(imx_handle_t h, const char* who, int B, int Cout, int Cin, int H, int W) {
  if (B < 1 || B > 65535 || Cout < 1 || Cout > 1024 || Cin < 1 || Cin > 1024 || H < 1 || H > 4096 || W < 1 || W > 4096)
    return fail(h, "%s: bad shape B=%d Cout=%d Cin=%d H=%d W=%d (B in [1,65535], Cout and Cin in [1,1024], H and W in [1,4096])", who, B, Cout,
                Cin, H, W);
  const long long grid = conv3_max_grid(B, Cout, Cin, H, W);
  if (grid > INT32_MAX) return fail(h, "%s: B=%d Cout=%d Cin=%d H=%d W=%d needs %lld workgroups, more than a grid of 2^31 - 1", who, B, Cout, Cin, H, W, grid);
  return 0;
}

// the byte ranges [p, p + floats) and [q, q + floats) share an address
bool overlap(const float* p, size_t np, const float* q, size_t nq) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return p && q && a < b + nq * sizeof(float) && b < a + np * sizeof(float);
}

Conv3Args shape_args(int B, int Cout, int Cin, int H, int W, const float* x, const float* w) {
  Conv3Args a{};
  a.x = x; a.w = w; a.B = B; a.Cout = Cout; a.Cin = Cin; a.H = H; a.W = W;
  return a;
}

}  // namespace

extern "C" {

int imx_conv3x3_forward_train(imx_handle_t h, int B, int Cout, int Cin, int H, int W, const float* x_dev, const float* w_dev,
                              const float* bias_dev, float* y_dev, void* stream) {
  return on_device(h, "imx_conv3x3_forward_train", [&]() -> int {
    const char* who = "imx_conv3x3_forward_train";
    if (check_shape(h, who, B, Cout, Cin, H, W)) return -1;
    if (!x_dev || !w_dev || !y_dev) return fail(h, "%s: null argument", who);
    const size_t nx = (size_t)B * Cin * H * W, ny = (size_t)B * Cout * H * W, nw = (size_t)Cout * Cin * 9;
    if (overlap(y_dev, ny, x_dev, nx) || overlap(y_dev, ny, w_dev, nw) || overlap(y_dev, ny, bias_dev, Cout)) return fail(h, "%s: y aliases an input", who);
    hipStream_t s = as_stream(stream);
    Conv3Args a = shape_args(B, Cout, Cin, H, W, x_dev, w_dev);
    a.bias = bias_dev; a.y = y_dev;
    RUN("conv3_fwd", launch_conv3_fwd(a, s));
    return 0;
  });
}

int imx_conv3x3_backward(imx_handle_t h, int B, int Cout, int Cin, int H, int W, const float* x_dev, const float* w_dev,
                         const float* dy_dev, float* dx_dev, float* dw_dev, float* db_dev, void* stream) {
  return on_device(h, "imx_conv3x3_backward", [&]() -> int {
    const char* who = "imx_conv3x3_backward";
    if (check_shape(h, who, B, Cout, Cin, H, W)) return -1;
    if (!x_dev || !w_dev || !dy_dev) return fail(h, "%s: null argument", who);
    const size_t nx = (size_t)B * Cin * H * W, ny = (size_t)B * Cout * H * W, nw = (size_t)Cout * Cin * 9;
    const struct { float* p; size_t n; const char* name; } outs[3] = {{dx_dev, nx, "dx"}, {dw_dev, nw, "dw"}, {db_dev, (size_t)Cout, "db"}};
    for (int i = 0; i < 3; ++i) {
      if (overlap(outs[i].p, outs[i].n, x_dev, nx) || overlap(outs[i].p, outs[i].n, w_dev, nw) || overlap(outs[i].p, outs[i].n, dy_dev, ny))
        return fail(h, "%s: %s aliases an input", who, outs[i].name);
      for (int j = i + 1; j < 3; ++j)
        if (overlap(outs[i].p, outs[i].n, outs[j].p, outs[j].n)) return fail(h, "%s: %s aliases %s", who, outs[i].name, outs[j].name);
    }
    hipStream_t s = as_stream(stream);
    Conv3Args a = shape_args(B, Cout, Cin, H, W, x_dev, w_dev);
    a.dy = dy_dev; a.dx = dx_dev; a.dw = dw_dev; a.db = db_dev;
    if (dx_dev) RUN("conv3_dx", launch_conv3_dx(a, s));
    if (dw_dev || db_dev) {
      WS(part, float, "conv3.part", conv3_part_floats(B, Cout, Cin, H, W) * sizeof(float));
      a.part = part;
      RUN("conv3_dw", launch_conv3_dw(a, s));
      RUN("conv3_dw_reduce", launch_conv3_dw_reduce(a, s));
    }
    return 0;
  });
}

}  // extern "C"
