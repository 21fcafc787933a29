// imx_poolgrad.cpp -- the host unit of libimx_sppool.so (include/imx_sppool.h), on the handle libimx.so made: nn.MaxPool2d(2) and the
// descriptor normalisation desc / ||desc||_2 of SuperPoint's training step, forward and backward.  The kernels are sppool_train.hip's;
// nothing of the other five libraries is linked here, and no call draws on the handle's workspace.
#include "imx_host.h"
#include "sppool_train.h"
#include "../../include/imx_sppool.h"

#include <cstdint>

namespace {

int check_pool_shape(imx_handle_t h, const char* who, int B, int C, int H, int W) {
  if (B < 1 || B > 65535 || C < 1 || C > 1024 || H < 2 || H > 4096 || W < 2 || W > 4096)
    return fail(h, "%s: bad shape B=%d C=%d H=%d W=%d (B in [1,65535], C in [1,1024], H and W in [2,4096])", who, B, C, H, W);
  return 0;
}
int check_l2_shape(imx_handle_t h, const char* who, int B, int C, int HW) {
  if (B < 1 || C < 1 || C > 1024 || HW < 1 || HW > (1 << 24) || (long long)B * HW > INT32_MAX)
    return fail(h, "%s: bad shape B=%d C=%d HW=%d (B >= 1, C in [1,1024], HW in [1,2^24], B HW <= 2^31 - 1)", who, B, C, HW);
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

int imx_maxpool2_forward_train(imx_handle_t h, int B, int C, int H, int W, const float* x_dev, float* y_dev, uint8_t* idx_dev, void* stream) {
  return on_device(h, "imx_maxpool2_forward_train", [&]() -> int {
    const char* who = "imx_maxpool2_forward_train";
    if (check_pool_shape(h, who, B, C, H, W)) return -1;
    if (!x_dev || !y_dev) return fail(h, "%s: null argument", who);
    const size_t planes = (size_t)B * C, outs_n = planes * (size_t)(H / 2) * (size_t)(W / 2);
    const Range ins[1] = {{x_dev, planes * H * W * sizeof(float), "x"}};
    const Range outs[2] = {{y_dev, outs_n * sizeof(float), "y"}, {idx_dev, outs_n, "idx"}};
    if (check_alias(h, who, outs, 2, ins, 1)) return -1;
    hipStream_t s = as_stream(stream);
    PoolArgs a{};
    a.x = x_dev; a.y = y_dev; a.idx = idx_dev; a.B = B; a.C = C; a.H = H; a.W = W;
    RUN("maxpool2_fwd", (last_form = form_of(pool_x4(W, x_dev, y_dev, idx_dev)), launch_maxpool2_fwd(a, s)));
    return 0;
  });
}

int imx_maxpool2_backward(imx_handle_t h, int B, int C, int H, int W, const uint8_t* idx_dev, const float* dy_dev, float* dx_dev, void* stream) {
  return on_device(h, "imx_maxpool2_backward", [&]() -> int {
    const char* who = "imx_maxpool2_backward";
    if (check_pool_shape(h, who, B, C, H, W)) return -1;
    if (!idx_dev || !dy_dev || !dx_dev) return fail(h, "%s: null argument", who);
    const size_t planes = (size_t)B * C, outs_n = planes * (size_t)(H / 2) * (size_t)(W / 2);
    const Range ins[2] = {{idx_dev, outs_n, "idx"}, {dy_dev, outs_n * sizeof(float), "dy"}};
    const Range outs[1] = {{dx_dev, planes * H * W * sizeof(float), "dx"}};
    if (check_alias(h, who, outs, 1, ins, 2)) return -1;
    hipStream_t s = as_stream(stream);
    PoolArgs a{};
    a.idx_in = idx_dev; a.dy = dy_dev; a.dx = dx_dev; a.B = B; a.C = C; a.H = H; a.W = W;
    RUN("maxpool2_bwd", (last_form = form_of(pool_x4(W, dx_dev, dy_dev, idx_dev)), launch_maxpool2_bwd(a, s)));
    return 0;
  });
}

int imx_l2norm_forward_train(imx_handle_t h, int B, int C, int HW, const float* x_dev, float* y_dev, float* norm_dev, void* stream) {
  return on_device(h, "imx_l2norm_forward_train", [&]() -> int {
    const char* who = "imx_l2norm_forward_train";
    if (check_l2_shape(h, who, B, C, HW)) return -1;
    if (!x_dev || !y_dev || !norm_dev) return fail(h, "%s: null argument", who);
    const size_t full = (size_t)B * C * HW * sizeof(float), pix = (size_t)B * HW * sizeof(float);
    const Range ins[1] = {{x_dev, full, "x"}};
    const Range outs[2] = {{y_dev, full, "y"}, {norm_dev, pix, "norm"}};
    if (check_alias(h, who, outs, 2, ins, 1)) return -1;
    hipStream_t s = as_stream(stream);
    L2Args a{};
    a.x = x_dev; a.y = y_dev; a.norm = norm_dev; a.B = B; a.C = C; a.HW = HW;
    RUN("l2norm_fwd", (last_form = form_of(l2_x4(B, HW, x_dev, y_dev, norm_dev)), launch_l2norm_fwd(a, s)));
    return 0;
  });
}

int imx_l2norm_backward(imx_handle_t h, int B, int C, int HW, const float* y_dev, const float* norm_dev, const float* dy_dev, float* dx_dev,
                        void* stream) {
  return on_device(h, "imx_l2norm_backward", [&]() -> int {
    const char* who = "imx_l2norm_backward";
    if (check_l2_shape(h, who, B, C, HW)) return -1;
    if (!y_dev || !norm_dev || !dy_dev || !dx_dev) return fail(h, "%s: null argument", who);
    const size_t full = (size_t)B * C * HW * sizeof(float), pix = (size_t)B * HW * sizeof(float);
    const Range ins[3] = {{y_dev, full, "y"}, {norm_dev, pix, "norm"}, {dy_dev, full, "dy"}};
    const Range outs[1] = {{dx_dev, full, "dx"}};
    if (check_alias(h, who, outs, 1, ins, 3)) return -1;
    hipStream_t s = as_stream(stream);
    L2Args a{};
    a.y_in = y_dev; a.norm_in = norm_dev; a.dy = dy_dev; a.dx = dx_dev; a.B = B; a.C = C; a.HW = HW;
    RUN("l2norm_bwd", (last_form = form_of(l2_x4(B, HW, y_dev, norm_dev, dy_dev, dx_dev)), launch_l2norm_bwd(a, s)));
    return 0;
  });
}

}  // extern "C"
