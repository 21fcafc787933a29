// imx_sploop.cpp -- the host unit of libimx_sploop.so (include/imx_sploop.h), on the handle libimx.so made: the bilinear label splat of
// SuperPoint's gaussian_label and the flat Adam step.  The kernels are sploop.hip's; nothing of the other seven libraries is linked here.
// imx_warp_labels_bi draws on the handle's workspace ("spl.owner", written in full by every call); imx_adam_flat on nothing.
#include "imx_host.h"
#include "sploop.h"
#include "../../include/imx_sploop.h"

#include <cmath>
#include <cstdint>

namespace {

// the byte ranges [a, a + n) and [b, b + n) share an address
bool overlap(const void* a, const void* b, size_t bytes) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + bytes && pb < pa + bytes;
}

}  // namespace

extern "C" {

int imx_warp_labels_bi(imx_handle_t h, const float* pts_dev, const int32_t* counts_dev, int B, int Kcap, const float* mats_dev, int H, int W,
                       int levels, float* out_dev, int32_t* flag_dev, void* stream) {
  return on_device(h, "imx_warp_labels_bi", [&]() -> int {
    const char* who = "imx_warp_labels_bi";
    if (B < 1 || B > 65535 || Kcap < 0 || Kcap >= (1 << 29) || H < 1 || W < 1 || (int64_t)B * H * W > (1ll << 31))
      return fail(h, "%s: bad shape B=%d Kcap=%d H=%d W=%d (B in [1,65535], Kcap < 2^29, B H W <= 2^31)", who, B, Kcap, H, W);
    if (levels != 0 && levels != 255) return fail(h, "%s: levels must be 0 (the raw weight) or 255 (8-bit quantisation), got %d", who, levels);
    if (!out_dev || !mats_dev || (Kcap && !pts_dev)) return fail(h, "%s: null argument", who);
    hipStream_t s = as_stream(stream);
    WS(owner, int32_t, "spl.owner", (size_t)B * H * W * sizeof(int32_t));
    LabelsBiArgs a{};
    a.pts = pts_dev; a.counts = counts_dev; a.mats = mats_dev; a.out = out_dev; a.owner = owner; a.flag = flag_dev;
    a.B = B; a.Kcap = Kcap; a.H = H; a.W = W; a.levels = levels;
    RUN("warp_labels_bi", launch_labels_bi(a, s));
    return 0;
  });
}

int imx_adam_flat(imx_handle_t h, float* p_dev, float* g_dev, float* m_dev, float* v_dev, int64_t n, double step_size, double beta1, double beta2,
                  double inv_sqrt_bc2, double eps, double weight_decay, int zero_grad, void* stream) {
  return on_device(h, "imx_adam_flat", [&]() -> int {
    const char* who = "imx_adam_flat";
    if (n < 0 || n > (1ll << 38)) return fail(h, "%s: n=%lld outside [0, 2^38]", who, (long long)n);
    if (!std::isfinite(step_size) || !std::isfinite(inv_sqrt_bc2) || !(beta1 >= 0. && beta1 < 1.) || !(beta2 >= 0. && beta2 < 1.) ||
        !(eps >= 0.) || !std::isfinite(eps) || !std::isfinite(weight_decay))
      return fail(h, "%s: bad scalar (step_size %g, beta1 %g, beta2 %g, inv_sqrt_bc2 %g, eps %g, weight_decay %g)", who, step_size, beta1, beta2,
                  inv_sqrt_bc2, eps, weight_decay);
    if (n == 0) return 0;
    if (!p_dev || !g_dev || !m_dev || !v_dev) return fail(h, "%s: null argument", who);
    float* ptr[4] = {p_dev, g_dev, m_dev, v_dev};
    const char* name[4] = {"p", "g", "m", "v"};
    for (int i = 0; i < 4; ++i) {
      if (reinterpret_cast<uintptr_t>(ptr[i]) & 3) return fail(h, "%s: %s is not 4-byte aligned", who, name[i]);
      for (int j = i + 1; j < 4; ++j)
        if (overlap(ptr[i], ptr[j], (size_t)n * sizeof(float))) return fail(h, "%s: %s aliases %s", who, name[i], name[j]);
    }
    hipStream_t s = as_stream(stream);
    AdamArgs a{};
    a.p = p_dev; a.g = g_dev; a.m = m_dev; a.v = v_dev; a.n = n;
    // each scalar is rounded to float32 once, here
    a.step_size = (float)step_size; a.beta1 = (float)beta1; a.c1 = (float)(1.0 - beta1); a.beta2 = (float)beta2; a.c2 = (float)(1.0 - beta2);
    a.inv_sqrt_bc2 = (float)inv_sqrt_bc2; a.eps = (float)eps; a.weight_decay = (float)weight_decay; a.zero_grad = zero_grad ? 1 : 0;
    RUN("adam_flat", (last_form = adam_x4(a) ? "x4" : "x1", launch_adam_flat(a, s)));
    return 0;
  });
}

}  // extern "C"
