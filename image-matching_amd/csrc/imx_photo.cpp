// imx_photo.cpp -- the host unit of libimx_photo.so (include/imx_photo.h), on the handle libimx.so made: the photometric augmentation of
// SuperPoint's training data.  The kernels are photo_aug.hip's; nothing of the other six libraries is linked here.  imx_photo_shade draws
// on the handle's workspace ("photo.mask", "photo.rows"); imx_photo_pixels on nothing.
#include "imx_host.h"
#include "photo_aug.h"
#include "../../include/imx_photo.h"

#include <cstdint>

namespace {

int check_shape(imx_handle_t h, const char* who, int B, int H, int W) {
  if (B < 1 || B > 65535 || H < 2 || H > 4096 || W < 2 || W > 4096)
    return fail(h, "%s: bad shape B=%d H=%d W=%d (B in [1,65535], H and W in [2,4096])", who, B, H, W);
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
// the output against every input; 0 or the error code with the text set
int check_alias(imx_handle_t h, const char* who, const Range& out, const Range* ins, int n_in) {
  for (int j = 0; j < n_in; ++j)
    if (overlap(out, ins[j])) return fail(h, "%s: %s aliases %s", who, out.name, ins[j].name);
  return 0;
}

}  // namespace

extern "C" {

int imx_photo_pixels(imx_handle_t h, int B, int H, int W, const float* img_dev, const uint8_t* lut_dev, const float* noise_scale_dev,
                     const uint32_t* thresh_dev, const uint8_t* table_dev, const float* blur_kernel_dev, const int32_t* blur_on_dev,
                     const uint32_t* key_dev, uint8_t* out_dev, void* stream) {
  return on_device(h, "imx_photo_pixels", [&]() -> int {
    const char* who = "imx_photo_pixels";
    if (check_shape(h, who, B, H, W)) return -1;
    if (!img_dev || !lut_dev || !noise_scale_dev || !thresh_dev || !table_dev || !blur_kernel_dev || !blur_on_dev || !key_dev || !out_dev)
      return fail(h, "%s: null argument", who);
    const size_t n = (size_t)B * H * W;
    const Range ins[8] = {{img_dev, n * sizeof(float), "img"}, {lut_dev, (size_t)B * 256, "lut"}, {noise_scale_dev, (size_t)B * 4, "noise_scale"},
                          {thresh_dev, (size_t)B * 4, "thresh"}, {table_dev, 256, "table"}, {blur_kernel_dev, (size_t)B * 36, "blur_kernel"},
                          {blur_on_dev, (size_t)B * 4, "blur_on"}, {key_dev, (size_t)B * 8, "key"}};
    if (check_alias(h, who, Range{out_dev, n, "out"}, ins, 8)) return -1;
    hipStream_t s = as_stream(stream);
    PixelArgs a{};
    a.img = img_dev; a.lut = lut_dev; a.noise_scale = noise_scale_dev; a.thresh = thresh_dev; a.table = table_dev; a.blur_k = blur_kernel_dev;
    a.blur_on = blur_on_dev; a.key = key_dev; a.out = out_dev; a.B = B; a.H = H; a.W = W;
    RUN("photo_pixels", (last_form = pixels_x4(W, img_dev, out_dev) ? "x4" : "x1", launch_photo_pixels(a, s)));
    return 0;
  });
}

int imx_photo_shade(imx_handle_t h, int B, int H, int W, int E, int Kcap, const uint8_t* img_dev, const float* ellipses_dev,
                    const int32_t* n_ellipses_dev, const float* taps_dev, const int32_t* ksize_host, const float* transparency_dev,
                    const int32_t* on_dev, float* out_dev, void* stream) {
  return on_device(h, "imx_photo_shade", [&]() -> int {
    const char* who = "imx_photo_shade";
    if (check_shape(h, who, B, H, W)) return -1;
    if (E < 1 || E > kShadeMaxE || Kcap < 3 || Kcap > kShadeMaxK)
      return fail(h, "%s: bad capacity E=%d Kcap=%d (E in [1,%d], Kcap in [3,%d])", who, E, Kcap, kShadeMaxE, kShadeMaxK);
    if (!img_dev || !ellipses_dev || !n_ellipses_dev || !taps_dev || !ksize_host || !transparency_dev || !on_dev || !out_dev)
      return fail(h, "%s: null argument", who);
    for (int b = 0; b < B; ++b)
      if (ksize_host[b] < 3 || ksize_host[b] > Kcap || ksize_host[b] % 2 == 0)
        return fail(h, "%s: ksize[%d]=%d (odd, in [3,%d], at most Kcap=%d)", who, b, ksize_host[b], kShadeMaxK, Kcap);
    const size_t n = (size_t)B * H * W;
    const Range ins[6] = {{img_dev, n, "img"}, {ellipses_dev, (size_t)B * E * 20, "ellipses"}, {n_ellipses_dev, (size_t)B * 4, "n_ellipses"},
                          {taps_dev, (size_t)B * Kcap * 4, "taps"}, {transparency_dev, (size_t)B * 4, "transparency"}, {on_dev, (size_t)B * 4, "on"}};
    if (check_alias(h, who, Range{out_dev, n * sizeof(float), "out"}, ins, 6)) return -1;
    hipStream_t s = as_stream(stream);
    WS(mask, uint8_t, "photo.mask", n);
    WS(rows, float, "photo.rows", n * sizeof(float));
    ShadeArgs a{};
    a.img = img_dev; a.ell = ellipses_dev; a.n_ell = n_ellipses_dev; a.taps = taps_dev; a.transparency = transparency_dev; a.on = on_dev;
    a.mask = mask; a.tmp = rows; a.out = out_dev; a.B = B; a.H = H; a.W = W; a.E = E; a.Kcap = Kcap;
    RUN("shade_mask", launch_shade_mask(a, s));
    for (int b0 = 0; b0 < B; b0 += kShadeChunk) {
      const int nb = std::min(kShadeChunk, B - b0);
      a.b0 = b0;
      for (int i = 0; i < kShadeChunk; ++i) a.ks[i] = (uint16_t)(i < nb ? ksize_host[b0 + i] : 3);
      RUN("shade_rows", launch_shade_rows(a, nb, s));
      RUN("shade_cols", launch_shade_cols(a, nb, s));
    }
    return 0;
  });
}

}  // extern "C"
