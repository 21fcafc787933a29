// imx_host.h -- internal header of the host units of libimx.so (imx_api.cpp, imx_options.cpp, imx_weights.cpp, imx_superpoint.cpp,
// imx_superglue.cpp, imx_trainpairs.cpp), of libimx_train.so (imx_sptrain.cpp, imx_spgrad.cpp, imx_otgrad.cpp, imx_mhagrad.cpp,
// imx_lingrad.cpp, imx_bngrad.cpp), of libimx_sgtrain.so (imx_scoregrad.cpp), of libimx_spnet.so (imx_conv3grad.cpp), of
// libimx_spnorm.so (imx_bn2dgrad.cpp), of libimx_sppool.so (imx_poolgrad.cpp), of libimx_photo.so (imx_photo.cpp), of libimx_sploop.so (imx_sploop.cpp) and of libimx_sgloop.so (imx_sgloop.cpp), which work on the
// handles libimx.so makes: the handle,
// its weight sets and workspaces, the launch helpers, the weights-derived guards of the fp16-plane forms, and the stage functions
// libimx.so's entry points call.  Nothing here is exported (hidden visibility; imx.map).
#pragma once
#include "../../include/imx.h"
#include "imx_kernels.h"
#include "gnn_tail_pack.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <exception>
#include <map>
#include <new>
#include <string>
#include <vector>

namespace imx::host {

constexpr int HEADS = 4;          // AttentionalPropagation(feature_dim, 4), superglue_test.py:126

struct HostTensor {
  std::vector<float> data;
  std::vector<int64_t> shape;
};
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
};
struct ConvW {
  float* w = nullptr;    // direct form  [9][Cin][Cout] (conv3x3.hip: IMX_CONV=direct, and the fallback for shapes wino24 rejects)
  float* wu24 = nullptr; // Winograd F(2x4,3x3) form (conv1ab_wino24.hip / conv3x3_wino24.hip layout)
  float u_spread = 1.f;  // wino24h_pack: max |U| / median over output channels of their max |U| (the fp16-plane guard)
  void* wuh = nullptr;   // the same as two fp16 planes scaled by a power of two (conv3x3_wino24h.hip; wino24_pack.h: wino24h_pack), cin % 64 == 0 only
  float su_inv = 0.f;    // 1 / that power of two
  float* b = nullptr;
  int cin = 0, cout = 0;
};
struct GemmW {
  float* w = nullptr;
  float* wx3 = nullptr;   // the same weights as three bf16 terms per value in MFMA fragment order (split_bf16x3; gemm_x3.hip)
  float* wf = nullptr;    // the same fp32 weights in the B-fragment order of gnn_small.hip (fragment_order; K % 16 == 0 only)
  float* wh2 = nullptr;   // the same weights as two fp16 planes of w s in MFMA fragment order (split_f16x2; gemm_h2.hip), 1 / s, and how far
  float wh2_inv = 0.f;    // the largest |w| sits above the median over output columns of their largest |w| (the guard of the fp16 form:
  float wh2_spread = 0.f; // beyond kLinearSpreadMax the typical column loses bits of its low plane and the chain stays on gemm_x3)
  float* b = nullptr;
  int K = 0, N = 0, Npad = 0;
};
struct GnnLayer {
  GemmW qkv, merge, mlp1, mlp2;
  float* tail_stream = nullptr;    // gnn_tail_pack() of (mlp.0', mlp.3, the NEXT layer's q|k|v or final_proj): gnn_tail.hip (FmtX3), d = 128 only
  void* tail_stream_h2 = nullptr;  // gnn_tail_pack_h2() of the same three matrices (two fp16 planes): gnn_tail.hip (FmtH2)
  GnnTailH2Consts h2c{};           // reciprocal weight scales and column L1 norms
  float bmax_1 = 0.f, bmax_2 = 0.f;   // largest |bias| of mlp.0' and mlp.3
  float qkv_spread = 1.f;          // over q | k | v: (largest column L2 norm) / (median column L2 norm) of that projection -- how far its strongest output
                                   // channel sits above the typical one.  The two-plane attention scales a whole (side, pair) by its ACTUAL maximum: beyond
                                   // kAttnSpreadMax the typical channel would lose its low plane and the layer's attention runs on three bf16 planes
};
struct Tap {
  const void* p;
  std::vector<int64_t> shape;      // what imx_debug_fetch returns (NHWC for activations)
  bool blocked = false;            // the device buffer is channel-blocked (B, C/8, H, W, 8): un-blocked on the host at fetch time
};
struct TimedEvent {
  std::string name;
  const char* form;      // what the launcher reported through imx::last_form (static strings), or nullptr
  hipEvent_t e0, e1;
};
struct TimingRow {
  std::string name, form;
  int64_t launches;
  double ms;
};

inline std::string g_create_error;

}  // namespace imx::host

using namespace imx;
using namespace imx::host;

struct imx_handle_s {
  int device = 0;
  imx_config_t cfg{};
  std::string err;
  std::map<std::string, std::vector<int64_t>> expected[2];
  std::map<std::string, HostTensor> raw[2];
  bool finalized[2] = {false, false};
  std::vector<void*> weight_allocs[2];   // per net: freed when that net's weights are finalized again
  int upload_net = 0;                    // net whose finalize is running (upload() files allocations under it)
  // SuperPoint
  float *w1 = nullptr, *b1 = nullptr;
  // the dense NMS map behind the "nms" tap when the detector ran the candidate-bit form: computed on demand by imx_debug_fetch
  struct { const float* smap = nullptr; float* nms = nullptr; void* scratch = nullptr; int B = 0, H = 0, W = 0, radius = 0; bool pending = false; } nms_lazy;
  float c1a_l1 = 0.f, c1a_bmax = 0.f, c1a_spread = 1.f;   // (c1a_spread: max over median of conv1a's output-channel maxima, the fp16-plane guard)
  ConvW conv[8];   // conv1b, 2a, 2b, 3a, 3b, 4a, 4b, heads (convPa | convDa)
  GemmW pb, db;
  // SuperGlue
  float *kenc0_w = nullptr, *kenc0_b = nullptr;
  int kenc_c1 = 0;
  std::vector<GemmW> kenc;
  std::vector<GnnLayer> layers;
  GemmW final_proj;
  float bin_score = 1.f;
  // workspace
  std::map<std::string, DevBuf> bufs;
  // what the last SuperGlue forward left in the workspace, for imx_match_loss: valid only once the entry point has put the counts
  // somewhere that outlives the call (sg_keep_counts); withdrawn wherever one of these buffers is freed or overwritten
  struct { bool valid = false; int B = 0, N0 = 0, N1 = 0, N0p = 0, N1p = 0; const float *S = nullptr, *u = nullptr, *v = nullptr;
           const int32_t *n0 = nullptr, *n1 = nullptr; float alpha = 1.f; } sg_last;
  // state of the last detect
  int det_B = 0, det_H = 0, det_W = 0, det_Hc = 0, det_Wc = 0, det_Ksel = 0;
  // kernel-form options (imx_set_option; the environment only seeds them at imx_create)
  Options opt;
  std::string opt_text;      // backing store of imx_get_option's return value
  // debug / timing
  bool debug = false, timing = false;
  int poison = -1;           // "debug_poison": the byte ws() fills a (re)allocated workspace with, -1 = off
  std::map<std::string, Tap> taps;
  std::vector<TimedEvent> events;
  std::vector<TimingRow> report;
};

namespace imx::host {

inline int fail(imx_handle_t h, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (h) h->err = buf; else g_create_error = buf;
  return -1;
}

#define HIP_OK(h, expr)                                                                      \
  do {                                                                                       \
    hipError_t e__ = (expr);                                                                 \
    if (e__ != hipSuccess) return fail(h, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
  } while (0)

// "debug_poison" (imx_set_option; tests/test_gpu_history.py): which workspaces the hook may fill with a byte pattern.  The hook
// writes VALUES into memory the library owns; it must never turn into a wild address or a wait that does not end.
//   poisoned      every float workspace (sp.*, sg.*, tap.*, mp.desc*, knn.*, ransac.scratch, kp.cand_score, kp.sel_score): their
//                 consumers read them as numbers only; and sg.amax / sp.amax (integer bit patterns of maxima): the forward zeroes
//                 the whole table with hipMemsetAsync before the first kernel that reads or atomicMax-es it, on every call.
//   never         sg.sk_merge_cnt (workgroup tickets a merging workgroup WAITS on), sg.sk_trace, sg.idx0 / sg.idx1 (column indices
//                 that launch_matches turns into match indices), kp.row_count / row_off / cand_count / cand_idx / sel_count /
//                 sel_idx / sort_slots (counts and pixel indices: loop bounds and gather addresses of the keypoint and describe
//                 kernels), sp.nms_scratch / op.nms_scratch (candidate bit rows), mp.counts (per-pair counts: loop bounds of every
//                 SuperGlue kernel).  Their consumers were not all read through for a bounds check, so they stay as they are.
inline bool poisonable(const std::string& name) {
  for (const char* no : {"sg.sk_merge_cnt", "sg.sk_trace", "sg.idx0", "sg.idx1", "kp.row_count", "kp.row_off", "kp.cand_count", "kp.cand_idx",
                         "kp.sel_count", "kp.sel_idx", "kp.sort_slots", "sp.nms_scratch", "op.nms_scratch", "mp.counts"})
    if (name == no) return false;
  return true;
}

inline bool inside(const void* p, const DevBuf& b) {
  return b.p && p >= b.p && static_cast<const char*>(p) < static_cast<const char*>(b.p) + b.bytes;
}

inline float* ws(imx_handle_t h, const std::string& name, size_t bytes) {
  DevBuf& b = h->bufs[name];
  if (b.bytes >= bytes && b.p) return static_cast<float*>(b.p);
  if (b.p) {
    // nothing may keep a pointer into the buffer that goes away: the debug taps into it (the next forward registers them again) and
    // the lazily materialised "nms" tap, whose inputs it may be
    for (auto it = h->taps.begin(); it != h->taps.end();) it = inside(it->second.p, b) ? h->taps.erase(it) : std::next(it);
    if (inside(h->nms_lazy.smap, b) || inside(h->nms_lazy.nms, b) || inside(h->nms_lazy.scratch, b)) h->nms_lazy.pending = false;
    // ... and what imx_match_loss would read of the last SuperGlue forward
    if (inside(h->sg_last.S, b) || inside(h->sg_last.u, b) || inside(h->sg_last.v, b) || inside(h->sg_last.n0, b) || inside(h->sg_last.n1, b)) h->sg_last.valid = false;
    (void)hipDeviceSynchronize();
    (void)hipFree(b.p);
    b.p = nullptr;
    b.bytes = 0;
  }
  size_t want = bytes + bytes / 8 + 256;
  if (hipMalloc(&b.p, want) != hipSuccess) {
    b.p = nullptr;
    h->err = "hipMalloc failed for workspace '" + name + "' (" + std::to_string(want) + " bytes)";
    return nullptr;
  }
  b.bytes = want;
  if (h->poison >= 0 && poisonable(name) && (hipMemset(b.p, h->poison, want) != hipSuccess || hipDeviceSynchronize() != hipSuccess)) {
    h->err = "debug_poison: hipMemset failed for workspace '" + name + "'";
    return nullptr;
  }
  return static_cast<float*>(b.p);
}
#define WS(var, type, name, bytes)                         \
  type* var = reinterpret_cast<type*>(ws(h, name, bytes)); \
  if (!var) return -1;

template <class F>
int run(imx_handle_t h, const char* name, hipStream_t s, F&& f) {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (h->timing) {
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return fail(h, "hipEventCreate failed");
    (void)hipEventRecord(e0, s);
  }
  last_form = nullptr;
  hipError_t e = f();
  if (h->timing) {
    (void)hipEventRecord(e1, s);
    h->events.push_back({name, last_form, e0, e1});
  }
  if (e != hipSuccess) return fail(h, "kernel '%s' launch failed: %s", name, hipGetErrorString(e));
  return 0;
}
#define RUN(name, expr)                                              \
  do {                                                               \
    if (run(h, name, s, [&]() -> hipError_t { return (expr); })) return -1; \
  } while (0)

inline void tap(imx_handle_t h, const char* name, const void* p, std::vector<int64_t> shape, bool blocked = false) {
  h->taps[name] = Tap{p, std::move(shape), blocked};
}

// Nothing may throw across the C ABI (include/imx.h): every entry point runs inside this guard.  The handle owns
// std::string / std::map / std::vector state, so std::bad_alloc (or any other exception) is possible in principle;
// it becomes an error code + imx_last_error text.  Recording the text must not throw either.
inline int fail_nothrow(imx_handle_t h, const char* where, const char* what) noexcept {
  try {
    return fail(h, "%s: exception: %s", where, what);
  } catch (...) {
    return -1;
  }
}
template <class F>
int guarded(imx_handle_t h, const char* where, F&& f) noexcept {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    return fail_nothrow(h, where, "out of host memory (std::bad_alloc)");
  } catch (const std::exception& e) {
    return fail_nothrow(h, where, e.what());
  } catch (...) {
    return fail_nothrow(h, where, "unknown C++ exception");
  }
}

// an entry point that works on the handle's device: guarded(), a null handle is an error, the device is made current
template <class F>
int on_device(imx_handle_t h, const char* where, F&& f) noexcept {
  return guarded(h, where, [&]() -> int {
    if (!h) return -1;
    HIP_OK(h, hipSetDevice(h->device));
    return f();
  });
}

inline hipStream_t as_stream(void* s) { return static_cast<hipStream_t>(s); }
inline int pad32(int n) { return ((n + 31) / 32) * 32; }

// the guards of the fp16-plane forms: see wino24_pack.h (spread) and gnn_tail_pack.h (loose_h / loose_x)
constexpr float kConvSpreadMax = 16384.f, kTailLooseMax = 65536.f;
// (a q / k / v channel 2^12 above the median, times an activation crest factor of 2^4, puts the typical value 2^16 below the maximum)
constexpr float kAttnSpreadMax = 4096.f;
constexpr float kLinearSpreadMax = 4096.f;       // the guard of gemm_h2's and gnn_tail_h2's weight planes (one power of two per matrix: beyond 2^12 the typical
                                                 // column's weights keep fewer than the scheme's 22 bits -- tests/test_gpu_heavy.py: a q / k channel at 2^14 used 0.8 of the tolerance)
inline bool gemm_h2_weights_ok(const GemmW& W) { return W.wh2 && W.wh2_inv > 0.f && W.wh2_spread <= kLinearSpreadMax && W.K % 32 == 0 && W.Npad % 64 == 0; }

// Each weights-derived guard is decided here, once: the planners (plan_superpoint, plan_superglue) and the "arith_guard" text of
// imx_get_option (imx_options.cpp) call the same functions.
// conv chain: how far the typical output channel of the worst 3x3 layer (conv1a's plain weights included) sits below its layer's one scale
inline float conv_chain_spread(const imx_handle_s* h) {
  float sp = h->c1a_spread;
  for (int i = 0; i < 8; ++i) sp = std::max(sp, h->conv[i].u_spread);
  return sp;
}
inline bool conv_spread_ok(float spread) { return spread <= kConvSpreadMax; }
inline bool conv_chain_h_ok(const imx_handle_s* h) {
  for (int i = 0; i < 8; ++i)
    if (!h->conv[i].wuh) return false;
  return conv_spread_ok(conv_chain_spread(h));
}
// layer tail: the bounds that scale gnn_tail_h2's operands are tight enough for both fp16 planes
inline bool tail_h2_safe(const GnnLayer& L) { return L.h2c.loose_h <= kTailLooseMax && L.h2c.loose_x <= kTailLooseMax && L.h2c.w_spread <= kLinearSpreadMax; }
// linear chain: every matrix gemm_h2 would run passes the spread guard
inline bool linear_chain_h2_ok(const imx_handle_s* h) {
  bool ok = gemm_h2_weights_ok(h->final_proj);
  for (const GnnLayer& L : h->layers) ok = ok && gemm_h2_weights_ok(L.qkv) && gemm_h2_weights_ok(L.mlp1) && gemm_h2_weights_ok(L.mlp2);
  return ok;
}
// attention: the layer's q | k | v channels are close enough for one scale per (side, pair)
inline bool attn_f16x2_ok(const GnnLayer& L) { return L.qkv_spread <= kAttnSpreadMax; }

// ----------------------------------------------------------------------------- the stage functions
// imx_weights.cpp
void build_expected(imx_handle_t h);
int finalize_superpoint(imx_handle_t h);
int finalize_superglue(imx_handle_t h);

// imx_superpoint.cpp
int sp_detect(imx_handle_t h, const float* img0, const float* img1, int split, int B, int H, int W, int32_t* counts_out,
              hipStream_t s, bool dense_only = false, int32_t* counts_lo = nullptr, int32_t* counts_hi = nullptr, bool det_only = false);
int sp_describe(imx_handle_t h, int b0, int B, int Kcap, float* kpts, float* scores, float* desc, hipStream_t s,
                int split = -1, float* kpts2 = nullptr, float* scores2 = nullptr, float* desc2 = nullptr);

// imx_superglue.cpp
struct SgSide {
  const float* kpts; const float* scores; const float* desc;
  int64_t sb, sc, sn;
  const int32_t* n; int N, H, W;
};
int sg_forward(imx_handle_t h, int B, const SgSide sd[2], int64_t* m0, int64_t* m1, float* ms0, float* ms1, hipStream_t s);
// A linear layer / 1x1 convolution: gemm() launches the form it is told.  gemm_args() fills the operand fields of GemmArgs over `opt`,
// which carries the OPTIONAL ones (the GNN's linear layers: the (side, pair) row structure, the q|k|v maxima the epilogue should
// write, gemm_h2's scale sources and the word its epilogue leaves).  gemm_form() is the small / x3 / tiled rule of a plain launch:
// plan_superglue and the overload without a form (kenc, convPb, convDb) ask it; only the planner picks H2 or X3Amax.
enum class GemmForm : unsigned char { Small, H2, X3, X3Amax, Tiled };
inline GemmArgs gemm_args(const GemmW& W, const float* a0, int lda0, int K0, const float* a1, int lda1, int K1, const float* res, int ldr,
                          float* out, int ldo, int M, bool relu, GemmArgs opt = GemmArgs{}) {
  opt.a0 = a0; opt.lda0 = lda0; opt.K0 = K0; opt.a1 = a1; opt.lda1 = lda1; opt.K1 = K1; opt.w = W.w; opt.bias = W.b; opt.res = res; opt.ldr = ldr;
  opt.out = out; opt.ldo = ldo; opt.M = M; opt.N = W.N; opt.Npad = W.Npad; opt.relu = relu ? 1 : 0;
  return opt;
}
GemmForm gemm_form(const Options& o, const GemmW& W, const GemmArgs& g);
int gemm(imx_handle_t h, hipStream_t s, const char* name, GemmForm form, const GemmW& W, GemmArgs g);
inline int gemm(imx_handle_t h, hipStream_t s, const char* name, const GemmW& W, const GemmArgs& g) { return gemm(h, s, name, gemm_form(h->opt, W, g), W, g); }

// imx_trainpairs.cpp
// after sg_forward, by the entry point that called it: keeps the per-pair counts of that forward where imx_match_loss can read them later
// (the caller's count tensors are borrowed for the call only) and marks the forward's score matrix and potentials as readable
int sg_keep_counts(imx_handle_t h, int B, const int32_t* n0, const int32_t* n1, hipStream_t s);

// imx_options.cpp
int apply_option(imx_handle_t h, const std::string& key, const std::string& v);   // 0, or -1 for an unknown key / value
const char* get_option(imx_handle_t h, const char* key);                           // the canonical spelling; "" for an unknown key
std::string option_listing();                                                      // "key = value|value, ..." of every key, for error messages
int seed_options_from_env(imx_handle_t h);                                         // at imx_create (h's errors go to the create error text)

}  // namespace imx::host
