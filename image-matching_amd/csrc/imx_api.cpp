// imx_api.cpp -- C ABI of libimx.so (include/imx.h): the entry points, each a guard around argument checks and the stage functions of
// imx_host.h (weights: imx_weights.cpp; launch sequences: imx_superpoint.cpp, imx_superglue.cpp; options: imx_options.cpp; the training-pair
// entry points live in imx_trainpairs.cpp), plus the
// RCCL loader, the debug-tap fetch and the timing report.  All arithmetic of the path runs in the kernels declared in imx_kernels.h.
#include "imx_host.h"

#include <dlfcn.h>

#include <atomic>
#include <memory>

namespace {
bool ends_with(const std::string& s, const std::string& suf) {
  return s.size() >= suf.size() && s.compare(s.size() - suf.size(), suf.size(), suf) == 0;
}
}  // namespace

// =============================================================================== C ABI
extern "C" {

#ifndef IMX_BUILD_ID
#define IMX_BUILD_ID "dev"
#endif
const char* imx_version(void) { return "imx 0.4 gfx950 hip-7.2 fp32 build " IMX_BUILD_ID; }

int imx_create(int device_id, const imx_config_t* cfg, imx_handle_t* out) {
  return guarded(nullptr, "imx_create", [&]() -> int {
    if (!cfg || !out) return fail(nullptr, "imx_create: null argument");
    if (cfg->num_gnn_layers < 0 || cfg->num_gnn_layers > IMX_MAX_GNN_LAYERS) return fail(nullptr, "imx_create: bad num_gnn_layers %d", cfg->num_gnn_layers);
    if (cfg->kenc_n < 1 || cfg->kenc_n > IMX_MAX_KENC) return fail(nullptr, "imx_create: bad keypoint_encoder length %d", cfg->kenc_n);
    // SuperPoint alone takes any descriptor_dim that keeps rows float4-aligned; SuperGlue's own limits (4 heads of 16/32/64
    // dims) are checked when ITS weights are finalized
    if (cfg->descriptor_dim <= 0 || cfg->descriptor_dim % 4 || cfg->descriptor_dim > 512) return fail(nullptr, "imx_create: descriptor_dim must be a multiple of 4 in [4,512] (got %d)", cfg->descriptor_dim);
    if (cfg->nms_radius < 0) return fail(nullptr, "imx_create: nms_radius must be >= 0 (got %d)", cfg->nms_radius);
    // the top-k stage rounds max_keypoints up to a power of two in 32-bit arithmetic (sp_tail.hip: launch_keypoints)
    if (cfg->max_keypoints > (1 << 30)) return fail(nullptr, "imx_create: max_keypoints must be <= 2^30 (got %d); use -1 for 'all'", cfg->max_keypoints);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, "imx_create: no HIP device available (this library has no CPU path)");
    if (device_id < 0 || device_id >= ndev) return fail(nullptr, "imx_create: device %d out of range (%d devices)", device_id, ndev);
    if (hipSetDevice(device_id) != hipSuccess) return fail(nullptr, "imx_create: hipSetDevice(%d) failed", device_id);
    std::unique_ptr<imx_handle_s> h(new imx_handle_s());      // released only once nothing below can throw
    h->device = device_id;
    h->cfg = *cfg;
    if (seed_options_from_env(h.get())) return -1;
    // switches of earlier rounds that no longer exist: say so once instead of silently measuring the default path
    static std::atomic<bool> warned{false};
    for (const char* old : {"IMX_GEMM", "IMX_GEMM_SMALL", "IMX_ATTN", "IMX_ATTN_SPLIT", "IMX_NMS", "IMX_CONV_BLOCKED", "IMX_WINO_EXP", "IMX_WINO_WGS",
                            "IMX_X3_WGS", "IMX_SINKHORN_WAVES", "IMX_CONV_SWZ", "IMX_QKV_AMAX", "IMX_SINKHORN_GROUP", "IMX_SINKHORN_PREFETCH", "IMX_SINKHORN_PREFETCH_NOW"})
      if (getenv(old) && !warned.exchange(true))
        fprintf(stderr, "libimx: the environment variable %s (and the other per-kernel switches of rounds 1-5) was removed; it is ignored. "
                        "Kernel forms are handle options now: imx_set_option(h, \"mfma\" | \"latency_forms\" | \"conv\", ...), seeded from IMX_MFMA / "
                        "IMX_LATENCY_FORMS / IMX_CONV at imx_create (an unknown VALUE of those three makes imx_create fail).\n", old);
    build_expected(h.get());
    *out = h.release();
    return 0;
  });
}

int imx_destroy(imx_handle_t h) {
  return guarded(h, "imx_destroy", [&]() -> int {
    if (!h) return 0;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    for (auto& va : h->weight_allocs) for (void* p : va) (void)hipFree(p);
    for (auto& kv : h->bufs) if (kv.second.p) (void)hipFree(kv.second.p);
    for (auto& e : h->events) { (void)hipEventDestroy(e.e0); (void)hipEventDestroy(e.e1); }
    delete h;
    return 0;
  });
}

const char* imx_last_error(imx_handle_t h) { return h ? h->err.c_str() : g_create_error.c_str(); }   // c_str() does not throw

int imx_load_weight(imx_handle_t h, int net, const char* name, const float* host, int ndim, const int64_t* shape) {
  return guarded(h, "imx_load_weight", [&]() -> int {
    if (!h) return -1;
    if (net != IMX_NET_SUPERPOINT && net != IMX_NET_SUPERGLUE) return fail(h, "imx_load_weight: bad net id %d", net);
    if (!name || !host) return fail(h, "imx_load_weight: null argument");
    std::string key = name;
    if (ends_with(key, "num_batches_tracked")) return 0;
    auto it = h->expected[net].find(key);
    if (it == h->expected[net].end()) return fail(h, "imx_load_weight: unexpected key '%s' for %s", name, net ? "SuperGlue" : "SuperPoint");
    int64_t want = 1, got = 1;
    for (int64_t v : it->second) want *= v;
    for (int i = 0; i < ndim; ++i) got *= shape[i];
    bool same = (size_t)ndim == it->second.size();
    for (int i = 0; same && i < ndim; ++i) same = shape[i] == it->second[i];
    if (!same && !(want == got && want == 1)) {
      std::string ws_, gs_;
      for (int64_t v : it->second) ws_ += std::to_string(v) + ",";
      for (int i = 0; i < ndim; ++i) gs_ += std::to_string(shape[i]) + ",";
      return fail(h, "imx_load_weight: size mismatch for %s: expected (%s) got (%s)", name, ws_.c_str(), gs_.c_str());
    }
    HostTensor t;
    t.data.assign(host, host + got);
    t.shape.assign(shape, shape + ndim);
    h->raw[net][key] = std::move(t);
    h->finalized[net] = false;
    return 0;
  });
}

int imx_finalize_weights(imx_handle_t h, int net) {
  return guarded(h, "imx_finalize_weights", [&]() -> int {
    if (!h) return -1;
    if (net != IMX_NET_SUPERPOINT && net != IMX_NET_SUPERGLUE) return fail(h, "imx_finalize_weights: bad net id %d", net);
    HIP_OK(h, hipSetDevice(h->device));
    for (auto& kv : h->expected[net])
      if (!h->raw[net].count(kv.first)) return fail(h, "Missing key in state_dict: \"%s\"", kv.first.c_str());
    // a second load_state_dict (checkpoint sweeps): the previous uploads of THIS net are released first
    if (!h->weight_allocs[net].empty()) {
      HIP_OK(h, hipDeviceSynchronize());
      for (void* p : h->weight_allocs[net]) (void)hipFree(p);
      h->weight_allocs[net].clear();
    }
    h->finalized[net] = false;
    h->upload_net = net;
    int rc = net == IMX_NET_SUPERPOINT ? finalize_superpoint(h) : finalize_superglue(h);
    if (rc) return rc;
    h->finalized[net] = true;
    return 0;
  });
}

int imx_superpoint_detect(imx_handle_t h, const float* img_dev, int B, int H, int W, int32_t* counts_dev, void* stream) {
  return on_device(h, "imx_superpoint_detect", [&]() -> int {
    return sp_detect(h, img_dev, nullptr, B, B, H, W, counts_dev, as_stream(stream));
  });
}

int imx_superpoint_dense(imx_handle_t h, const float* img_dev, int B, int H, int W, float* semi_dev, float* desc_dev, void* stream) {
  return on_device(h, "imx_superpoint_dense", [&]() -> int {
    hipStream_t s = as_stream(stream);
    if (sp_detect(h, img_dev, nullptr, B, B, H, W, nullptr, s, true)) return -1;
    RUN("dense_export", launch_dense_export(static_cast<const float*>(h->bufs["sp.semi"].p), 65,
                                            static_cast<const float*>(h->bufs["sp.dense"].p), h->cfg.descriptor_dim, semi_dev,
                                            desc_dev, B, h->det_Hc, h->det_Wc, h->cfg.sp_variant == IMX_SP_VARIANT_OFFICIAL, s));
    return 0;
  });
}

int imx_superpoint_describe(imx_handle_t h, int B, int Kcap, float* kpts_dev, float* scores_dev, float* desc_dev, void* stream) {
  return on_device(h, "imx_superpoint_describe", [&]() -> int {
    if (Kcap <= 0) return 0;
    return sp_describe(h, 0, B, Kcap, kpts_dev, scores_dev, desc_dev, as_stream(stream));
  });
}

int imx_superglue_forward(imx_handle_t h, int B, const float* kpts0_dev, const float* scores0_dev, const float* desc0_dev,
                          int64_t desc0_stride_b, int64_t desc0_stride_c, int64_t desc0_stride_n, const int32_t* n0_dev,
                          int N0, int H0, int W0, const float* kpts1_dev, const float* scores1_dev, const float* desc1_dev,
                          int64_t desc1_stride_b, int64_t desc1_stride_c, int64_t desc1_stride_n, const int32_t* n1_dev,
                          int N1, int H1, int W1, int64_t* matches0_dev, int64_t* matches1_dev, float* mscores0_dev,
                          float* mscores1_dev, void* stream) {
  return on_device(h, "imx_superglue_forward", [&]() -> int {
    SgSide sd[2] = {{kpts0_dev, scores0_dev, desc0_dev, desc0_stride_b, desc0_stride_c, desc0_stride_n, n0_dev, N0, H0, W0},
                    {kpts1_dev, scores1_dev, desc1_dev, desc1_stride_b, desc1_stride_c, desc1_stride_n, n1_dev, N1, H1, W1}};
    if (sg_forward(h, B, sd, matches0_dev, matches1_dev, mscores0_dev, mscores1_dev, as_stream(stream))) return -1;
    return sg_keep_counts(h, B, n0_dev, n1_dev, as_stream(stream));
  });
}

int imx_match_pairs(imx_handle_t h, const float* img0_dev, const float* img1_dev, int B, int H, int W, float* kpts0_dev,
                    float* kpts1_dev, float* scores0_dev, float* scores1_dev, int32_t* counts0_dev, int32_t* counts1_dev,
                    float* desc0_dev, float* desc1_dev, int64_t* matches0_dev, int64_t* matches1_dev, float* mscores0_dev,
                    float* mscores1_dev, void* stream) {
  return on_device(h, "imx_match_pairs", [&]() -> int {
    hipStream_t s = as_stream(stream);
    const int K = h->cfg.max_keypoints, d = h->cfg.descriptor_dim;
    if (K <= 0) return fail(h, "imx_match_pairs needs max_keypoints > 0 (fixed-size outputs); got %d", K);
    WS(counts, int32_t, "mp.counts", (size_t)2 * B * 4);
    if (sp_detect(h, img0_dev, img1_dev, B, 2 * B, H, W, counts, s, false, counts0_dev, counts1_dev)) return -1;
    if (!desc0_dev) { WS(t0, float, "mp.desc0", (size_t)B * K * d * 4); desc0_dev = t0; }
    if (!desc1_dev) { WS(t1, float, "mp.desc1", (size_t)B * K * d * 4); desc1_dev = t1; }
    if (sp_describe(h, 0, 2 * B, K, kpts0_dev, scores0_dev, desc0_dev, s, B, kpts1_dev, scores1_dev, desc1_dev)) return -1;   // both sides, one launch
    SgSide sd[2] = {{kpts0_dev, scores0_dev, desc0_dev, (int64_t)K * d, 1, d, counts, K, H, W},
                    {kpts1_dev, scores1_dev, desc1_dev, (int64_t)K * d, 1, d, counts + B, K, H, W}};
    if (sg_forward(h, B, sd, matches0_dev, matches1_dev, mscores0_dev, mscores1_dev, s)) return -1;
    return sg_keep_counts(h, B, counts, counts + B, s);       // (mp.counts is the handle's own: nothing is copied)
  });
}

int imx_pack_records(imx_handle_t h, const int32_t* pair_ids_dev, int B, int K, const float* kpts0_dev, const float* kpts1_dev,
                     const int32_t* counts0_dev, const int32_t* counts1_dev, const int64_t* matches0_dev, const int64_t* matches1_dev,
                     const float* mscores0_dev, const float* mscores1_dev, int32_t* rec_dev, int rows, void* stream) {
  return on_device(h, "imx_pack_records", [&]() -> int {
    hipStream_t s = as_stream(stream);
    if (B < 0 || K <= 0 || rows < B) return fail(h, "imx_pack_records: bad shape B=%d K=%d rows=%d", B, K, rows);
    if (B > 0 && (!pair_ids_dev || !kpts0_dev || !kpts1_dev || !counts0_dev || !counts1_dev || !matches0_dev || !matches1_dev ||
                  !mscores0_dev || !mscores1_dev)) return fail(h, "imx_pack_records: null argument");
    if (!rec_dev) return fail(h, "imx_pack_records: null record buffer");
    PackArgs a{pair_ids_dev, kpts0_dev, kpts1_dev, counts0_dev, counts1_dev, reinterpret_cast<const long long*>(matches0_dev),
               reinterpret_cast<const long long*>(matches1_dev), mscores0_dev, mscores1_dev, rec_dev, B, K, rows};
    RUN("pack_records", launch_pack_records(a, s));
    return 0;
  });
}

// RCCL entry points, resolved at the first call from the RCCL already in the process (a torch process has its own copy loaded;
// a C host links one), else from librccl.so: libimx.so itself carries no link-time dependency on a particular RCCL build.
extern "C++" {
namespace {
struct Rccl {
  int (*CommCount)(void*, int*) = nullptr;
  int (*CommUserRank)(void*, int*) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  int (*Send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*Recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  bool ok = false;
};
const Rccl& rccl() {
  static Rccl r = [] {
    Rccl t;
    void* lib = nullptr;
    auto sym = [&](const char* name) -> void* {
      if (void* p = dlsym(RTLD_DEFAULT, name)) return p;
      if (!lib) {
        // the host names the RCCL build that created its communicators with IMX_RCCL_LIBRARY (a path) when that library is not
        // visible to dlsym(RTLD_DEFAULT) -- e.g. loaded RTLD_LOCAL under another soname; otherwise the usual names are tried
        if (const char* path = getenv("IMX_RCCL_LIBRARY")) lib = dlopen(path, RTLD_NOW | RTLD_GLOBAL);
        for (const char* so : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so"})
          if (!lib && (lib = dlopen(so, RTLD_NOW | RTLD_GLOBAL))) break;
      }
      return lib ? dlsym(lib, name) : nullptr;
    };
    t.CommCount = reinterpret_cast<decltype(t.CommCount)>(sym("ncclCommCount"));
    t.CommUserRank = reinterpret_cast<decltype(t.CommUserRank)>(sym("ncclCommUserRank"));
    t.GroupStart = reinterpret_cast<decltype(t.GroupStart)>(sym("ncclGroupStart"));
    t.GroupEnd = reinterpret_cast<decltype(t.GroupEnd)>(sym("ncclGroupEnd"));
    t.Send = reinterpret_cast<decltype(t.Send)>(sym("ncclSend"));
    t.Recv = reinterpret_cast<decltype(t.Recv)>(sym("ncclRecv"));
    t.GetErrorString = reinterpret_cast<decltype(t.GetErrorString)>(sym("ncclGetErrorString"));
    t.ok = t.CommCount && t.CommUserRank && t.GroupStart && t.GroupEnd && t.Send && t.Recv;
    return t;
  }();
  return r;
}
}  // namespace
}  // extern "C++"

int imx_gather_records(imx_handle_t h, const int32_t* rec_dev, int rows, int width, int32_t* out_dev, int dst, void* nccl_comm, void* stream) {
  return on_device(h, "imx_gather_records", [&]() -> int {
    if (!nccl_comm || !rec_dev || rows < 0 || width <= 0) return fail(h, "imx_gather_records: bad arguments");
    const Rccl& n = rccl();
    if (!n.ok) return fail(h, "imx_gather_records: no RCCL in this process and librccl.so could not be loaded");
    int world = 0, rank = 0, rc = 0;
    auto chk = [&](int e, const char* what) { if (e && !rc) { rc = e; fail(h, "imx_gather_records: %s failed: %s", what, n.GetErrorString ? n.GetErrorString(e) : "RCCL error"); } };
    chk(n.CommCount(nccl_comm, &world), "ncclCommCount");
    chk(n.CommUserRank(nccl_comm, &rank), "ncclCommUserRank");
    if (rc) return -1;
    if (dst < 0 || dst >= world) return fail(h, "imx_gather_records: destination rank %d outside the communicator (%d ranks)", dst, world);
    if (rank == dst && !out_dev) return fail(h, "imx_gather_records: the destination rank needs an output buffer");
    const size_t count = (size_t)rows * width;
    constexpr int kInt32 = 2;                       // ncclInt32
    hipStream_t s = as_stream(stream);
    // one group: every rank sends its rows to `dst`; `dst` posts one receive per rank into its slot (rank order = gather order)
    chk(n.GroupStart(), "ncclGroupStart");
    if (count) {
      chk(n.Send(rec_dev, count, kInt32, dst, nccl_comm, s), "ncclSend");
      if (rank == dst)
        for (int r = 0; r < world; ++r) chk(n.Recv(out_dev + (size_t)r * count, count, kInt32, r, nccl_comm, s), "ncclRecv");
    }
    chk(n.GroupEnd(), "ncclGroupEnd");
    return rc ? -1 : 0;
  });
}

int imx_op_nms(imx_handle_t h, const float* scores_dev, float* out_dev, int B, int H, int W, int radius, void* stream) {
  return on_device(h, "imx_op_nms", [&]() -> int {
    hipStream_t s = as_stream(stream);
    if (radius < 0) return fail(h, "imx_op_nms: radius must be >= 0 (got %d)", radius);
    WS(nms_scratch, unsigned, "op.nms_scratch", nms_scratch_bytes(B, H, W, radius));
    RUN("nms", launch_nms(scores_dev, out_dev, B, H, W, radius, s, nms_scratch));
    return 0;
  });
}

int imx_estimate_affine_partial(imx_handle_t h, const float* kpts0_dev, const float* kpts1_dev, const int64_t* matches0_dev,
                                const int32_t* counts0_dev, int B, int K, float ransac_threshold, int hypotheses, uint32_t seed,
                                float* M_dev, uint8_t* inlier_dev, int32_t* n_inliers_dev, void* stream) {
  return on_device(h, "imx_estimate_affine_partial", [&]() -> int {
    hipStream_t s = as_stream(stream);
    if (B <= 0 || K <= 0) return fail(h, "imx_estimate_affine_partial: bad shape B=%d K=%d", B, K);
    float* scratch = nullptr;
    if (K > 8192) {      // the compacted coordinates no longer fit LDS: they live in HBM (slower; nothing is refused)
      WS(rs, float, "ransac.scratch", (size_t)B * 4 * K * sizeof(float));
      scratch = rs;
    }
    RansacArgs a{kpts0_dev, kpts1_dev, reinterpret_cast<const long long*>(matches0_dev), counts0_dev, B, K, ransac_threshold,
                 hypotheses, seed, M_dev, inlier_dev, n_inliers_dev, scratch};
    RUN("ransac", launch_ransac(a, s));
    return 0;
  });
}

int imx_knn_ratio_match(imx_handle_t h, int B, const float* desc0_dev, int64_t s0b, int64_t s0c, int64_t s0n, const int32_t* n0_dev,
                        int N0, const float* desc1_dev, int64_t s1b, int64_t s1c, int64_t s1n, const int32_t* n1_dev, int N1,
                        float ratio, int64_t* matches_dev, float* dist1_dev, float* dist2_dev, void* stream) {
  return on_device(h, "imx_knn_ratio_match", [&]() -> int {
    hipStream_t s = as_stream(stream);
    const int d = h->cfg.descriptor_dim;
    if (B <= 0 || N0 <= 0 || N1 < 0) return fail(h, "imx_knn_ratio_match: bad shape B=%d N0=%d N1=%d", B, N0, N1);
    const int N0p = pad32(N0), N1p = pad32(std::max(N1, 1));
    const size_t f = sizeof(float);
    WS(r0, float, "knn.rows0", (size_t)B * N0p * d * f);
    WS(r1, float, "knn.rows1", (size_t)B * N1p * d * f);
    WS(nr0, float, "knn.norm0", (size_t)B * N0p * f);
    WS(nr1, float, "knn.norm1", (size_t)B * N1p * f);
    WS(dots, float, "knn.dots", (size_t)B * N0p * N1p * f);
    RUN("gather_desc", launch_gather_desc(desc0_dev, s0b, s0c, s0n, B, N0, N0p, d, n0_dev, r0, s));
    RUN("gather_desc", launch_gather_desc(desc1_dev, s1b, s1c, s1n, B, N1, N1p, d, n1_dev, r1, s));
    RUN("rownorm2", launch_rownorm2(r0, d, (long)B * N0p, nr0, s));
    RUN("rownorm2", launch_rownorm2(r1, d, (long)B * N1p, nr1, s));
    ScoreArgs sc{r0, r1, dots, B, N0p, N1p, d, 1.0f};
    RUN("knn_dots", launch_score_gemm(sc, s));
    KnnArgs k{dots, nr0, nr1, B, N0, N1, N0p, N1p, n0_dev, n1_dev, ratio, reinterpret_cast<long long*>(matches_dev), dist1_dev, dist2_dev};
    RUN("knn2", launch_knn2(k, s));
    return 0;
  });
}

int imx_ingest_resize_u8(imx_handle_t h, const uint8_t* src_dev, int B, int Hs, int Ws, int64_t src_stride_b, float* dst_dev, int H,
                         int W, void* stream) {
  return on_device(h, "imx_ingest_resize_u8", [&]() -> int {
    if (B <= 0 || Hs <= 0 || Ws <= 0 || H <= 0 || W <= 0) return fail(h, "imx_ingest_resize_u8: bad shape %dx%dx%d -> %dx%d", B, Hs, Ws, H, W);
    hipStream_t s = as_stream(stream);
    RUN("ingest_resize", launch_resize_u8_unit(src_dev, (long)src_stride_b, B, Hs, Ws, dst_dev, H, W, s));
    return 0;
  });
}

int imx_warp_affine_u8(imx_handle_t h, const uint8_t* src_dev, int Hs, int Ws, const double* M_host, uint8_t* dst_dev, int H, int W,
                       void* stream) {
  return on_device(h, "imx_warp_affine_u8", [&]() -> int {
    if (Hs <= 0 || Ws <= 0 || H <= 0 || W <= 0 || !M_host) return fail(h, "imx_warp_affine_u8: bad arguments");
    // cv2.warpAffine without WARP_INVERSE_MAP inverts the 2x3 matrix in double precision (imgwarp.cpp invertAffineTransform path)
    const double* M = M_host;
    double D = M[0] * M[4] - M[1] * M[3];
    D = D != 0.0 ? 1.0 / D : 0.0;
    const double A11 = M[4] * D, A22 = M[0] * D;
    double inv[6];
    inv[0] = A11; inv[1] = M[1] * (-D); inv[3] = M[3] * (-D); inv[4] = A22;
    inv[2] = -inv[0] * M[2] - inv[1] * M[5];
    inv[5] = -inv[3] * M[2] - inv[4] * M[5];
    hipStream_t s = as_stream(stream);
    RUN("warp_affine", launch_warp_affine_u8(src_dev, Hs, Ws, dst_dev, H, W, inv, s));
    return 0;
  });
}

int imx_warp_homography(imx_handle_t h, const float* src_dev, int src_shared, int N, int H, int W, const float* mats_dev, int nearest,
                        float* dst_dev, void* stream) {
  return on_device(h, "imx_warp_homography", [&]() -> int {
    if (N < 1 || N > 65535 || H < 2 || W < 2) return fail(h, "imx_warp_homography: bad shape N=%d H=%d W=%d (N in [1,65535], H, W >= 2)", N, H, W);
    if (!mats_dev || !dst_dev) return fail(h, "imx_warp_homography: null argument");
    hipStream_t s = as_stream(stream);
    RUN("ha_warp", launch_ha_warp(src_dev, src_shared ? 0 : (long)H * W, mats_dev, N, H, W, nearest != 0, dst_dev, nullptr, s));
    return 0;
  });
}

int imx_combine_heatmap(imx_handle_t h, const float* heat_dev, const float* mask_dev, const float* unwarp_dev, int N, int H, int W,
                        float* out_dev, float* count_dev, void* stream) {
  return on_device(h, "imx_combine_heatmap", [&]() -> int {
    if (N < 1 || H < 2 || W < 2) return fail(h, "imx_combine_heatmap: bad shape N=%d H=%d W=%d (N >= 1, H, W >= 2)", N, H, W);
    if (!heat_dev || !mask_dev || !unwarp_dev || !out_dev) return fail(h, "imx_combine_heatmap: null argument");
    hipStream_t s = as_stream(stream);
    RUN("ha_combine", launch_ha_combine(heat_dev, mask_dev, nullptr, unwarp_dev, N, H, W, out_dev, count_dev, s));
    return 0;
  });
}

int imx_superpoint_heatmap(imx_handle_t h, const float* img_dev, int B, int H, int W, float* heat_dev, void* stream) {
  return on_device(h, "imx_superpoint_heatmap", [&]() -> int {
    if (H < 8 || W < 8 || H % 8 || W % 8) return fail(h, "imx_superpoint_heatmap: H and W must be multiples of 8 (got %d x %d)", H, W);
    if (!img_dev || !heat_dev) return fail(h, "imx_superpoint_heatmap: null argument");
    hipStream_t s = as_stream(stream);
    if (sp_detect(h, img_dev, nullptr, B, B, H, W, nullptr, s, true, nullptr, nullptr, true)) return -1;
    RUN("ha_heat", launch_softmax_shuffle(static_cast<const float*>(h->bufs["sp.semi"].p), 65, heat_dev, B, H / 8, W / 8, s));
    return 0;
  });
}

int imx_homography_adapt(imx_handle_t h, const float* img_dev, int H, int W, int N, const float* warp_dev, const float* unwarp_dev,
                         float* heatmap_dev, float* count_dev, void* stream) {
  return on_device(h, "imx_homography_adapt", [&]() -> int {
    if (N < 1 || N > 65535) return fail(h, "imx_homography_adapt: N must be in [1,65535] (got %d)", N);
    if (H < 8 || W < 8 || H % 8 || W % 8) return fail(h, "imx_homography_adapt: H and W must be multiples of 8 (got %d x %d)", H, W);
    if (!img_dev || !warp_dev || !unwarp_dev || !heatmap_dev) return fail(h, "imx_homography_adapt: null argument");
    if (!h->finalized[IMX_NET_SUPERPOINT]) return fail(h, "SuperPoint weights not finalized");
    hipStream_t s = as_stream(stream);
    const size_t stack = (size_t)N * H * W * sizeof(float);
    WS(warped, float, "ha.warped", stack);
    // "ha_masks" = recompute: no mask stack (the combine evaluates the predicate itself) unless the debug tap wants it
    const bool stored = h->opt.ha_masks == 0 || h->debug;
    float* mask = nullptr;
    if (stored) {
      WS(mask_, float, "ha.mask", stack);
      mask = mask_;
    }
    WS(heat, float, "ha.heat", stack);
    // the N warps of the ONE image (the reference's repeat is never materialised) and their valid masks in one launch
    RUN("ha_warp", launch_ha_warp(img_dev, 0, warp_dev, N, H, W, 0, warped, mask, s));
    if (sp_detect(h, warped, nullptr, N, N, H, W, nullptr, s, true, nullptr, nullptr, true)) return -1;
    RUN("ha_heat", launch_softmax_shuffle(static_cast<const float*>(h->bufs["sp.semi"].p), 65, heat, N, H / 8, W / 8, s));
    RUN("ha_combine", launch_ha_combine(heat, h->opt.ha_masks == 0 ? mask : nullptr, warp_dev, unwarp_dev, N, H, W, heatmap_dev, count_dev, s));
    tap(h, "ha_warped", warped, {N, H, W});
    // (the only tap that is ever withdrawn: without a stored stack an "ha_mask" left by an earlier call would point at masks of OTHER
    // matrices, and imx_debug_fetch would hand them out as this call's)
    if (mask) tap(h, "ha_mask", mask, {N, H, W}); else h->taps.erase("ha_mask");
    tap(h, "ha_heat", heat, {N, H, W});
    return 0;
  });
}

int imx_heatmap_points(imx_handle_t h, const float* heatmap_dev, int H, int W, float conf_thresh, int nms_dist, int top_k, int subpixel,
                       float* pts_dev, int cap, int32_t* count_dev, void* stream) {
  return on_device(h, "imx_heatmap_points", [&]() -> int {
    if (H < 1 || W < 1 || (int64_t)H * W > (1 << 30)) return fail(h, "imx_heatmap_points: bad map shape %d x %d", H, W);
    if (nms_dist < 0) return fail(h, "imx_heatmap_points: nms_dist must be >= 0 (got %d)", nms_dist);
    if (cap < 0 || (cap > 0 && !pts_dev) || !heatmap_dev) return fail(h, "imx_heatmap_points: null argument or negative cap");
    hipStream_t s = as_stream(stream);
    WS(scratch, char, "hp.scratch", heatmap_points_scratch_bytes(H, W));
    HeatmapPointsArgs a{};
    a.heatmap = heatmap_dev; a.H = H; a.W = W; a.conf_thresh = conf_thresh; a.nms_dist = nms_dist; a.border = 4; a.top_k = top_k;
    a.subpixel = subpixel != 0; a.pts = pts_dev; a.cap = cap; a.count = count_dev; a.scratch = scratch;
    RUN("heatmap_points", launch_heatmap_points(a, s));
    // the scratch's counter words: [0 .. kHeatmapPointsRounds) pixels still undecided after each bounded round, then how many the
    // unbounded pass took over, then the survivors inside the border (32-bit integers; the fetch copies their bit patterns)
    tap(h, "hp_counters", scratch, {16});
    return 0;
  });
}

int imx_set_debug(imx_handle_t h, int enable) {
  return guarded(h, "imx_set_debug", [&]() -> int {
    if (!h) return -1;
    h->debug = enable != 0;
    return 0;
  });
}

int imx_debug_fetch(imx_handle_t h, const char* name, float* host_out, int64_t capacity, int64_t* shape_out, int* ndim_out) {
  return guarded(h, "imx_debug_fetch", [&]() -> int {
    if (!h) return -1;
    auto it = h->taps.find(name ? name : "");
    if (it == h->taps.end()) return fail(h, "imx_debug_fetch: no tap named '%s'", name ? name : "(null)");
    int64_t n = 1;
    for (int64_t v : it->second.shape) n *= v;
    if (ndim_out) *ndim_out = (int)it->second.shape.size();
    if (shape_out) for (size_t i = 0; i < it->second.shape.size() && i < 4; ++i) shape_out[i] = it->second.shape[i];
    if (!host_out) return 0;   // shape query
    if (capacity < n) return fail(h, "imx_debug_fetch: capacity %lld < %lld elements", (long long)capacity, (long long)n);
    HIP_OK(h, hipSetDevice(h->device));
    HIP_OK(h, hipDeviceSynchronize());
    if (h->nms_lazy.pending && name && std::string(name) == "nms") {
      auto& z = h->nms_lazy;
      HIP_OK(h, launch_nms(z.smap, z.nms, z.B, z.H, z.W, z.radius, nullptr, z.scratch));
      HIP_OK(h, hipDeviceSynchronize());
      z.pending = false;
    }
    if (!it->second.blocked) {
      HIP_OK(h, hipMemcpy(host_out, it->second.p, (size_t)n * 4, hipMemcpyDeviceToHost));
      return 0;
    }
    // channel-blocked activation (B, C/8, H, W, 8) -> the NHWC tensor the tap promises
    std::vector<float> raw((size_t)n);
    HIP_OK(h, hipMemcpy(raw.data(), it->second.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    const int64_t Bn = it->second.shape[0], Hn = it->second.shape[1], Wn = it->second.shape[2], Cn = it->second.shape[3];
    for (int64_t bb = 0; bb < Bn; ++bb)
      for (int64_t ck = 0; ck < Cn / 8; ++ck)
        for (int64_t yx = 0; yx < Hn * Wn; ++yx)
          for (int64_t c = 0; c < 8; ++c)
            host_out[(bb * Hn * Wn + yx) * Cn + ck * 8 + c] = raw[((bb * (Cn / 8) + ck) * Hn * Wn + yx) * 8 + c];
    return 0;
  });
}

int imx_set_timing(imx_handle_t h, int enable) {
  return guarded(h, "imx_set_timing", [&]() -> int {
    if (!h) return -1;
    h->timing = enable != 0;
    return 0;
  });
}

int imx_timing_reset(imx_handle_t h) {
  return guarded(h, "imx_timing_reset", [&]() -> int {
    if (!h) return -1;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    for (auto& e : h->events) { (void)hipEventDestroy(e.e0); (void)hipEventDestroy(e.e1); }
    h->events.clear();
    h->report.clear();
    return 0;
  });
}

int imx_timing_report(imx_handle_t h, int index, const char** name_out, int64_t* launches_out, double* total_ms_out) {
  return guarded(h, "imx_timing_report", [&]() -> int {
    if (!h) return -1;
    if (index < 0) {   // (re)build the report; returns the number of rows
      HIP_OK(h, hipSetDevice(h->device));
      HIP_OK(h, hipDeviceSynchronize());
      std::map<std::string, TimingRow> agg;      // keyed by name + form: a name whose launches took different forms gets one row per form
      std::vector<std::string> order;
      for (auto& e : h->events) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, e.e0, e.e1) != hipSuccess) continue;
        const std::string form = e.form ? e.form : "", key = e.name + "|" + form;
        auto it = agg.find(key);
        if (it == agg.end()) { agg[key] = TimingRow{e.name, form, 1, ms}; order.push_back(key); }
        else { it->second.launches++; it->second.ms += ms; }
      }
      h->report.clear();
      for (auto& n : order) h->report.push_back(agg[n]);
      return (int)h->report.size();
    }
    if ((size_t)index >= h->report.size()) return fail(h, "imx_timing_report: index %d out of range", index);
    if (name_out) *name_out = h->report[index].name.c_str();
    if (launches_out) *launches_out = h->report[index].launches;
    if (total_ms_out) *total_ms_out = h->report[index].ms;
    return 0;
  });
}

const char* imx_timing_form(imx_handle_t h, int index) {
  if (!h || index < 0 || (size_t)index >= h->report.size()) return "";
  return h->report[index].form.c_str();
}

int imx_set_option(imx_handle_t h, const char* key, const char* value) {
  return guarded(h, "imx_set_option", [&]() -> int {
    if (!h) return -1;
    if (!key || !value) return fail(h, "imx_set_option: null argument");
    if (apply_option(h, key, value)) return fail(h, "imx_set_option: unknown option or value '%s' = '%s' (%s)", key, value, option_listing().c_str());
    return 0;
  });
}

const char* imx_get_option(imx_handle_t h, const char* key) {
  if (!h || !key) return "";
  try {
    return get_option(h, key);
  } catch (...) {
    return "";
  }
}

}  // extern "C"
