// imx_weights.cpp -- checkpoint keys, BatchNorm folding and every weight packer of libimx.so: what imx_finalize_weights moves to the
// device, once per checkpoint, in the layouts the kernels read (imx_kernels.h, wino24_pack.h, gnn_tail_pack.h).
#include "imx_host.h"
#include "wino24_pack.h"

#include <cmath>
#include <cstring>

namespace imx::host {
namespace {

constexpr double BN_EPS = 1e-5;   // nn.BatchNorm default (unet_parts.py:16; superglue_test.py:58)

// ----------------------------------------------------------------------------- expected keys
void add_conv_keys(std::map<std::string, std::vector<int64_t>>& m, const std::string& conv, int cout, int cin, int k,
                   const std::string& bn) {
  if (k > 0) m[conv + ".weight"] = {cout, cin, k, k}; else m[conv + ".weight"] = {cout, cin, 1};
  m[conv + ".bias"] = {cout};
  if (!bn.empty())
    for (const char* leaf : {"weight", "bias", "running_mean", "running_var"}) m[bn + "." + leaf] = {cout};
}

// the eight 3x3 layers of the shared encoder: conv key ck[i] and BatchNorm key bk[i] ("" without one) in the checkpoint of either variant
void sp_encoder_keys(bool bn, std::string (&ck)[8], std::string (&bk)[8]) {
  const char* blocks[4] = {"inc.conv.conv", "down1.mpconv.1.conv", "down2.mpconv.1.conv", "down3.mpconv.1.conv"};
  const char* names[8] = {"conv1a", "conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b"};
  for (int i = 0; i < 8; ++i) {
    ck[i] = bn ? std::string(blocks[i / 2]) + (i % 2 ? ".3" : ".0") : names[i];
    bk[i] = bn ? std::string(blocks[i / 2]) + (i % 2 ? ".4" : ".1") : "";
  }
}

}  // namespace

void build_expected(imx_handle_t h) {
  const imx_config_t& c = h->cfg;
  auto& sp = h->expected[IMX_NET_SUPERPOINT];
  const int c1 = 64, c2 = 64, c3 = 128, c4 = 128, c5 = 256, d = c.descriptor_dim;
  const bool bn = c.sp_variant == IMX_SP_VARIANT_BN;
  std::string ck[8], bk[8];
  sp_encoder_keys(bn, ck, bk);
  const int cin[8] = {1, c1, c1, c2, c2, c3, c3, c4}, cout[8] = {c1, c1, c2, c2, c3, c3, c4, c4};
  for (int i = 0; i < 8; ++i) add_conv_keys(sp, ck[i], cout[i], cin[i], 3, bk[i]);
  add_conv_keys(sp, "convPa", c5, c4, 3, bn ? "bnPa" : "");
  add_conv_keys(sp, "convPb", 65, c5, 1, bn ? "bnPb" : "");
  add_conv_keys(sp, "convDa", c5, c4, 3, bn ? "bnDa" : "");
  add_conv_keys(sp, "convDb", d, c5, 1, bn ? "bnDb" : "");
  auto& sg = h->expected[IMX_NET_SUPERGLUE];
  sg["bin_score"] = {};
  std::vector<int> ch = {3};
  for (int i = 0; i < c.kenc_n; ++i) ch.push_back(c.kenc_channels[i]);
  ch.push_back(d);
  for (size_t i = 1; i < ch.size(); ++i) {
    int j = 3 * (int)(i - 1);
    std::string p = "kenc.encoder." + std::to_string(j);
    add_conv_keys(sg, p, ch[i], ch[i - 1], 0, i + 1 < ch.size() ? "kenc.encoder." + std::to_string(j + 1) : "");
  }
  for (int l = 0; l < c.num_gnn_layers; ++l) {
    std::string p = "gnn.layers." + std::to_string(l);
    add_conv_keys(sg, p + ".attn.merge", d, d, 0, "");
    for (int k = 0; k < 3; ++k) add_conv_keys(sg, p + ".attn.proj." + std::to_string(k), d, d, 0, "");
    add_conv_keys(sg, p + ".mlp.0", 2 * d, 2 * d, 0, p + ".mlp.1");
    add_conv_keys(sg, p + ".mlp.3", d, 2 * d, 0, "");
  }
  add_conv_keys(sg, "final_proj", d, d, 0, "");
}

namespace {

// ----------------------------------------------------------------------------- weight folding
void* upload_bytes(imx_handle_t h, const void* src, size_t bytes) {
  void* p = nullptr;
  if (hipMalloc(&p, bytes + 16) != hipSuccess) return nullptr;
  if (hipMemcpy(p, src, bytes, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(p);
    return nullptr;
  }
  h->weight_allocs[h->upload_net].push_back(p);
  return p;
}
float* upload(imx_handle_t h, const std::vector<float>& v) { return static_cast<float*>(upload_bytes(h, v.data(), v.size() * sizeof(float))); }
void* upload_u16(imx_handle_t h, const std::vector<uint16_t>& v) { return upload_bytes(h, v.data(), v.size() * 2); }
// 16-bit patterns packed two per float slot (bit patterns only)
std::vector<float> as_float_words(const std::vector<uint16_t>& pl) {
  std::vector<float> out((pl.size() + 1) / 2);
  memcpy(out.data(), pl.data(), pl.size() * sizeof(uint16_t));
  return out;
}

// per-output-channel scale s and shift t such that BN(conv + b) = conv*s + t
void fold_bn(const std::map<std::string, HostTensor>& raw, const std::string& conv, const std::string& bn, int cout,
             std::vector<double>& s, std::vector<double>& t) {
  const std::vector<float>& b = raw.at(conv + ".bias").data;
  s.assign(cout, 1.0);
  t.resize(cout);
  if (bn.empty()) {
    for (int c = 0; c < cout; ++c) t[c] = b[c];
    return;
  }
  const auto& g = raw.at(bn + ".weight").data;
  const auto& be = raw.at(bn + ".bias").data;
  const auto& mu = raw.at(bn + ".running_mean").data;
  const auto& var = raw.at(bn + ".running_var").data;
  for (int c = 0; c < cout; ++c) {
    s[c] = (double)g[c] / std::sqrt((double)var[c] + BN_EPS);
    t[c] = ((double)b[c] - (double)mu[c]) * s[c] + (double)be[c];
  }
}

// torch Conv2d (Cout,Cin,3,3) -> [tap = ky*3+kx][ci][co_off + co] of a [9][Cin][cout_total] buffer
void put_conv3(const std::map<std::string, HostTensor>& raw, const std::string& conv, const std::string& bn, int cin,
               int cout, int cout_total, int co_off, std::vector<float>& w, std::vector<float>& bias) {
  std::vector<double> s, t;
  fold_bn(raw, conv, bn, cout, s, t);
  const std::vector<float>& src = raw.at(conv + ".weight").data;
  for (int co = 0; co < cout; ++co) {
    for (int ci = 0; ci < cin; ++ci)
      for (int tp = 0; tp < 9; ++tp)
        w[((size_t)tp * cin + ci) * cout_total + co_off + co] = (float)((double)src[((size_t)co * cin + ci) * 9 + tp] * s[co]);
    bias[co_off + co] = (float)t[co];
  }
}

int upload_conv(imx_handle_t h, ConvW& out, const std::vector<float>& w, const std::vector<float>& b, int cin, int cout, const char* what) {
  out.w = upload(h, w);
  out.wu24 = upload(h, wino24_transform(w, cin, cout));
  if (cin % 64 == 0 && cout % 64 == 0) out.wuh = upload_u16(h, wino24h_pack(w, cin, cout, &out.su_inv, &out.u_spread));
  out.b = upload(h, b);
  out.cin = cin;
  out.cout = cout;
  return (out.w && out.wu24 && out.b) ? 0 : fail(h, "weight upload failed (%s)", what);
}

int make_conv(imx_handle_t h, ConvW& out, const std::map<std::string, HostTensor>& raw, const std::string& conv,
              const std::string& bn, int cin, int cout) {
  std::vector<float> w((size_t)9 * cin * cout), b(cout);
  put_conv3(raw, conv, bn, cin, cout, cout, 0, w, b);
  return upload_conv(h, out, w, b, cin, cout, conv.c_str());
}

// linear weight (N,K[,1[,1]]) -> W[k_perm(k)][n_perm(n)] padded to Npad columns, folded BN
void build_gemm_host(const std::map<std::string, HostTensor>& raw, const std::string& conv, const std::string& bn, int K,
                     int N, const std::vector<int>* kperm, std::vector<float>& w, std::vector<float>& b, int& Npad) {
  Npad = ((N + 63) / 64) * 64;
  std::vector<double> s, t;
  fold_bn(raw, conv, bn, N, s, t);
  const std::vector<float>& src = raw.at(conv + ".weight").data;
  w.assign((size_t)K * Npad, 0.f);
  b.assign(Npad, 0.f);
  for (int n = 0; n < N; ++n) {
    for (int k = 0; k < K; ++k) {
      const int kk = kperm ? (*kperm)[k] : k;   // kk = position of reference input channel k in OUR layout
      w[(size_t)kk * Npad + n] = (float)((double)src[(size_t)n * K + k] * s[n]);
    }
    b[n] = (float)t[n];
  }
}

// x = h + m + l with three bf16 terms (round-to-nearest-even residuals; exact for every finite fp32 whose last term does not
// underflow): W[k][n] -> planes [3][Npad][K], k contiguous, packed two bf16 per float slot (bit patterns only)
std::vector<float> split_bf16x3(const std::vector<float>& w, int K, int Npad) {
  // fragment order of v_mfma_f32_32x32x16_bf16's B operand (pack_host.h: b_fragment_index)
  std::vector<uint16_t> pl((size_t)3 * Npad * K);
  for (int k = 0; k < K; ++k)
    for (int n = 0; n < Npad; ++n) {
      uint16_t t[3];
      gt_split(w[(size_t)k * Npad + n], t);
      for (int q = 0; q < 3; ++q) pl[b_fragment_index(k, n, K, 3, q)] = t[q];
    }
  return as_float_words(pl);
}

// W [K][Npad] -> [K/16][4 (kq)][Npad][4 (j)], element (t, kq, col, j) = W[16 t + 4 kq + j][col]: the four B values a lane of
// v_mfma_f32_16x16x4_f32 feeds to the four MFMAs of a 16-k group are one 16-byte load, sixteen lanes 256 contiguous bytes
std::vector<float> fragment_order(const std::vector<float>& w, int K, int Npad) {
  std::vector<float> f((size_t)K * Npad);
  for (int t = 0; t < K / 16; ++t)
    for (int kq = 0; kq < 4; ++kq)
      for (int col = 0; col < Npad; ++col)
        for (int j = 0; j < 4; ++j) f[(((size_t)t * 4 + kq) * Npad + col) * 4 + j] = w[(size_t)(16 * t + 4 * kq + j) * Npad + col];
  return f;
}

// w s = h + m with two fp16 planes, s = the power of two that brings max |w| to [2^13, 2^14) (round-to-nearest-even, subnormals kept:
// exact to 2^-38 of max |w|), in the fragment order of v_mfma_f32_32x32x16_f16's B operand (pack_host.h: b_fragment_index).
// Returns 1 / s and the spread (GemmW::wh2_spread).
std::vector<float> split_f16x2(const std::vector<float>& w, int K, int N, int Npad, float* s_inv, float* spread) {
  double mx = 0.0;
  std::vector<double> colmax(N > 0 ? N : 1, 0.0);
  for (int k = 0; k < K; ++k)
    for (int n = 0; n < N; ++n) {
      const double a = std::fabs((double)w[(size_t)k * Npad + n]);
      colmax[n] = std::max(colmax[n], a);
      mx = std::max(mx, a);
    }
  *spread = (float)std::min(1e30, spread_over_median(std::move(colmax), mx, 1e30));
  const double sc = pow2_scale_for(mx);
  *s_inv = (float)(1.0 / sc);
  std::vector<uint16_t> pl((size_t)2 * Npad * K);
  for (int k = 0; k < K; ++k)
    for (int n = 0; n < Npad; ++n) {
      const float x = (float)((double)w[(size_t)k * Npad + n] * sc);
      const uint16_t hh = f16_rne(x), mm = f16_rne(x - f16_to_f32(hh));
      pl[b_fragment_index(k, n, K, 2, 0)] = hh;
      pl[b_fragment_index(k, n, K, 2, 1)] = mm;
    }
  return as_float_words(pl);
}

// (stat_N: the columns that enter the spread statistic of the fp16 planes where fewer than N are real -- zero-padded widths)
int upload_gemm(imx_handle_t h, GemmW& out, const std::vector<float>& w, const std::vector<float>& b, int K, int N, int Npad,
                const char* what, int stat_N = -1) {
  out.w = upload(h, w);
  out.wf = (K % 16 == 0 && K <= 512 && N == Npad) ? upload(h, fragment_order(w, K, Npad)) : nullptr;
  out.wx3 = upload(h, split_bf16x3(w, K, Npad));
  if (K % 32 == 0 && Npad % 64 == 0) out.wh2 = upload(h, split_f16x2(w, K, stat_N > 0 ? stat_N : N, Npad, &out.wh2_inv, &out.wh2_spread));
  out.b = upload(h, b);
  out.K = K;
  out.N = N;
  out.Npad = Npad;
  return (out.w && out.wx3 && out.b) ? 0 : fail(h, "weight upload failed (%s)", what);
}

int make_gemm(imx_handle_t h, GemmW& out, const std::map<std::string, HostTensor>& raw, const std::string& conv,
              const std::string& bn, int K, int N, const std::vector<int>* kperm = nullptr) {
  std::vector<float> w, b;
  int Npad = 0;
  build_gemm_host(raw, conv, bn, K, N, kperm, w, b, Npad);
  return upload_gemm(h, out, w, b, K, N, Npad, conv.c_str());
}

}  // namespace

int finalize_superpoint(imx_handle_t h) {
  const auto& raw = h->raw[IMX_NET_SUPERPOINT];
  const bool bn = h->cfg.sp_variant == IMX_SP_VARIANT_BN;
  const int d = h->cfg.descriptor_dim;
  std::string ck[8], bk[8];
  sp_encoder_keys(bn, ck, bk);
  // conv1a: (64,1,3,3) -> [9][64]
  {
    std::vector<float> w(9 * 64), b(64);
    put_conv3(raw, ck[0], bk[0], 1, 64, 64, 0, w, b);
    h->w1 = upload(h, w);
    h->b1 = upload(h, b);
    if (!h->w1 || !h->b1) return fail(h, "weight upload failed (conv1a)");
    // |conv1a output| <= max|image patch| * c1a_l1 + c1a_bmax (conv1ab_wino24h.hip's per-tile scale)
    h->c1a_l1 = 0.f; h->c1a_bmax = 0.f;
    for (int c = 0; c < 64; ++c) {
      float l1 = 0.f;
      for (int t = 0; t < 9; ++t) l1 += std::fabs(w[t * 64 + c]);
      h->c1a_l1 = std::max(h->c1a_l1, l1);
      h->c1a_bmax = std::max(h->c1a_bmax, std::fabs(b[c]));
    }
    h->c1a_l1 = std::max(h->c1a_l1, 1e-30f);
    // conv1a's weights meet no fp16 scale (fp32 pipe), but an output channel far above the others is what conv1b's input transform then
    // sees -- one channel owning the tile's power of two, the typical channel 2^k below it.  wino24h_pack's statistic on the plain
    // weights (the rescale conv1a x 2^k / conv1b's column x 2^-k showed in no transformed-weight table)
    std::vector<double> comax(64, 0.0);
    double wmax = 0.0;
    for (int t = 0; t < 9; ++t)
      for (int c = 0; c < 64; ++c) {
        comax[c] = std::max(comax[c], (double)std::fabs(w[t * 64 + c]));
        wmax = std::max(wmax, comax[c]);
      }
    h->c1a_spread = (float)std::min(3.0e38, spread_over_median(std::move(comax), wmax, 3.0e38));
  }
  const int cin[8] = {1, 64, 64, 64, 64, 128, 128, 128}, cout[8] = {64, 64, 64, 64, 128, 128, 128, 128};
  for (int i = 1; i < 8; ++i)
    if (make_conv(h, h->conv[i - 1], raw, ck[i], bk[i], cin[i], cout[i])) return -1;
  // heads: convPa | convDa merged into one 128 -> 512 convolution
  {
    std::vector<float> w((size_t)9 * 128 * 512), b(512);
    put_conv3(raw, "convPa", bn ? "bnPa" : "", 128, 256, 512, 0, w, b);
    put_conv3(raw, "convDa", bn ? "bnDa" : "", 128, 256, 512, 256, w, b);
    if (upload_conv(h, h->conv[7], w, b, 128, 512, "heads")) return -1;
  }
  if (make_gemm(h, h->pb, raw, "convPb", bn ? "bnPb" : "", 256, 65)) return -1;
  if (make_gemm(h, h->db, raw, "convDb", bn ? "bnDb" : "", 256, d)) return -1;
  return 0;
}

int finalize_superglue(imx_handle_t h) {
  const auto& raw = h->raw[IMX_NET_SUPERGLUE];
  const imx_config_t& c = h->cfg;
  const int d = c.descriptor_dim;
  if (d % HEADS != 0 || (d / HEADS != 16 && d / HEADS != 32 && d / HEADS != 64))
    return fail(h, "SuperGlue needs descriptor_dim/4 in {16,32,64} (got descriptor_dim=%d)", d);
  h->bin_score = raw.at("bin_score").data[0];
  std::vector<int> ch = {3};
  for (int i = 0; i < c.kenc_n; ++i) ch.push_back(c.kenc_channels[i]);
  ch.push_back(d);
  for (size_t i = 1; i < ch.size(); ++i)
    if (ch[i] < 1) return fail(h, "keypoint_encoder widths must be positive (got %d)", ch[i]);
  // The kernels take widths that are multiples of 32.  Any other width (the reference accepts every positive one) is padded with
  // channels whose folded weights and biases are zero: they stay 0 through the ReLU and meet zero rows of the next layer's matrix,
  // so every sum of the layer gains exact zeros only.
  std::vector<int> cp(ch);
  for (size_t i = 1; i < cp.size(); ++i) cp[i] = (ch[i] + 31) / 32 * 32;
  // layer 0: (C1,3,1) + BN -> w[3][C1]
  {
    const int C1 = cp[1];
    std::vector<double> s, t;
    fold_bn(raw, "kenc.encoder.0", ch.size() > 2 ? "kenc.encoder.1" : "", ch[1], s, t);
    const auto& src = raw.at("kenc.encoder.0.weight").data;
    std::vector<float> w(3 * C1, 0.f), b(C1, 0.f);
    for (int n = 0; n < ch[1]; ++n) {
      for (int k = 0; k < 3; ++k) w[k * C1 + n] = (float)((double)src[n * 3 + k] * s[n]);
      b[n] = (float)t[n];
    }
    h->kenc0_w = upload(h, w);
    h->kenc0_b = upload(h, b);
    h->kenc_c1 = C1;
    if (!h->kenc0_w || !h->kenc0_b) return fail(h, "weight upload failed (kenc0)");
  }
  h->kenc.clear();
  for (size_t i = 2; i < ch.size(); ++i) {
    int j = 3 * (int)(i - 1);
    GemmW g;
    const std::string conv = "kenc.encoder." + std::to_string(j);
    std::vector<float> w, b;
    int Npad = 0;
    build_gemm_host(raw, conv, i + 1 < ch.size() ? "kenc.encoder." + std::to_string(j + 1) : "", ch[i - 1], ch[i], nullptr, w, b, Npad);
    w.resize((size_t)cp[i - 1] * Npad, 0.f);      // (rows of the padded input channels; the padded output columns are zero already)
    if (upload_gemm(h, g, w, b, cp[i - 1], cp[i], Npad, conv.c_str(), ch[i])) return -1;
    h->kenc.push_back(g);
  }
  // channel permutation: reference channel c = dim*HEADS + head (view(b, dim, heads, n),
  // superglue_test.py:104)  ->  ours = head*HD + dim
  const int HD = d / HEADS;
  std::vector<int> perm(d);
  for (int cidx = 0; cidx < d; ++cidx) perm[cidx] = (cidx % HEADS) * HD + cidx / HEADS;
  h->layers.clear();
  std::vector<std::vector<float>> host_qkv, host_w1, host_w2;      // host copies for the fused layer tail's weight stream (d = 128)
  std::vector<int> host_ld1, host_ld2;
  for (int l = 0; l < c.num_gnn_layers; ++l) {
    std::string p = "gnn.layers." + std::to_string(l);
    GnnLayer L;
    // fused q|k|v projection: W[k][which*d + perm(n)]
    {
      const int N = 3 * d;
      std::vector<float> w((size_t)d * N, 0.f), b(N, 0.f);
      for (int which = 0; which < 3; ++which) {
        const auto& src = raw.at(p + ".attn.proj." + std::to_string(which) + ".weight").data;
        const auto& bs = raw.at(p + ".attn.proj." + std::to_string(which) + ".bias").data;
        for (int n = 0; n < d; ++n) {
          for (int k = 0; k < d; ++k) w[(size_t)k * N + which * d + perm[n]] = src[(size_t)n * d + k];
          b[which * d + perm[n]] = bs[n];
        }
      }
      host_qkv.push_back(w);
      L.qkv_spread = 1.f;
      for (int which = 0; which < 3; ++which) {
        std::vector<double> l2(d, 0.0);
        for (int n = 0; n < d; ++n) {
          double sq = 0.0;
          for (int k = 0; k < d; ++k) sq += (double)w[(size_t)k * N + which * d + n] * w[(size_t)k * N + which * d + n];
          l2[n] = std::sqrt(sq);
        }
        const double mx = *std::max_element(l2.begin(), l2.end());
        L.qkv_spread = std::max(L.qkv_spread, (float)std::min(1e30, spread_over_median(std::move(l2), mx, 1e30)));
      }
      if (upload_gemm(h, L.qkv, w, b, d, N, N, (p + " qkv").c_str())) return -1;
    }
    // attn.merge is linear and feeds only mlp.0's second input half (superglue_test.py:107,119):
    //   mlp.0([x ; Wm a + bm]) = W1x x + (W1m Wm) a + (W1m bm + b1)
    // so the merge GEMM is folded into the (BN-folded) mlp.0 weights once, in double, and the kernel
    // chain per layer is qkv -> attention -> mlp1([x | a]) -> mlp2 (+residual).
    {
      std::vector<float> wm, bm, w1, b1;
      int npm = 0, np1 = 0;
      build_gemm_host(raw, p + ".attn.merge", "", d, d, &perm, wm, bm, npm);      // wm[a_ch (ours)][c], bm[c]
      build_gemm_host(raw, p + ".mlp.0", p + ".mlp.1", 2 * d, 2 * d, nullptr, w1, b1, np1);
      std::vector<float> wf((size_t)2 * d * np1, 0.f), bf(b1);
      for (int k = 0; k < d; ++k)
        for (int n = 0; n < 2 * d; ++n) wf[(size_t)k * np1 + n] = w1[(size_t)k * np1 + n];
      for (int n = 0; n < 2 * d; ++n) {
        double accb = b1[n];
        for (int cch = 0; cch < d; ++cch) accb += (double)bm[cch] * (double)w1[(size_t)(d + cch) * np1 + n];
        bf[n] = (float)accb;
      }
      for (int kk = 0; kk < d; ++kk)
        for (int n = 0; n < 2 * d; ++n) {
          double acc = 0.0;
          for (int cch = 0; cch < d; ++cch) acc += (double)wm[(size_t)kk * npm + cch] * (double)w1[(size_t)(d + cch) * np1 + n];
          wf[(size_t)(d + kk) * np1 + n] = (float)acc;
        }
      if (upload_gemm(h, L.mlp1, wf, bf, 2 * d, 2 * d, np1, (p + ".mlp.0 (+merge)").c_str())) return -1;
      for (int n = 0; n < 2 * d; ++n) L.bmax_1 = std::max(L.bmax_1, std::fabs(bf[n]));
      host_w1.push_back(wf);
      host_ld1.push_back(np1);
    }
    {
      std::vector<float> w2, b2;
      int np2 = 0;
      build_gemm_host(raw, p + ".mlp.3", "", 2 * d, d, nullptr, w2, b2, np2);
      if (upload_gemm(h, L.mlp2, w2, b2, 2 * d, d, np2, (p + ".mlp.3").c_str())) return -1;
      for (int n = 0; n < d; ++n) L.bmax_2 = std::max(L.bmax_2, std::fabs(b2[n]));
      host_w2.push_back(w2);
      host_ld2.push_back(np2);
    }
    h->layers.push_back(L);
  }
  std::vector<float> wfin, bfin;
  int npf = 0;
  build_gemm_host(raw, "final_proj", "", d, d, nullptr, wfin, bfin, npf);
  if (upload_gemm(h, h->final_proj, wfin, bfin, d, d, npf, "final_proj")) return -1;
  // the fused layer tail of the throughput path (gnn_tail.hip): one weight stream per layer, in consumption order
  if (d == 128) {
    for (int l = 0; l < c.num_gnn_layers; ++l) {
      const bool last = l + 1 == c.num_gnn_layers;
      const std::vector<uint16_t> st = gnn_tail_pack(host_w1[l].data(), host_ld1[l], host_w2[l].data(), host_ld2[l],
                                                     last ? wfin.data() : host_qkv[l + 1].data(), last ? npf : 3 * d, d, last ? d : 3 * d);
      h->layers[l].tail_stream = upload(h, as_float_words(st));
      if (!h->layers[l].tail_stream) return fail(h, "weight upload failed (layer %d tail stream)", l);
      h->layers[l].tail_stream_h2 = upload_u16(h, gnn_tail_pack_h2(host_w1[l].data(), host_ld1[l], host_w2[l].data(), host_ld2[l],
                                                                   last ? wfin.data() : host_qkv[l + 1].data(), last ? npf : 3 * d, d, last ? d : 3 * d,
                                                                   &h->layers[l].h2c));
      if (!h->layers[l].tail_stream_h2) return fail(h, "weight upload failed (layer %d fp16 tail stream)", l);
    }
  }
  return 0;
}

}  // namespace imx::host
