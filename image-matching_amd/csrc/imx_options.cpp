// imx_options.cpp -- the handle options of libimx.so (imx_set_option / imx_get_option; the environment seeds some at imx_create): one
// table holds every key and every spelling of its values.
#include "imx_host.h"

#include <cctype>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace imx::host {

namespace {

struct OptValue { const char* text; int value; };
// One row per key imx_set_option accepts: the ONLY place a key or a value is spelled.  `values`: the canonical spellings, in the order
// the error message lists them (imx_get_option answers with these); `aliases`: what is accepted beside them.  A row without a field
// goes through its hooks: set(handle, value) -> 0 / -1 and get(handle) -> value.  `env`: IMX_<KEY> seeds the option at imx_create.
// The read-only "arith_guard" (arith_guard_text below) is not a row.  Meanings: the Options struct in imx_kernels.h, include/imx.h.
struct OptionRow {
  const char* key;
  int Options::*field;
  bool env;
  OptValue values[5], aliases[4];
  int (*set)(imx_handle_t, int);
  int (*get)(imx_handle_t);
};

// "conv": one key, two fields ("direct" leaves the Winograd form as it was); -2 = "wx3", round 3's bf16-plane experiment, deleted in
// round 4: its nearest living form
int set_conv(imx_handle_t h, int v) {
  Options& o = h->opt;
  if (v == -2) {
    fprintf(stderr, "imx: conv = wx3 was removed (round 4); using wino32\n");
    v = 0;
  }
  if (v < 0) o.conv_direct = 1;
  else { o.conv_direct = 0; o.conv_f16 = v; }
  return 0;
}
int get_conv(imx_handle_t h) { return h->opt.conv_direct ? -1 : h->opt.conv_f16; }

// the test hook "debug_poison" (poisonable() in imx_host.h): the byte pattern as floats: 0xFF.. a NaN, 0x7F7F7F7F = 3.4e38, 0
int set_poison(imx_handle_t h, int byte) {
  if (byte >= 0) {
    if (hipSetDevice(h->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return -1;
    for (auto& kv : h->bufs)
      if (kv.second.p && poisonable(kv.first) && hipMemset(kv.second.p, byte, kv.second.bytes) != hipSuccess) return -1;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    h->nms_lazy.pending = false;   // (its inputs are gone: the "nms" tap now reads what every other tap reads, the pattern)
    h->sg_last.valid = false;      // (likewise the score matrix and potentials imx_match_loss would read)
  }
  h->poison = byte;
  return 0;
}
int get_poison(imx_handle_t h) { return h->poison; }

const OptionRow kOptionTable[] = {
  {"mfma", &Options::mfma_f32, true, {{"x3", 0}, {"f32", 1}}},
  {"latency_forms", &Options::latency_forms, true, {{"auto", -1}, {"off", 0}, {"on", 1}, {"unfused", 2}}, {{"0", 0}, {"1", 1}}},
  {"conv", nullptr, true, {{"wino", 1}, {"wino_h", 2}, {"wino32", 0}, {"direct", -1}}, {{"wx3", -2}}, set_conv, get_conv},
  {"gnn_tail", &Options::gnn_tail, true, {{"auto", -1}, {"fused", 1}, {"bf16x3", 2}, {"unfused", 0}}, {{"0", 0}, {"1", 1}}},
  {"attention", &Options::attention, true, {{"auto", -1}, {"f16x2", 1}, {"bf16x3", 0}}, {{"x3", 0}, {"0", 0}, {"1", 1}}},
  {"linear", &Options::linear, true, {{"auto", -1}, {"f16x2", 1}, {"bf16x3", 0}}, {{"x3", 0}, {"0", 0}, {"1", 1}}},
  {"attention_qblocks", &Options::attention_qblocks, true, {{"auto", -1}, {"1", 1}, {"2", 2}}},
  {"conv_swizzle", &Options::conv_swizzle, false, {{"on", 1}, {"off", 0}}, {{"1", 1}, {"0", 0}}},
  {"qkv_amax", &Options::qkv_amax, false, {{"epilogue", 0}, {"kernel", 1}}},
  {"sinkhorn_group", &Options::sinkhorn_group, false, {{"auto", 0}, {"1", 1}, {"2", 2}, {"4", 4}}, {{"0", 0}}},
  {"sinkhorn_prefetch", &Options::sinkhorn_prefetch, false, {{"auto", -1}, {"off", 0}, {"on", 1}}, {{"0", 0}, {"1", 1}}},
  {"sinkhorn_merge", &Options::sinkhorn_merge, false, {{"auto", -1}, {"kernel", 0}, {"fused", 1}}},
  {"keypoints", &Options::keypoints, false, {{"auto", -1}, {"dense", 0}, {"bits", 1}}},
  {"ha_masks", &Options::ha_masks, false, {{"stored", 0}, {"recompute", 1}}},
  {"debug_poison", nullptr, false, {{"off", -1}, {"nan", 0xFF}, {"huge", 0x7F}, {"zero", 0x00}}, {}, set_poison, get_poison},
};

const OptionRow* find_row(const char* key) {
  for (const OptionRow& r : kOptionTable)
    if (!strcmp(r.key, key)) return &r;
  return nullptr;
}

// read-only: what the weights-derived guards decided (after imx_finalize_weights)
const char* arith_guard_text(imx_handle_t h) {
  char buf[96];
  const float sp = conv_chain_spread(h);
  snprintf(buf, sizeof buf, "conv: max spread 2^%.1f -> %s; gnn_tail bf16x3 layers:", std::log2(std::max(sp, 1.f)), conv_spread_ok(sp) ? "f16x2" : "f32");
  h->opt_text = buf;
  for (size_t l = 0; l < h->layers.size(); ++l)
    if (h->layers[l].tail_stream_h2 && !tail_h2_safe(h->layers[l])) h->opt_text += " " + std::to_string(l);
  float lx = 0.f;
  for (const auto& L : h->layers) lx = std::max(lx, std::max(L.h2c.loose_h, L.h2c.loose_x));
  snprintf(buf, sizeof buf, " (largest bound looseness 2^%.1f)", std::log2(std::max(lx, 1.f)));
  h->opt_text += buf;
  h->opt_text += "; attention bf16x3 layers:";
  float qs = 1.f;
  for (size_t l = 0; l < h->layers.size(); ++l) {
    qs = std::max(qs, h->layers[l].qkv_spread);
    if (!attn_f16x2_ok(h->layers[l])) h->opt_text += " " + std::to_string(l);
  }
  snprintf(buf, sizeof buf, " (largest q|k|v channel spread 2^%.1f)", std::log2(qs));
  h->opt_text += buf;
  float ws = 1.f;
  for (const auto& L : h->layers) ws = std::max(ws, std::max(L.qkv.wh2_spread, std::max(L.mlp1.wh2_spread, L.mlp2.wh2_spread)));
  snprintf(buf, sizeof buf, "; linear: max spread 2^%.1f -> %s", std::log2(ws), linear_chain_h2_ok(h) ? "f16x2" : "bf16x3");
  h->opt_text += buf;
  return h->opt_text.c_str();
}

}  // namespace

int apply_option(imx_handle_t h, const std::string& key, const std::string& v) {
  const OptionRow* r = find_row(key.c_str());
  if (!r) return -1;
  for (const auto* list : {r->values, r->aliases})
    for (const OptValue* o = list; o->text; ++o)
      if (v == o->text) return r->set ? r->set(h, o->value) : (h->opt.*r->field = o->value, 0);
  return -1;
}

const char* get_option(imx_handle_t h, const char* key) {
  if (!strcmp(key, "arith_guard")) return arith_guard_text(h);
  const OptionRow* r = find_row(key);
  if (!r) return "";
  const int cur = r->get ? r->get(h) : h->opt.*r->field;
  for (const OptValue* o = r->values; o->text; ++o)
    if (o->value == cur) return o->text;
  return "";
}

std::string option_listing() {
  std::string out;
  for (const OptionRow& r : kOptionTable) {
    out += std::string(out.empty() ? "" : ", ") + r.key + " = ";
    for (const OptValue* o = r.values; o->text; ++o) out += std::string(o == r.values ? "" : "|") + o->text;
  }
  return out;
}

// the environment seeds the options once, at imx_create; afterwards only imx_set_option changes them
int seed_options_from_env(imx_handle_t h) {
  for (const OptionRow& r : kOptionTable) {
    if (!r.env) continue;
    std::string env = std::string("IMX_") + r.key;
    for (char& ch : env) ch = (char)toupper((unsigned char)ch);
    if (const char* e = getenv(env.c_str()))
      if (apply_option(h, r.key, e)) return fail(nullptr, "imx_create: bad value '%s' in the environment variable %s", e, env.c_str());
  }
  return 0;
}

}  // namespace imx::host
