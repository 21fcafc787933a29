// imx_sgloop.cpp -- the host unit of libimx_sgloop.so (include/imx_sgloop.h), on the handle libimx.so made: the matches of SuperGlue's
// training forward from the loss's own Sinkhorn.  The extraction kernels are sgloop.hip's; the fused call runs otgrad.hip's kernels (the
// same source that libimx_train.so links, compiled into this library too) through the one launch sequence of otgrad_seq.h.  Scratch:
// "sgl.row_val", "sgl.row_idx" (B N0 words each) and "sgl.col_idx" (B N1), each written by the call before it is read.
#include "imx_host.h"
#include "otgrad_seq.h"
#include "sgloop.h"
#include "../../include/imx_sgloop.h"

namespace {

// the checks of the extraction's own arguments (the shape was checked by the caller) and its three launches; u / v with their per-pair strides
int extract_matches(imx_handle_t h, const char* who, int B, const float* scores, int N0, int N1, const int32_t* n0, const int32_t* n1, const float* u,
                    size_t su, const float* v, size_t sv, float threshold, const int64_t* gt0, int64_t* m0, int64_t* m1, float* ms0, float* ms1,
                    int32_t* stats, hipStream_t s) {
  SglArgs a{};
  a.scores = scores; a.n0 = n0; a.n1 = n1; a.u = u; a.v = v; a.su = su; a.sv = sv; a.B = B; a.N0 = N0; a.N1 = N1; a.threshold = threshold;
  a.gt0 = reinterpret_cast<const long long*>(gt0); a.matches0 = reinterpret_cast<long long*>(m0); a.matches1 = reinterpret_cast<long long*>(m1);
  a.mscores0 = ms0; a.mscores1 = ms1; a.stats = stats;
  WS(rv, float, "sgl.row_val", (size_t)B * N0 * sizeof(float));
  WS(ri, int, "sgl.row_idx", (size_t)B * N0 * sizeof(int));
  WS(ci, int, "sgl.col_idx", (size_t)B * N1 * sizeof(int));
  a.row_val = rv; a.row_idx = ri; a.col_idx = ci;
  RUN("sgl_row_max", launch_sgl_row_max(a, s));
  RUN("sgl_col_max", launch_sgl_col_max(a, s));
  RUN("sgl_mutual", launch_sgl_mutual(a, s));
  return 0;
}

int check_outputs(imx_handle_t h, const char* who, float threshold, const int64_t* gt0, const int64_t* m0, const int64_t* m1, const float* ms0,
                  const float* ms1, const int32_t* stats) {
  if (!m0 || !m1 || !ms0 || !ms1) return fail(h, "%s: null argument", who);
  if (!gt0 != !stats) return fail(h, "%s: gt0_dev and stats_dev go together (both or neither)", who);
  if (threshold != threshold) return fail(h, "%s: threshold is NaN", who);
  return 0;
}

}  // namespace

extern "C" {

int imx_assignment_matches(imx_handle_t h, int B, const float* scores_dev, int N0, int N1, const int32_t* n0_dev, const int32_t* n1_dev,
                           const float* u_dev, const float* v_dev, float threshold, const int64_t* gt0_dev, int64_t* matches0_dev,
                           int64_t* matches1_dev, float* mscores0_dev, float* mscores1_dev, int32_t* stats_dev, void* stream) {
  return on_device(h, "imx_assignment_matches", [&]() -> int {
    const char* who = "imx_assignment_matches";
    if (B < 1 || B > 65535 || N0 < 1 || N1 < 1 || N0 > (1 << 20) || N1 > (1 << 20))
      return fail(h, "%s: bad shape B=%d N0=%d N1=%d (B in [1,65535], N0 N1 in [1,2^20])", who, B, N0, N1);
    if (!scores_dev) return fail(h, "%s: null argument", who);
    if (check_outputs(h, who, threshold, gt0_dev, matches0_dev, matches1_dev, mscores0_dev, mscores1_dev, stats_dev)) return -1;
    return extract_matches(h, who, B, scores_dev, N0, N1, n0_dev, n1_dev, u_dev, (size_t)N0 + 1, v_dev, (size_t)N1 + 1, threshold, gt0_dev,
                           matches0_dev, matches1_dev, mscores0_dev, mscores1_dev, stats_dev, as_stream(stream));
  });
}

int imx_ot_match_loss_grad_matches(imx_handle_t h, int B, const float* scores_dev, int N0, int N1, const int32_t* n0_dev, const int32_t* n1_dev,
                                   const float* bin_score_dev, int iters, const int64_t* all_matches_dev, const int32_t* n_all_dev, int L,
                                   const float* gout_dev, float* loss_dev, float* grad_scores_dev, float* grad_bin_dev, int32_t* flag_dev,
                                   float threshold, const int64_t* gt0_dev, int64_t* matches0_dev, int64_t* matches1_dev, float* mscores0_dev,
                                   float* mscores1_dev, int32_t* stats_dev, void* stream) {
  return on_device(h, "imx_ot_match_loss_grad_matches", [&]() -> int {
    const char* who = "imx_ot_match_loss_grad_matches";
    if (check_outputs(h, who, threshold, gt0_dev, matches0_dev, matches1_dev, mscores0_dev, mscores1_dev, stats_dev)) return -1;
    hipStream_t s = as_stream(stream);
    OtArgs a;
    if (ot_loss_grad_sequence(h, who, B, scores_dev, N0, N1, n0_dev, n1_dev, bin_score_dev, iters, all_matches_dev, n_all_dev, L, gout_dev,
                              loss_dev, grad_scores_dev, grad_bin_dev, flag_dev, s, a))
      return -1;
    // u_T and v_T where the sequence left them: slot `iters` of each pair's (iters + 1) rows (written by this call: slot 0 by ot_init)
    const size_t r0 = (size_t)N0 + 1, r1 = (size_t)N1 + 1, T1 = (size_t)iters + 1;
    return extract_matches(h, who, B, scores_dev, N0, N1, n0_dev, n1_dev, a.U + (size_t)iters * r0, T1 * r0, a.V + (size_t)iters * r1, T1 * r1,
                           threshold, gt0_dev, matches0_dev, matches1_dev, mscores0_dev, mscores1_dev, stats_dev, s);
  });
}

}  // extern "C"
