// otgrad_seq.h -- the launch sequence of the SuperGlue match loss through the unrolled Sinkhorn (otgrad.hip), shared by the two host
// units that run it: imx_otgrad.cpp (libimx_train.so: imx_ot_match_loss_grad) and imx_sgloop.cpp (libimx_sgloop.so:
// imx_ot_match_loss_grad_matches, which goes on to extract the matches from the final potentials).  One definition, inlined at both
// calls, so the two sequences cannot drift: the same checks, the same workspaces ("otg.*"), the same launches in the same order.
#pragma once
#include "imx_host.h"
#include "otgrad.h"

namespace imx::host {

// Checks the arguments, draws the workspaces and enqueues the whole sequence on s.  On success `a` holds what was launched: a.U / a.V
// are (B, iters+1, N0+1) / (B, iters+1, N1+1), the final potentials in slot `iters`.  `who` names the entry point in error texts.
inline int ot_loss_grad_sequence(imx_handle_t h, const char* who, int B, const float* scores_dev, int N0, int N1, const int32_t* n0_dev,
                                 const int32_t* n1_dev, const float* bin_score_dev, int iters, const int64_t* all_matches_dev,
                                 const int32_t* n_all_dev, int L, const float* gout_dev, float* loss_dev, float* grad_scores_dev,
                                 float* grad_bin_dev, int32_t* flag_dev, hipStream_t s, OtArgs& a) {
  if (B < 1 || B > 65535 || N0 < 1 || N1 < 1 || N0 > (1 << 20) || N1 > (1 << 20) || L < 0 || iters < 0 || iters > 4096)
    return fail(h, "%s: bad shape B=%d N0=%d N1=%d L=%d iters=%d (B in [1,65535], N0 N1 in [1,2^20], L >= 0, iters in [0,4096])", who,
                B, N0, N1, L, iters);
  if (!scores_dev || !bin_score_dev || !n_all_dev || !loss_dev || (L && !all_matches_dev) || (grad_scores_dev && !grad_bin_dev))
    return fail(h, "%s: null argument", who);
  const size_t T1 = (size_t)iters + 1, r0 = (size_t)N0 + 1, r1 = (size_t)N1 + 1;
  a = OtArgs{};
  a.scores = scores_dev; a.n0 = n0_dev; a.n1 = n1_dev; a.bin = bin_score_dev; a.B = B; a.N0 = N0; a.N1 = N1; a.T = iters;
  a.all_matches = reinterpret_cast<const long long*>(all_matches_dev); a.n_all = n_all_dev; a.L = L; a.gout = gout_dev;
  a.loss = loss_dev; a.grad = grad_scores_dev; a.grad_bin = grad_bin_dev; a.flag = flag_dev;
  WS(U, float, "otg.u", B * T1 * r0 * sizeof(float));
  WS(V, float, "otg.v", B * T1 * r1 * sizeof(float));
  a.U = U; a.V = V;
  if (a.grad) {
    WS(UB, float, "otg.u_bar", B * T1 * r0 * sizeof(float));
    WS(VB, float, "otg.v_bar", B * T1 * r1 * sizeof(float));
    WS(cnt, int, "otg.counts", (size_t)B * (2 * (r0 + r1) - 1) * sizeof(int));
    WS(binv, float, "otg.bin_terms", (size_t)B * (r0 + r1 - 1) * sizeof(float));
    a.UB = UB; a.VB = VB; a.cnt_row = cnt; a.cnt_col = cnt + B * r0; a.cnt_bin = cnt + B * (r0 + r1); a.binv = binv;
  }
  RUN("ot_init", launch_ot_init(a, s));
  for (int t = 1; t <= iters; ++t) {
    RUN("ot_row_lse", launch_ot_row_lse(a, t, s));
    RUN("ot_col_lse", launch_ot_col_lse(a, t, s));
  }
  RUN("ot_gather", launch_ot_gather(a, s));
  if (!a.grad) return 0;
  if (iters > 0) RUN("ot_seed", launch_ot_seed(a, s));
  for (int t = iters; t >= 1; --t) {
    RUN("ot_row_bwd", launch_ot_row_bwd(a, t, s));
    RUN("ot_col_bwd", launch_ot_col_bwd(a, t, s));
  }
  RUN("ot_assemble", launch_ot_assemble(a, s));
  RUN("ot_bin", launch_ot_bin(a, s));
  return 0;
}

}  // namespace imx::host
