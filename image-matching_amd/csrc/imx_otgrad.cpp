// imx_otgrad.cpp -- a host unit of libimx_train.so (include/imx_train.h), on the handle libimx.so made: the SuperGlue match loss
// through the unrolled Sinkhorn as one value-and-gradient call.  The kernels are otgrad.hip's; the forward's Sinkhorn and match kernels
// (sg_misc.hip, trainpairs.hip) are not linked here and not touched.  Every scratch buffer ("otg.*") is written, as far as it is
// read, by the call that reads it: 2 (iters + 1) (N0 + N1 + 2) floats per pair and a few vectors, nothing of matrix size.  The checks,
// the workspaces and the launch sequence are otgrad_seq.h's, which libimx_sgloop.so's fused call runs as well.
#include "imx_host.h"
#include "otgrad_seq.h"
#include "../../include/imx_train.h"

extern "C" {

int imx_ot_match_loss_grad(imx_handle_t h, int B, const float* scores_dev, int N0, int N1, const int32_t* n0_dev, const int32_t* n1_dev,
                           const float* bin_score_dev, int iters, const int64_t* all_matches_dev, const int32_t* n_all_dev, int L,
                           const float* gout_dev, float* loss_dev, float* grad_scores_dev, float* grad_bin_dev, int32_t* flag_dev,
                           void* stream) {
  return on_device(h, "imx_ot_match_loss_grad", [&]() -> int {
    OtArgs a;
    return ot_loss_grad_sequence(h, "imx_ot_match_loss_grad", B, scores_dev, N0, N1, n0_dev, n1_dev, bin_score_dev, iters, all_matches_dev,
                                 n_all_dev, L, gout_dev, loss_dev, grad_scores_dev, grad_bin_dev, flag_dev, as_stream(stream), a);
  });
}

}  // extern "C"
