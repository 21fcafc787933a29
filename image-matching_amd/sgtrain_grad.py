"""The SuperGlue training objective as a differentiable torch function whose value AND gradient come from libimx
(include/imx_otgrad.h): the optimal-transport layer and the match loss of the reference's SuperGlue.forward
(superglue/models/superglue_train.py:271-299) under PyTorch-ROCm.  The library supplies the cotangents at the score matrix and at
bin_score, differentiated through the unrolled Sinkhorn as the reference's autograd does; PyTorch runs the backward of the einsum and of
the network.

    scores = torch.einsum('bdn,bdm->bnm', mdesc0, mdesc1) / d ** .5
    loss = match_loss(engine, scores, self.bin_score, all_matches, n_all, iters).mean()
    loss.backward()

Inputs are contiguous fp32 cuda tensors; anything else raises (no silent copy, no CPU path)."""
import torch
from torch.autograd.function import once_differentiable

from .engine import ImxError


def _require(t, what):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.dtype != torch.float32 or not t.is_contiguous():
        raise ImxError(f"{what} must be a contiguous fp32 cuda tensor, got "
                       f"{(t.dtype, t.device.type, t.is_contiguous()) if isinstance(t, torch.Tensor) else type(t).__name__}")


class ot_match_loss(torch.autograd.Function):
    """ot_match_loss.apply(engine, scores, bin_score, all_matches, n_all, iters, n0, n1): log_optimal_transport(scores, bin_score, iters)
    and the mean of -log(exp(Z[x][y])) over each pair's listed (x, y); a (B) device tensor, differentiable with respect to scores
    (B,N0,N1) and bin_score (one element).  all_matches (B,2,L) int64 and n_all (B) int32 as Engine.gt_matches returns them; n0 / n1 (B)
    int32 counts of a padded batch or None.  Where a listed entry's exp underflows the value is +inf and the gradient that of -Z."""

    @staticmethod
    def forward(ctx, engine, scores, bin_score, all_matches, n_all, iters, n0=None, n1=None):
        _require(scores, "ot_match_loss: scores")
        _require(bin_score, "ot_match_loss: bin_score")
        res = engine.ot_match_loss_grad(scores, bin_score, all_matches, n_all, iters, n0=n0, n1=n1)   # gout = NULL: the gradient of each pair's loss
        ctx.save_for_backward(res["grad_scores"], res["grad_bin"])
        ctx.bin_shape = bin_score.shape
        ctx.mark_non_differentiable(res["flag"])
        return res["loss"], res["flag"]

    @staticmethod
    @once_differentiable                                                 # the saved gradients are constants: no second derivative here
    def backward(ctx, grad_loss, _grad_flag):
        gs, gb = ctx.saved_tensors
        need = ctx.needs_input_grad
        return (None, gs * grad_loss.reshape(-1, 1, 1) if need[1] else None,
                (gb * grad_loss.reshape(-1)).sum().reshape(ctx.bin_shape) if need[2] else None, None, None, None, None, None)


def match_loss(engine, scores, bin_score, all_matches, n_all, iters, n0=None, n1=None):
    """The per-pair loss (B) of superglue_train.py:289-299 on scores (B,N0,N1) = einsum(mdesc0, mdesc1) / sqrt(d), replacing lines
    271-299 of the reference's forward; `.backward()` reaches scores and bin_score."""
    return ot_match_loss.apply(engine, scores, bin_score, all_matches, n_all, int(iters), n0, n1)[0]
