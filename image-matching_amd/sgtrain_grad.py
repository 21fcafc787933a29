"""The SuperGlue training objective as a differentiable torch function whose value AND gradient come from libimx
(include/imx_train.h): the optimal-transport layer and the match loss of the reference's SuperGlue.forward
(superglue/models/superglue_train.py:271-299) under PyTorch-ROCm.  The library supplies the cotangents at the score matrix and at
bin_score, differentiated through the unrolled Sinkhorn as the reference's autograd does; PyTorch runs the backward of the einsum and of
the network.

    scores = torch.einsum('bdn,bdm->bnm', mdesc0, mdesc1) / d ** .5
    loss = match_loss(engine, scores, self.bin_score, all_matches, n_all, iters).mean()
    loss.backward()

`match_loss_matches(...)` returns the same loss together with the matches and matching scores the reference's forward reports
(superglue_train.py:276-286), extracted from that same Sinkhorn's final potentials (include/imx_sgloop.h).

The attention of the GNN (superglue_train.py:82-86) is here as well, forward and backward from libimx (include/imx_train.h): inside the
reference's MultiHeadedAttention.forward,

    x, _ = attention(engine, query, key, value)

keeps O(B H N) floats per layer for the backward instead of the (B, H, N, M) probabilities.

The 1x1 convolutions around it (superglue_train.py:52, 96, 97, 111) are here too, forward and backward from libimx
(include/imx_train.h): inside MultiHeadedAttention.forward and MLP,

    y = conv1d(engine, x, conv.weight, conv.bias)                # nn.Conv1d(kernel_size=1)
    y = conv1d(engine, x, conv.weight, conv.bias, x1=message)    # the same on torch.cat([x, message], 1), never formed

and a whole layer of the GNN, `delta0 = attentional_propagation(engine, layer, desc0, src0)` for `layer(desc0, src0)` in
AttentionalGNN.forward: every matrix product in libimx, BatchNorm and ReLU PyTorch's.

BatchNorm1d followed by ReLU (superglue_train.py:55-56, inside every MLP) is here as well, one launch forward and one backward
(include/imx_train.h): `h = batchnorm_relu(engine, bn, h)` for `relu(bn(h))`, `mlp(engine, seq, x)` for a whole Sequential that the
reference's MLP() built, `keypoint_encoder(engine, kenc, kpts, scores)` for `kenc(kpts, scores)`, and `gnn_layer(engine, layer, desc0,
src0, n=n0, ns=n1)` for `layer(desc0, src0)` with everything in libimx -- and with per-pair counts, so a padded batch of pairs with
different keypoint counts goes through a layer: the BatchNorm statistics are those of the valid columns only.

The score product between the two images' projected descriptors (superglue_train.py:267-268) is here too, forward and backward from
libimx_sgtrain (include/imx_sgtrain.h): `scores(engine, mdesc0, mdesc1, n0, n1)` for `torch.einsum('bdn,bdm->bnm', mdesc0, mdesc1) /
descriptor_dim ** .5`, with counts.  With it every matrix product of the training forward is the library's;
sgtrain_model.SuperGlueTrainable composes the whole step.

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


class ot_match_loss_matches(torch.autograd.Function):
    """ot_match_loss_matches.apply(engine, scores, bin_score, all_matches, n_all, iters, threshold, n0, n1, gt0): ot_match_loss with the
    matches of superglue_train.py:276-286 taken from the SAME Sinkhorn (Engine.ot_match_loss_grad_matches, include/imx_sgloop.h).
    Returns (loss (B), flag, matches0, matches1, matching_scores0, matching_scores1, stats): the loss is differentiable with respect to
    scores and bin_score, with the bits and the gradients of ot_match_loss; everything else is marked non-differentiable.  stats (B,3)
    int32 needs gt0 (B,N0) int64; without it an empty (B,0) tensor stands in its place."""

    @staticmethod
    def forward(ctx, engine, scores, bin_score, all_matches, n_all, iters, threshold, n0=None, n1=None, gt0=None):
        _require(scores, "ot_match_loss_matches: scores")
        _require(bin_score, "ot_match_loss_matches: bin_score")
        res = engine.ot_match_loss_grad_matches(scores, bin_score, all_matches, n_all, iters, n0=n0, n1=n1, threshold=threshold, gt0=gt0)
        ctx.save_for_backward(res["grad_scores"], res["grad_bin"])
        ctx.bin_shape = bin_score.shape
        stats = res["stats"] if "stats" in res else torch.empty(scores.shape[0], 0, dtype=torch.int32, device=scores.device)
        extra = (res["flag"], res["matches0"], res["matches1"], res["matching_scores0"], res["matching_scores1"], stats)
        ctx.mark_non_differentiable(*extra)
        return (res["loss"],) + extra

    @staticmethod
    @once_differentiable                                                 # the saved gradients are constants: no second derivative here
    def backward(ctx, grad_loss, *_unused):
        gs, gb = ctx.saved_tensors
        need = ctx.needs_input_grad
        return (None, gs * grad_loss.reshape(-1, 1, 1) if need[1] else None,
                (gb * grad_loss.reshape(-1)).sum().reshape(ctx.bin_shape) if need[2] else None) + (None,) * 7


def match_loss_matches(engine, scores, bin_score, all_matches, n_all, iters, threshold, n0=None, n1=None, gt0=None):
    """match_loss and the reference's matches in one call, one Sinkhorn: (loss (B), {matches0, matches1, matching_scores0,
    matching_scores1[, stats]}).  `.backward()` of the loss reaches scores and bin_score exactly as match_loss's does; the dict's tensors
    require no grad."""
    loss, _flag, m0, m1, ms0, ms1, stats = ot_match_loss_matches.apply(engine, scores, bin_score, all_matches, n_all, int(iters), float(threshold),
                                                                     n0, n1, gt0)
    out = {"matches0": m0, "matches1": m1, "matching_scores0": ms0, "matching_scores1": ms1}
    if gt0 is not None:
        out["stats"] = stats
    return loss, out


class mha(torch.autograd.Function):
    """mha.apply(engine, query, key, value, nq, nk): softmax(query^T key / sqrt(D)) value per (pair, head) on the reference's own
    (B, D, H, N) / (B, D, H, M) tensors, differentiable with respect to query, key and value.  Saved for the backward: query, key, value,
    the output and the row log-sum-exp (B, H, N) -- nothing of size N M; the backward recomputes the probabilities (Engine.mha_backward).
    nq / nk (B) int32 counts of a padded batch or None."""

    @staticmethod
    def forward(ctx, engine, query, key, value, nq=None, nk=None):
        for t, what in ((query, "query"), (key, "key"), (value, "value")):
            _require(t, f"mha: {what}")
        res = engine.mha_forward_train(query, key, value, nq=nq, nk=nk)
        ctx.engine, ctx.nq, ctx.nk = engine, nq, nk
        ctx.save_for_backward(query, key, value, res["out"], res["lse"])
        return res["out"]

    @staticmethod
    @once_differentiable                                                 # the kernels form first derivatives only
    def backward(ctx, grad_out):
        query, key, value, out, lse = ctx.saved_tensors
        need = ctx.needs_input_grad[1:4]
        if not any(need):
            return (None,) * 6
        grad_out = grad_out.contiguous()                                 # (autograd's own tensor: the merge's backward may hand over a view)
        _require(grad_out, "mha: grad_out")
        g = ctx.engine.mha_backward(query, key, value, out, lse, grad_out, nq=ctx.nq, nk=ctx.nk, want=tuple(need))
        return None, g.get("dq"), g.get("dk"), g.get("dv"), None, None


def attention(engine, query, key, value, nq=None, nk=None):
    """attention() of superglue_train.py:82-86 with the engine in front: (x, None), x = einsum('bhnm,bdhm->bdhn', softmax(einsum(
    'bdhn,bdhm->bhnm', query, key) / dim ** .5, dim=-1), value).  The reference returns the probabilities second and discards them at
    its only call site (`x, _ = attention(...)`); they are never formed here, so None stands for them.  `.backward()` reaches query, key
    and value through the library's kernels."""
    return mha.apply(engine, query, key, value, nq, nk), None


class conv1x1(torch.autograd.Function):
    """conv1x1.apply(engine, x, weight, bias, x1, n): F.conv1d(torch.cat([x, x1], 1), weight, bias) of kernel size 1 on x (B,C0,N), x1
    (B,C1,N) or None, weight (Cout, C0+C1, 1) or (Cout, C0+C1), bias (Cout) or None, differentiable with respect to x, weight, bias and
    x1.  Saved for the backward: the inputs only (x, x1, weight).  n (B) int32 counts of a padded batch or None."""

    @staticmethod
    def forward(ctx, engine, x, weight, bias=None, x1=None, n=None):
        for t, what in ((x, "x"), (weight, "weight")) + (((bias, "bias"),) if bias is not None else ()) + (((x1, "x1"),) if x1 is not None else ()):
            _require(t, f"conv1x1: {what}")
        y = engine.conv1x1_forward_train(x, weight, bias, x1=x1, n=n)["y"]
        ctx.engine, ctx.n, ctx.has_x1 = engine, n, x1 is not None
        ctx.save_for_backward(x, weight, *((x1,) if x1 is not None else ()))
        return y

    @staticmethod
    @once_differentiable                                                 # the kernels form first derivatives only
    def backward(ctx, grad_y):
        x, weight = ctx.saved_tensors[:2]
        x1 = ctx.saved_tensors[2] if ctx.has_x1 else None
        need = ctx.needs_input_grad                                      # (engine, x, weight, bias, x1, n)
        want = (need[1], need[4] and ctx.has_x1, need[2], need[3])
        if not any(want):
            return (None,) * 6
        grad_y = grad_y.contiguous()                                     # (autograd's own tensor: it may hand over a view)
        _require(grad_y, "conv1x1: grad_y")
        g = ctx.engine.conv1x1_backward(x, weight, grad_y, x1=x1, n=ctx.n, want=want)
        return None, g.get("dx0"), g.get("dw"), g.get("db"), g.get("dx1"), None


def conv1d(engine, x, weight, bias=None, x1=None, n=None):
    """F.conv1d(torch.cat([x, x1], 1), weight, bias) for a weight of kernel size 1, without forming the cat; x1 = None is
    F.conv1d(x, weight, bias), what nn.Conv1d(kernel_size=1) computes.  `.backward()` reaches x, x1, weight and bias through the
    library's kernels.  n (B) int32: columns past n[b] are not read and come out as 0."""
    return conv1x1.apply(engine, x, weight, bias, x1, n)


def attentional_propagation(engine, layer, x, source):
    """AttentionalPropagation.forward (superglue_train.py:99-116) on any module with .attn.proj, .attn.merge, .attn.dim,
    .attn.num_heads and .mlp (Conv1d, BatchNorm1d, ReLU, Conv1d): `layer(x, source)` with the six convolutions through conv1d (mlp.0
    takes x1 = message, so torch.cat([x, message], 1) is never formed) and the attention through attention().  layer.mlp[1]
    (BatchNorm1d, in whatever mode the module is in; PyTorch updates its running statistics as usual) and layer.mlp[2] are called as
    they are.  Full frames only, no counts: BatchNorm's batch statistics would count the padding of a ragged batch."""
    attn, mlp = layer.attn, layer.mlp
    b = x.size(0)
    query, key, value = [conv1d(engine, t, l.weight, l.bias).view(b, attn.dim, attn.num_heads, -1)
                         for l, t in zip(attn.proj, (x, source, source))]
    m, _ = attention(engine, query, key, value)
    message = conv1d(engine, m.view(b, attn.dim * attn.num_heads, -1), attn.merge.weight, attn.merge.bias)
    h = mlp[2](mlp[1](conv1d(engine, x, mlp[0].weight, mlp[0].bias, x1=message)))
    return conv1d(engine, h.contiguous(), mlp[3].weight, mlp[3].bias)


class bn_relu(torch.autograd.Function):
    """bn_relu.apply(engine, x, gamma, beta, running_mean, running_var, num_batches_tracked, n, training, momentum, eps):
    F.relu(F.batch_norm(x, running_mean, running_var, gamma, beta, training, momentum, eps)) on x (B,C,N), differentiable with respect to
    x, gamma and beta.  Saved for the backward: x, gamma, beta and the (C) mean and rstd only -- neither the BatchNorm output nor the ReLU
    output; the backward recomputes the mask.  The running statistics are updated in place in training mode.  n (B) int32 counts of a
    padded batch or None."""

    @staticmethod
    def forward(ctx, engine, x, gamma, beta, running_mean=None, running_var=None, num_batches_tracked=None, n=None, training=True,
                momentum=0.1, eps=1e-5):
        for t, what in ((x, "x"), (gamma, "gamma"), (beta, "beta")):
            _require(t, f"bn_relu: {what}")
        res = engine.bn_relu_forward_train(x, gamma, beta, running_mean, running_var, num_batches_tracked, n=n, training=training,
                                           momentum=momentum, eps=eps)
        ctx.engine, ctx.n, ctx.training = engine, n, bool(training)
        ctx.save_for_backward(x, gamma, beta, res["mean"], res["rstd"])
        return res["y"]

    @staticmethod
    @once_differentiable                                                 # the kernel forms first derivatives only
    def backward(ctx, grad_y):
        x, gamma, beta, mean, rstd = ctx.saved_tensors
        want = tuple(ctx.needs_input_grad[1:4])
        if not any(want):
            return (None,) * 11
        grad_y = grad_y.contiguous()                                     # (autograd's own tensor: it may hand over a view)
        _require(grad_y, "bn_relu: grad_y")
        g = ctx.engine.bn_relu_backward(x, gamma, beta, mean, rstd, grad_y, n=ctx.n, training=ctx.training, want=want)
        return (None, g.get("dx"), g.get("dgamma"), g.get("dbeta")) + (None,) * 7


def batchnorm_relu(engine, bn, x, n=None):
    """F.relu(bn(x)) for an nn.BatchNorm1d module bn on x (B,C,N): bn.training, bn.eps and bn.momentum are honoured, and in training mode
    bn.running_mean, bn.running_var and bn.num_batches_tracked are updated in place, as the module's own forward does.  momentum = None
    (the cumulative average), affine = False and track_running_stats = False are not built: ImxError.  n (B) int32: columns past n[b]
    are not read, come out as 0 and do not enter the statistics."""
    if not isinstance(bn, torch.nn.BatchNorm1d):
        raise ImxError(f"batchnorm_relu: bn must be an nn.BatchNorm1d, got {type(bn).__name__}")
    if bn.momentum is None or not bn.affine or not bn.track_running_stats:
        raise ImxError("batchnorm_relu: momentum=None, affine=False and track_running_stats=False are not supported")
    return bn_relu.apply(engine, x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, n, bn.training,
                         float(bn.momentum), float(bn.eps))


def _is_conv1(m):
    return isinstance(m, torch.nn.Conv1d) and m.kernel_size == (1,) and m.stride == (1,) and m.padding == (0,) and m.groups == 1


class _bias_before_batchnorm(torch.autograd.Function):
    """_bias_before_batchnorm.apply(h, bias) -> h, for h = conv1d(..., bias.detach(), ...) that feeds a BatchNorm1d in training mode.
    Such a bias has a gradient of exactly 0: it shifts every valid column of its channel alike, the batch mean takes the shift out
    again, and the gradient is sum_n dx[c,n] over the BatchNorm's input gradient, whose terms cancel identically (sum xhat = 0 and
    dbeta / M is the mean of g; with counts the sums run over the valid columns, and with M <= 1 dx is 0).  Forming that sum in fp32
    returns the rounding residue of terms that can be hundreds; this returns the 0 itself and no kernel runs for it."""

    @staticmethod
    def forward(ctx, h, bias):
        ctx.like = bias
        return h.view_as(h)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_h):
        return grad_h, torch.zeros_like(ctx.like) if ctx.needs_input_grad[1] else None


def mlp(engine, seq, x, x1=None, n=None):
    """seq(torch.cat([x, x1], 1)) for any nn.Sequential that the reference's MLP() builds (superglue_train.py:46-57: Conv1d [BatchNorm1d
    ReLU] ... Conv1d, kernel size 1): the convolutions through conv1d (the first takes x1, so the cat is never formed), every BatchNorm1d
    + ReLU through batchnorm_relu.  The bias of a convolution whose BatchNorm is in training mode gets its exact gradient, 0
    (_bias_before_batchnorm); in evaluation mode it is formed like any other.  Any other layout raises ImxError.  n (B) int32 counts of
    a padded batch or None."""
    mods = list(seq)
    if len(mods) % 3 != 1 or not all(_is_conv1(m) for m in mods[0::3]) or not all(isinstance(m, torch.nn.BatchNorm1d) for m in mods[1::3]) \
            or not all(isinstance(m, torch.nn.ReLU) for m in mods[2::3]):
        raise ImxError("mlp: expected Conv1d(kernel_size=1) [BatchNorm1d ReLU Conv1d(kernel_size=1)] ..., got "
                       + " ".join(type(m).__name__ for m in mods))
    h = x
    for i in range(0, len(mods), 3):
        conv, bias = mods[i], mods[i].bias
        cancels = bias is not None and i + 1 < len(mods) and mods[i + 1].training
        h = conv1d(engine, h, conv.weight, bias.detach() if cancels else bias, x1=x1 if i == 0 else None, n=n)
        if cancels:
            h = _bias_before_batchnorm.apply(h, bias)
        if i + 1 < len(mods):
            h = batchnorm_relu(engine, mods[i + 1], h, n=n)
    return h


def keypoint_encoder(engine, kenc, kpts, scores, n=None):
    """KeypointEncoder.forward (superglue_train.py:77-79) on kpts (B,N,2) and scores (B,N): kenc.encoder through mlp(), the cat of the
    transposed keypoints and the scores formed by conv1d's second source."""
    return mlp(engine, kenc.encoder, kpts.transpose(1, 2).contiguous(), x1=scores.unsqueeze(1).contiguous(), n=n)


def gnn_layer(engine, layer, x, source, n=None, ns=None):
    """AttentionalPropagation.forward (superglue_train.py:114-116) with everything in libimx: the six convolutions through conv1d, the
    attention through attention(), BatchNorm1d + ReLU through batchnorm_relu (the module's mode, momentum and eps; its buffers are updated
    in place).  n / ns (B) int32 counts of x's and source's columns in a padded batch, or None: they reach the convolutions, the attention
    (nq = n, nk = ns) and the BatchNorm, whose statistics are those of the valid columns of all pairs."""
    attn = layer.attn
    b = x.size(0)
    query, key, value = [conv1d(engine, t, l.weight, l.bias, n=c).view(b, attn.dim, attn.num_heads, -1)
                         for l, t, c in zip(attn.proj, (x, source, source), (n, ns, ns))]
    m, _ = attention(engine, query, key, value, nq=n, nk=ns)
    message = conv1d(engine, m.view(b, attn.dim * attn.num_heads, -1), attn.merge.weight, attn.merge.bias, n=n)
    return mlp(engine, layer.mlp, x, x1=message, n=n)


class score_product(torch.autograd.Function):
    """score_product.apply(engine, mdesc0, mdesc1, n0, n1): torch.einsum('bdn,bdm->bnm', mdesc0, mdesc1) / D ** .5 on mdesc0 (B,D,N0)
    and mdesc1 (B,D,N1), differentiable with respect to both.  Saved for the backward: mdesc0 and mdesc1 only.  n0 / n1 (B) int32 counts
    of a padded batch or None."""

    @staticmethod
    def forward(ctx, engine, mdesc0, mdesc1, n0=None, n1=None):
        for t, what in ((mdesc0, "mdesc0"), (mdesc1, "mdesc1")):
            _require(t, f"score_product: {what}")
        s = engine.score_product_forward_train(mdesc0, mdesc1, n0=n0, n1=n1)["scores"]
        ctx.engine, ctx.n0, ctx.n1 = engine, n0, n1
        ctx.save_for_backward(mdesc0, mdesc1)
        return s

    @staticmethod
    @once_differentiable                                                 # the kernels form first derivatives only
    def backward(ctx, grad_scores):
        mdesc0, mdesc1 = ctx.saved_tensors
        want = tuple(ctx.needs_input_grad[1:3])
        if not any(want):
            return (None,) * 5
        grad_scores = grad_scores.contiguous()                           # (autograd's own tensor: it may hand over a view)
        _require(grad_scores, "score_product: grad_scores")
        g = ctx.engine.score_product_backward(mdesc0, mdesc1, grad_scores, n0=ctx.n0, n1=ctx.n1, want=want)
        return None, g.get("da"), g.get("db"), None, None


def scores(engine, mdesc0, mdesc1, n0=None, n1=None):
    """torch.einsum('bdn,bdm->bnm', mdesc0, mdesc1) / descriptor_dim ** .5 of superglue_train.py:267-268; `.backward()` reaches mdesc0
    and mdesc1 through the library's kernels.  n0 / n1 (B) int32: rows past n0[b] and columns past n1[b] are not read and come out as
    0."""
    return score_product.apply(engine, mdesc0, mdesc1, n0, n1)
