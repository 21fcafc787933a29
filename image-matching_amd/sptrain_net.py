"""SuperPoint's own layers in their training form, with `loss.backward()` running through the project's kernels: the 3x3 convolutions
of libimx_spnet (include/imx_spnet.h, csrc/conv3_train.hip), the BatchNorm2d [+ ReLU] of libimx_spnorm
(include/imx_spnorm.h, csrc/bn2d_train.hip; section 19) and the max-pooling and descriptor normalisation of libimx_sppool
(include/imx_sppool.h, csrc/sppool_train.hip; section 20) as torch.autograd.Functions, and on them the reference's `double_conv` and `down`
blocks (superpoint/models/unet_parts.py:10-48) and the two-layer heads of its network (superpoint/models/superpoint_train.py:47-54).

    conv3x3.apply(engine, x, weight, bias)      F.conv2d(x, weight, bias, padding=1) for a (Cout,Cin,3,3) weight
    conv2d(engine, x, weight, bias)             the same, as a function
    bn2d.apply(engine, x, gamma, beta, ...)     F.batch_norm on (B,C,H,W), followed by F.relu when asked
    batchnorm2d(engine, bn, x, relu=False)      bn(x) for an nn.BatchNorm2d, F.relu(bn(x)) with relu=True
    conv_bn_relu(engine, conv, bn, x)           F.relu(bn(conv(x))) for nn.Conv2d(.., 3, padding=1) and nn.BatchNorm2d
    double_conv(engine, block, x)               block(x) for the reference's double_conv
    down(engine, block, x)                      block(x) for the reference's down (nn.MaxPool2d(2) stays F.max_pool2d)
    conv_bn_relu_form / double_conv_form / down_form (..., form="auto")    the same three with the BatchNorm form chosen by the caller
    head(engine, conv_a, bn_a, conv_b, bn_b, x) bn_b(conv_b(relu(bn_a(conv_a(x))))), conv_a 3x3 and conv_b 1x1
    maxpool2.apply(engine, x)                   F.max_pool2d(x, 2); saved for the backward: one index byte per output
    max_pool2(engine, x)                        the same, as a function
    l2norm.apply(engine, x)                     x / torch.norm(x, p=2, dim=1, keepdim=True); saved: the output and the norms
    normalize_descriptors(engine, x)            the same, as a function
    down_pooled(engine, block, x, form="auto")  down_form with the max-pooling on libimx_sppool's kernels

Tensors are the reference's own, NCHW contiguous fp32 on the engine's device; nothing is copied to another layout.  BatchNorm + ReLU has
two forms.  "channel": the kernels of libimx_train (sgtrain_grad.bn_relu) on the (B, C, H W) view, one workgroup per channel, bound to
H W <= 2^20.  "pixels": libimx_spnorm's, the work split over slabs of 4096 pixels, H W <= 2^24 and B H W < 2^31.  "auto" chooses by
pixels_form(B, C, H W), a rule on the shape alone.  conv2d alone serves H, W <= 4096.  down / down_form keep F.max_pool2d; down_pooled
pools through max_pool2.  The network assembled from these with live parameters is sptrain_model.SuperPointTrainable."""
import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from .engine import ImxError
from .sgtrain_grad import _bias_before_batchnorm, _require, bn_relu, conv1d


class conv3x3(torch.autograd.Function):
    """conv3x3.apply(engine, x, weight, bias): F.conv2d(x, weight, bias, padding=1) on x (B,Cin,H,W), weight (Cout,Cin,3,3), bias (Cout)
    or None, differentiable with respect to x, weight and bias.  Saved for the backward: x and weight only."""

    @staticmethod
    def forward(ctx, engine, x, weight, bias=None):
        for t, what in ((x, "x"), (weight, "weight")) + (((bias, "bias"),) if bias is not None else ()):
            _require(t, f"conv3x3: {what}")
        y = engine.conv3x3_forward_train(x, weight, bias)["y"]
        ctx.engine = engine
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    @once_differentiable                                                 # the kernels form first derivatives only
    def backward(ctx, grad_y):
        x, weight = ctx.saved_tensors
        want = tuple(ctx.needs_input_grad[1:4])                          # (engine, x, weight, bias)
        if not any(want):
            return (None,) * 4
        grad_y = grad_y.contiguous()                                     # (autograd's own tensor: it may hand over a view)
        _require(grad_y, "conv3x3: grad_y")
        g = ctx.engine.conv3x3_backward(x, weight, grad_y, want=want)
        return None, g.get("dx"), g.get("dw"), g.get("db")


def conv2d(engine, x, weight, bias=None):
    """F.conv2d(x, weight, bias, padding=1) for a weight of kernel size 3 x 3, what nn.Conv2d(Cin, Cout, 3, padding=1) computes.
    `.backward()` reaches x, weight and bias through the library's kernels; an input that needs no gradient (the image of the first
    layer) costs no kernel."""
    return conv3x3.apply(engine, x, weight, bias)


def _is_conv3(m):
    return (isinstance(m, torch.nn.Conv2d) and m.kernel_size == (3, 3) and m.stride == (1, 1) and m.padding == (1, 1) and m.dilation == (1, 1)
            and m.groups == 1 and m.padding_mode == "zeros")


class bn2d(torch.autograd.Function):
    """bn2d.apply(engine, x, gamma, beta, running_mean, running_var, num_batches_tracked, relu, training, momentum, eps):
    F.batch_norm(x, running_mean, running_var, gamma, beta, training, momentum, eps) on x (B,C,H,W), followed by F.relu when `relu`,
    differentiable with respect to x, gamma and beta.  Saved for the backward: x, gamma, beta and the (C) mean and rstd only -- neither the
    BatchNorm output nor the ReLU output; the backward recomputes the mask.  The running statistics are updated in place in training mode."""

    @staticmethod
    def forward(ctx, engine, x, gamma, beta, running_mean=None, running_var=None, num_batches_tracked=None, relu=True, training=True,
                momentum=0.1, eps=1e-5):
        for t, what in ((x, "x"), (gamma, "gamma"), (beta, "beta")):
            _require(t, f"bn2d: {what}")
        res = engine.bn2d_forward_train(x, gamma, beta, running_mean, running_var, num_batches_tracked, relu=relu, training=training,
                                        momentum=momentum, eps=eps)
        ctx.engine, ctx.relu, ctx.training = engine, bool(relu), bool(training)
        ctx.save_for_backward(x, gamma, beta, res["mean"], res["rstd"])
        return res["y"]

    @staticmethod
    @once_differentiable                                                 # the kernels form first derivatives only
    def backward(ctx, grad_y):
        x, gamma, beta, mean, rstd = ctx.saved_tensors
        want = tuple(ctx.needs_input_grad[1:4])
        if not any(want):
            return (None,) * 11
        grad_y = grad_y.contiguous()                                     # (autograd's own tensor: it may hand over a view)
        _require(grad_y, "bn2d: grad_y")
        g = ctx.engine.bn2d_backward(x, gamma, beta, mean, rstd, grad_y, relu=ctx.relu, training=ctx.training, want=want)
        return (None, g.get("dx"), g.get("dgamma"), g.get("dbeta")) + (None,) * 7


def _check_bn2d(who, bn, channels=None):
    if not isinstance(bn, torch.nn.BatchNorm2d) or (channels is not None and bn.num_features != channels):
        raise ImxError(f"{who}: bn must be nn.BatchNorm2d({'C' if channels is None else channels}), got {bn!r}")
    if bn.momentum is None or not bn.affine or not bn.track_running_stats:
        raise ImxError(f"{who}: momentum=None, affine=False and track_running_stats=False are not supported")


def batchnorm2d(engine, bn, x, relu=False):
    """bn(x) for an nn.BatchNorm2d module bn on x (B,C,H,W), F.relu(bn(x)) with relu=True, through libimx_spnorm's kernels: bn.training,
    bn.eps and bn.momentum are honoured, and in training mode bn.running_mean, bn.running_var and bn.num_batches_tracked are updated in
    place, as the module's own forward does.  momentum = None (the cumulative average), affine = False and track_running_stats = False
    are not built: ImxError."""
    _check_bn2d("batchnorm2d", bn)
    return bn2d.apply(engine, x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, bool(relu), bn.training,
                      float(bn.momentum), float(bn.eps))


# "auto": the smallest B H W from which the "pixels" kernels were at least as fast as the "channel" kernels at every measured channel
# count (profiles/bn2d_time.json); never below 4096, so that the small blocks keep the "channel" path and its bits
PIXELS_FROM = 9600


def pixels_form(B, C, HW):
    """the rule of form="auto": a function of the shape alone, never of the device"""
    return B * HW >= max(PIXELS_FROM, 4096)


def conv_bn_relu_form(engine, conv, bn, x, form="auto"):
    """F.relu(bn(conv(x))) for conv = nn.Conv2d(Cin, Cout, 3, padding=1) and bn = nn.BatchNorm2d(Cout): the convolution through conv2d,
    BatchNorm + ReLU through form "channel" (sgtrain_grad.bn_relu on the (B, Cout, H W) view of the same memory, H W <= 2^20), "pixels"
    (bn2d, the work split over pixels) or "auto" (pixels_form(B, Cout, H W) decides).  bn.training, bn.eps and bn.momentum are honoured,
    and in training mode bn.running_mean, bn.running_var and bn.num_batches_tracked are updated in place, as the module's own forward
    does.  The bias of the convolution gets its exact gradient in training mode, 0 (sgtrain_grad._bias_before_batchnorm); in evaluation
    mode it is formed like any other.  Any other layout raises ImxError."""
    if form not in ("auto", "channel", "pixels"):
        raise ImxError(f"conv_bn_relu_form: form must be 'auto', 'channel' or 'pixels', got {form!r}")
    if not _is_conv3(conv):
        raise ImxError(f"conv_bn_relu: conv must be nn.Conv2d(Cin, Cout, 3, padding=1) with stride 1, no dilation and no groups, got {conv!r}")
    _check_bn2d("conv_bn_relu", bn, conv.out_channels)
    bias = conv.bias
    cancels = bias is not None and bn.training
    h = conv2d(engine, x, conv.weight, bias.detach() if cancels else bias)
    if cancels:
        h = _bias_before_batchnorm.apply(h, bias)
    B, C, H, W = h.shape
    if form == "pixels" or (form == "auto" and pixels_form(B, C, H * W)):
        return batchnorm2d(engine, bn, h, relu=True)
    y = bn_relu.apply(engine, h.view(B, C, H * W), bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, None,
                      bn.training, float(bn.momentum), float(bn.eps))
    return y.view(B, C, H, W)


def conv_bn_relu(engine, conv, bn, x):
    """conv_bn_relu_form(engine, conv, bn, x, form="auto"): F.relu(bn(conv(x))) for conv = nn.Conv2d(Cin, Cout, 3, padding=1) and bn =
    nn.BatchNorm2d(Cout), BatchNorm + ReLU in the form that pixels_form(B, Cout, H W) chooses.  Below B H W = 4096 that is always the
    "channel" form, which is bound to H W <= 2^20; from PIXELS_FROM on it is the "pixels" form (H W <= 2^24)."""
    return conv_bn_relu_form(engine, conv, bn, x, "auto")


def double_conv_form(engine, block, x, form="auto"):
    """block(x) for the reference's double_conv (unet_parts.py:10-25): block.conv = Sequential(Conv2d, BatchNorm2d, ReLU, Conv2d,
    BatchNorm2d, ReLU), both convolutions 3 x 3 with padding 1; `form` as in conv_bn_relu_form.  Any other layout raises ImxError."""
    seq = getattr(block, "conv", None)
    mods = list(seq) if isinstance(seq, torch.nn.Sequential) else []
    if len(mods) != 6 or not all(_is_conv3(m) for m in mods[0::3]) or not all(isinstance(m, torch.nn.BatchNorm2d) for m in mods[1::3]) \
            or not all(isinstance(m, torch.nn.ReLU) for m in mods[2::3]):
        raise ImxError("double_conv: expected .conv = Sequential(Conv2d(3, padding=1), BatchNorm2d, ReLU, Conv2d(3, padding=1), BatchNorm2d, ReLU), got "
                       + (" ".join(type(m).__name__ for m in mods) if mods else type(block).__name__))
    return conv_bn_relu_form(engine, mods[3], mods[4], conv_bn_relu_form(engine, mods[0], mods[1], x, form), form)


def double_conv(engine, block, x):
    """double_conv_form(engine, block, x, form="auto")"""
    return double_conv_form(engine, block, x, "auto")


def down_form(engine, block, x, form="auto"):
    """block(x) for the reference's down (unet_parts.py:38-48): block.mpconv = Sequential(MaxPool2d(2), double_conv).  The max-pooling
    is F.max_pool2d, forward and backward; the double_conv runs through double_conv_form(); `form` as in conv_bn_relu_form.  Any other
    layout raises ImxError."""
    seq = getattr(block, "mpconv", None)
    mods = list(seq) if isinstance(seq, torch.nn.Sequential) else []
    if len(mods) != 2 or not isinstance(mods[0], torch.nn.MaxPool2d) or mods[0].kernel_size not in (2, (2, 2)) \
            or mods[0].stride not in (2, (2, 2)) or mods[0].padding not in (0, (0, 0)) or mods[0].dilation not in (1, (1, 1)) \
            or mods[0].ceil_mode or mods[0].return_indices:
        raise ImxError("down: expected .mpconv = Sequential(MaxPool2d(2), double_conv), got "
                       + (" ".join(type(m).__name__ for m in mods) if mods else type(block).__name__))
    return double_conv_form(engine, mods[1], F.max_pool2d(x, 2).contiguous(), form)


def down(engine, block, x):
    """down_form(engine, block, x, form="auto")"""
    return down_form(engine, block, x, "auto")


def _is_conv1x1(m):
    return (isinstance(m, torch.nn.Conv2d) and m.kernel_size == (1, 1) and m.stride == (1, 1) and m.padding == (0, 0) and m.dilation == (1, 1)
            and m.groups == 1)


def head(engine, conv_a, bn_a, conv_b, bn_b, x):
    """bn_b(conv_b(relu(bn_a(conv_a(x))))), the arrangement of both heads of the reference's network (superpoint_train.py:47-48: convPa,
    bnPa, convPb, bnPb; :50-51: convDa, bnDa, convDb, bnDb): conv_a = nn.Conv2d(Cin, Cmid, 3, padding=1) with bn_a through conv_bn_relu,
    conv_b = nn.Conv2d(Cmid, Cout, 1) through sgtrain_grad.conv1d on the (B, Cmid, H W) view, bn_b = nn.BatchNorm2d(Cout) without ReLU
    through batchnorm2d.  Both convolution biases get their exact gradient, 0, when their BatchNorm trains.  Any other layout raises
    ImxError."""
    if not _is_conv1x1(conv_b) or not _is_conv3(conv_a) or conv_b.in_channels != conv_a.out_channels:
        raise ImxError(f"head: expected nn.Conv2d(Cin, Cmid, 3, padding=1) and nn.Conv2d(Cmid, Cout, 1), got {conv_a!r} and {conv_b!r}")
    _check_bn2d("head", bn_b, conv_b.out_channels)
    h = conv_bn_relu(engine, conv_a, bn_a, x)
    B, C, H, W = h.shape
    bias = conv_b.bias
    cancels = bias is not None and bn_b.training
    z = conv1d(engine, h.view(B, C, H * W), conv_b.weight.view(conv_b.out_channels, C, 1), bias.detach() if cancels else bias)
    if cancels:
        z = _bias_before_batchnorm.apply(z, bias)
    return batchnorm2d(engine, bn_b, z.view(B, conv_b.out_channels, H, W), relu=False)


class maxpool2(torch.autograd.Function):
    """maxpool2.apply(engine, x): F.max_pool2d(x, 2) on x (B,C,H,W) -- kernel 2, stride 2, no padding, floor -- with PyTorch's tie and
    NaN rule, differentiable with respect to x.  Saved for the backward: idx only, one byte per output; neither x nor y."""

    @staticmethod
    def forward(ctx, engine, x):
        _require(x, "maxpool2: x")
        res = engine.maxpool2_forward_train(x, want_idx=bool(ctx.needs_input_grad[1]))
        ctx.engine, ctx.shape = engine, tuple(x.shape)
        if res["idx"] is not None:
            ctx.save_for_backward(res["idx"])
        return res["y"]

    @staticmethod
    @once_differentiable                                                 # the kernels form first derivatives only
    def backward(ctx, grad_y):
        if not ctx.needs_input_grad[1]:
            return None, None
        idx, = ctx.saved_tensors
        grad_y = grad_y.contiguous()                                     # (autograd's own tensor: it may hand over a view)
        _require(grad_y, "maxpool2: grad_y")
        return None, ctx.engine.maxpool2_backward(idx, grad_y, ctx.shape)["dx"]


def max_pool2(engine, x):
    """F.max_pool2d(x, 2), what nn.MaxPool2d(2) computes, through libimx_sppool's kernels; an input that needs no gradient records no
    indices."""
    return maxpool2.apply(engine, x)


class l2norm(torch.autograd.Function):
    """l2norm.apply(engine, x): x / torch.norm(x, p=2, dim=1, keepdim=True) on x (B,C,H,W) or (B,C,N), a true division without epsilon
    (superpoint_train.py:53-54), differentiable with respect to x.  Saved for the backward: y and norm; not x."""

    @staticmethod
    def forward(ctx, engine, x):
        _require(x, "l2norm: x")
        res = engine.l2norm_forward_train(x)
        ctx.engine = engine
        ctx.save_for_backward(res["y"], res["norm"])
        return res["y"]

    @staticmethod
    @once_differentiable                                                 # the kernels form first derivatives only
    def backward(ctx, grad_y):
        if not ctx.needs_input_grad[1]:
            return None, None
        y, norm = ctx.saved_tensors
        grad_y = grad_y.contiguous()                                     # (autograd's own tensor: it may hand over a view)
        _require(grad_y, "l2norm: grad_y")
        return None, ctx.engine.l2norm_backward(y, norm, grad_y)["dx"]


def normalize_descriptors(engine, x):
    """desc.div(torch.unsqueeze(torch.norm(desc, p=2, dim=1), 1)) (superpoint_train.py:53-54) through libimx_sppool's kernels"""
    return l2norm.apply(engine, x)


def _double_conv_layers(block):
    """the six modules of the reference's double_conv, or ImxError.  A COPY of the layout check inside double_conv_form, for a caller that
    has work to do before that function runs: whoever changes one changes the other (double_conv_form keeps its own because this
    change only adds to the module; having it call this helper is the tidy form)"""
    seq = getattr(block, "conv", None)
    mods = list(seq) if isinstance(seq, torch.nn.Sequential) else []
    if len(mods) != 6 or not all(_is_conv3(m) for m in mods[0::3]) or not all(isinstance(m, torch.nn.BatchNorm2d) for m in mods[1::3]) \
            or not all(isinstance(m, torch.nn.ReLU) for m in mods[2::3]):
        raise ImxError("double_conv: expected .conv = Sequential(Conv2d(3, padding=1), BatchNorm2d, ReLU, Conv2d(3, padding=1), BatchNorm2d, ReLU), got "
                       + (" ".join(type(m).__name__ for m in mods) if mods else type(block).__name__))
    return mods


def down_pooled(engine, block, x, form="auto"):
    """down_form(engine, block, x, form) with the max-pooling through max_pool2 instead of F.max_pool2d: block(x) for the reference's
    down (unet_parts.py:38-48), block.mpconv = Sequential(MaxPool2d(2), double_conv).  Any other layout raises ImxError."""
    seq = getattr(block, "mpconv", None)
    mods = list(seq) if isinstance(seq, torch.nn.Sequential) else []
    if len(mods) != 2 or not isinstance(mods[0], torch.nn.MaxPool2d) or mods[0].kernel_size not in (2, (2, 2)) \
            or mods[0].stride not in (2, (2, 2)) or mods[0].padding not in (0, (0, 0)) or mods[0].dilation not in (1, (1, 1)) \
            or mods[0].ceil_mode or mods[0].return_indices:
        raise ImxError("down: expected .mpconv = Sequential(MaxPool2d(2), double_conv), got "
                       + (" ".join(type(m).__name__ for m in mods) if mods else type(block).__name__))
    _double_conv_layers(mods[1])                                         # (a layout error before anything runs)
    return double_conv_form(engine, mods[1], max_pool2(engine, x), form)
