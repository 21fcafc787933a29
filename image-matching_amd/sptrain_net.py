"""SuperPoint's own layers in their training form, with `loss.backward()` running through the project's kernels: the 3x3 convolutions
of libimx_spnet (include/imx_spnet.h, csrc/conv3_train.hip) as a torch.autograd.Function, and with the BatchNorm +
ReLU kernels of libimx_train (sgtrain_grad.bn_relu) the reference's `double_conv` and `down` blocks (superpoint/models/unet_parts.py:10-48).

    conv3x3.apply(engine, x, weight, bias)      F.conv2d(x, weight, bias, padding=1) for a (Cout,Cin,3,3) weight
    conv2d(engine, x, weight, bias)             the same, as a function
    conv_bn_relu(engine, conv, bn, x)           F.relu(bn(conv(x))) for nn.Conv2d(.., 3, padding=1) and nn.BatchNorm2d
    double_conv(engine, block, x)               block(x) for the reference's double_conv
    down(engine, block, x)                      block(x) for the reference's down (nn.MaxPool2d(2) stays F.max_pool2d)

Tensors are the reference's own, NCHW contiguous fp32 on the engine's device; nothing is copied to another layout.  The BatchNorm kernels
take the (B, C, H W) view of the same memory and are bound to N = H W <= 2^20 columns, so conv_bn_relu, double_conv and down serve maps of
H W <= 2^20 pixels (1024 x 1024; the reference trains at 480 x 640); conv2d alone serves H, W <= 4096.  A trainable SuperPointNet (the
heads' BatchNorm without ReLU, the descriptor normalisation) is not here."""
import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from .engine import ImxError
from .sgtrain_grad import _bias_before_batchnorm, _require, bn_relu


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


def conv_bn_relu(engine, conv, bn, x):
    """F.relu(bn(conv(x))) for conv = nn.Conv2d(Cin, Cout, 3, padding=1) and bn = nn.BatchNorm2d(Cout): the convolution through conv2d,
    BatchNorm + ReLU through sgtrain_grad.bn_relu on the (B, Cout, H W) view of the same memory.  bn.training, bn.eps and bn.momentum are
    honoured, and in training mode bn.running_mean, bn.running_var and bn.num_batches_tracked are updated in place, as the module's own
    forward does.  The bias of the convolution gets its exact gradient in training mode, 0 (sgtrain_grad._bias_before_batchnorm); in
    evaluation mode it is formed like any other.  H W <= 2^20 (the BatchNorm kernels' bound).  Any other layout raises ImxError."""
    if not _is_conv3(conv):
        raise ImxError(f"conv_bn_relu: conv must be nn.Conv2d(Cin, Cout, 3, padding=1) with stride 1, no dilation and no groups, got {conv!r}")
    if not isinstance(bn, torch.nn.BatchNorm2d) or bn.num_features != conv.out_channels:
        raise ImxError(f"conv_bn_relu: bn must be nn.BatchNorm2d({conv.out_channels}), got {bn!r}")
    if bn.momentum is None or not bn.affine or not bn.track_running_stats:
        raise ImxError("conv_bn_relu: momentum=None, affine=False and track_running_stats=False are not supported")
    bias = conv.bias
    cancels = bias is not None and bn.training
    h = conv2d(engine, x, conv.weight, bias.detach() if cancels else bias)
    if cancels:
        h = _bias_before_batchnorm.apply(h, bias)
    B, C, H, W = h.shape
    y = bn_relu.apply(engine, h.view(B, C, H * W), bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, None,
                      bn.training, float(bn.momentum), float(bn.eps))
    return y.view(B, C, H, W)


def double_conv(engine, block, x):
    """block(x) for the reference's double_conv (unet_parts.py:10-25): block.conv = Sequential(Conv2d, BatchNorm2d, ReLU, Conv2d,
    BatchNorm2d, ReLU), both convolutions 3 x 3 with padding 1.  Any other layout raises ImxError."""
    seq = getattr(block, "conv", None)
    mods = list(seq) if isinstance(seq, torch.nn.Sequential) else []
    if len(mods) != 6 or not all(_is_conv3(m) for m in mods[0::3]) or not all(isinstance(m, torch.nn.BatchNorm2d) for m in mods[1::3]) \
            or not all(isinstance(m, torch.nn.ReLU) for m in mods[2::3]):
        raise ImxError("double_conv: expected .conv = Sequential(Conv2d(3, padding=1), BatchNorm2d, ReLU, Conv2d(3, padding=1), BatchNorm2d, ReLU), got "
                       + (" ".join(type(m).__name__ for m in mods) if mods else type(block).__name__))
    return conv_bn_relu(engine, mods[3], mods[4], conv_bn_relu(engine, mods[0], mods[1], x))


def down(engine, block, x):
    """block(x) for the reference's down (unet_parts.py:38-48): block.mpconv = Sequential(MaxPool2d(2), double_conv).  The max-pooling
    is F.max_pool2d, forward and backward; the double_conv runs through double_conv().  Any other layout raises ImxError."""
    seq = getattr(block, "mpconv", None)
    mods = list(seq) if isinstance(seq, torch.nn.Sequential) else []
    if len(mods) != 2 or not isinstance(mods[0], torch.nn.MaxPool2d) or mods[0].kernel_size not in (2, (2, 2)) \
            or mods[0].stride not in (2, (2, 2)) or mods[0].padding not in (0, (0, 0)) or mods[0].dilation not in (1, (1, 1)) \
            or mods[0].ceil_mode or mods[0].return_indices:
        raise ImxError("down: expected .mpconv = Sequential(MaxPool2d(2), double_conv), got "
                       + (" ".join(type(m).__name__ for m in mods) if mods else type(block).__name__))
    return double_conv(engine, mods[1], F.max_pool2d(x, 2).contiguous())
