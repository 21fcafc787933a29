"""A trainable SuperPoint: the reference's training network (superpoint/models/superpoint_train.py:8-58) as a torch.nn.Module with live
parameters whose forward AND backward run in the libraries -- every convolution, BatchNorm [+ ReLU], max-pooling and the descriptor
normalisation through image_matching_amd.sptrain_net (include/imx_spnet.h, imx_spnorm.h, imx_sppool.h, imx_train.h); PyTorch holds the
parameters and steps the optimiser.

    engine = Engine(None, None, "cuda")
    model = SuperPointTrainable(engine).train()
    optimizer = torch.optim.Adam(model.parameters(), lr=1e-3)
    out = model(images)                              # (B,1,H,W) fp32 -> {'semi': (B,65,H/8,W/8), 'desc': (B,d,H/8,W/8)}
    optimizer.zero_grad()
    loss(out).backward()
    optimizer.step()

The modules are plain nn.Conv2d / nn.BatchNorm2d / nn.ReLU / nn.MaxPool2d containers in the reference's layout with PyTorch's default
initialisation, so state_dict() has exactly the keys and shapes of the reference's checkpoints (synth.superpoint_bn_shapes): a checkpoint
of the reference loads here, and this model's state_dict loads into the inference SuperPoint of superpoint/models/superpoint_train.py,
which stays the inference class it is.  In .train() and .eval() alike the forward runs through sptrain_net; BatchNorm follows the
module's mode and updates its buffers in place in train mode."""
from collections.abc import Mapping

import torch
from torch import nn

from . import sptrain_net as N
from .engine import ImxError


class _DoubleConv(nn.Module):
    """(conv => BN => ReLU) * 2 (unet_parts.py:10-25): the parameters only"""

    def __init__(self, in_ch, out_ch):
        super().__init__()
        self.conv = nn.Sequential(nn.Conv2d(in_ch, out_ch, 3, padding=1), nn.BatchNorm2d(out_ch), nn.ReLU(inplace=True),
                                  nn.Conv2d(out_ch, out_ch, 3, padding=1), nn.BatchNorm2d(out_ch), nn.ReLU(inplace=True))


class _InConv(nn.Module):
    def __init__(self, in_ch, out_ch):
        super().__init__()
        self.conv = _DoubleConv(in_ch, out_ch)


class _Down(nn.Module):
    def __init__(self, in_ch, out_ch):
        super().__init__()
        self.mpconv = nn.Sequential(nn.MaxPool2d(2), _DoubleConv(in_ch, out_ch))


class SuperPointTrainable(nn.Module):
    """SuperPointTrainable(engine, descriptor_length=256, form="auto"): the reference's training SuperPoint with live parameters on
    engine's device.  `form` is the BatchNorm form of sptrain_net.conv_bn_relu_form for the encoder's blocks.  engine = None builds the
    parameters only (state_dict, load_state_dict and the optimiser work; forward raises)."""

    def __init__(self, engine=None, descriptor_length=256, form="auto"):
        super().__init__()
        if form not in ("auto", "channel", "pixels"):
            raise ImxError(f"SuperPointTrainable: form must be 'auto', 'channel' or 'pixels', got {form!r}")
        c1, c2, c3, c4, c5 = 64, 64, 128, 128, 256
        det_h = 65
        self.inc = _InConv(1, c1)
        self.down1 = _Down(c1, c2)
        self.down2 = _Down(c2, c3)
        self.down3 = _Down(c3, c4)
        self.convPa = nn.Conv2d(c4, c5, kernel_size=3, stride=1, padding=1)
        self.bnPa = nn.BatchNorm2d(c5)
        self.convPb = nn.Conv2d(c5, det_h, kernel_size=1, stride=1, padding=0)
        self.bnPb = nn.BatchNorm2d(det_h)
        self.convDa = nn.Conv2d(c4, c5, kernel_size=3, stride=1, padding=1)
        self.bnDa = nn.BatchNorm2d(c5)
        self.convDb = nn.Conv2d(c5, descriptor_length, kernel_size=1, stride=1, padding=0)
        self.bnDb = nn.BatchNorm2d(descriptor_length)
        self.form = form
        self.output = None
        self.engine = engine
        if engine is not None:
            self.to(engine.device)

    def load_state_dict(self, state_dict, strict=True):
        """a checkpoint of the reference, as it stands or as the training script wraps it ({'model_state_dict': state_dict, ...})"""
        if isinstance(state_dict, Mapping) and 'model_state_dict' in state_dict and isinstance(state_dict['model_state_dict'], Mapping):
            state_dict = state_dict['model_state_dict']
        return super().load_state_dict(state_dict, strict)

    def forward(self, x):
        """x (B,1,H,W) fp32 on the engine's device -> {'semi': (B,65,H/8,W/8), 'desc': (B,d,H/8,W/8)}, desc of unit length over its
        channels; the same dict is kept in self.output, as the reference does."""
        if self.engine is None:
            raise ImxError("SuperPointTrainable was built without an engine: there is no CPU path")
        eng = self.engine
        x1 = N.double_conv_form(eng, self.inc.conv, x, self.form)
        x2 = N.down_pooled(eng, self.down1, x1, self.form)
        x3 = N.down_pooled(eng, self.down2, x2, self.form)
        x4 = N.down_pooled(eng, self.down3, x3, self.form)
        semi = N.head(eng, self.convPa, self.bnPa, self.convPb, self.bnPb, x4)
        desc = N.normalize_descriptors(eng, N.head(eng, self.convDa, self.bnDa, self.convDb, self.bnDb, x4))
        output = {'semi': semi, 'desc': desc}
        self.output = output
        return output
