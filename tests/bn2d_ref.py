"""The NCHW view of the project's own statement of BatchNorm + ReLU (tests/bngrad_ref.py, DESIGN.md section 16, used as it is) for the
kernels of csrc/bn2d_train.hip: nn.BatchNorm2d on (B,C,H,W) is nn.BatchNorm1d on the (B,C,H W) view, and without ReLU the forward's
value is z and the backward's mask is all ones.  And the two-layer head of the reference's network (superpoint/models/
superpoint_train.py:20-23, 47-48) restated from torch's own modules, with its seeded state.  No autograd in batch_reference(); the
fixtures the reference's own modules wrote (tests/golden/make_golden_bn2d.py) hold it, and tests/test_bn2d_host.py checks that."""
import numpy as np
import torch

from tests import bngrad_ref as R
from tests.mhagrad_ref import heavy

EPS, MOMENTUM, KINK = R.EPS, R.MOMENTUM, R.KINK
bar = R.bar


def case(seed, B, C, H, W):
    """x (B,C,H,W), gamma (C), beta (C), dy (B,C,H,W): bngrad_ref.case at (B, C, H W), viewed as maps"""
    x, gamma, beta, dy = R.case(seed, B, C, H * W)
    return x.reshape(B, C, H, W), gamma, beta, dy.reshape(B, C, H, W)


def batch_reference(x, gamma, beta, dy, relu=True, training=True, running_mean=None, running_var=None, eps=EPS, momentum=MOMENTUM, mask=None,
                    dtype=torch.float64):
    """everything the two entry points write, as a dict of float64 arrays: y, z, dx (B,C,H,W), mean, rstd, dgamma, dbeta (C) and the
    running statistics after the step where given.  relu=False: y = z and every element passes dy on.  mask (B,C,H,W) booleans replaces
    z > 0 in the backward."""
    B, C, H, W = x.shape
    flat = lambda a: None if a is None else np.asarray(a).reshape(B, C, H * W)
    m = flat(mask) if relu else np.ones((B, C, H * W), bool)
    res = R.batch_reference(flat(x), gamma, beta, flat(dy), None, training, running_mean, running_var, eps, momentum, m, dtype)
    if not relu:
        res["y"] = res["z"].copy()
    for k in ("y", "z", "dx"):
        res[k] = res[k].reshape(B, C, H, W)
    return res


def kink(z64):
    return np.abs(np.asarray(z64)) < KINK


# ---------------------------------------------------------------------------------------------- the head, restated
class Head(torch.nn.Module):
    """superpoint_train.py:20-23 and 47-48 restated from torch's own modules: a 3 x 3 convolution with padding 1, BatchNorm2d, ReLU, a
    1 x 1 convolution, BatchNorm2d (no ReLU after it) -- convPa, bnPa, relu, convPb, bnPb of the detector head; the descriptor head
    (:25-28, :50-51) has the same arrangement"""

    def __init__(self, cin, cmid, cout):
        super().__init__()
        self.relu = torch.nn.ReLU(inplace=True)
        self.conv_a = torch.nn.Conv2d(cin, cmid, kernel_size=3, stride=1, padding=1)
        self.bn_a = torch.nn.BatchNorm2d(cmid)
        self.conv_b = torch.nn.Conv2d(cmid, cout, kernel_size=1, stride=1, padding=0)
        self.bn_b = torch.nn.BatchNorm2d(cout)

    def forward(self, x):
        return self.bn_b(self.conv_b(self.relu(self.bn_a(self.conv_a(x)))))


HEAD = ((16, 32, 9), (2, 16, 10, 12))              # constructor arguments, input shape


def head_state(seed, module):
    """seeded values for the 8 parameters and 4 float buffers of a Head, name -> fp32 array: convolution weights heavy / sqrt(fan-in),
    convolution and BatchNorm biases 0.1 heavy, BatchNorm weight 1 + 0.1 heavy, running_mean 0.1 heavy, running_var 1 + 0.1 |heavy|"""
    out = {}
    for name, p in list(module.named_parameters()) + [(n, b) for n, b in module.named_buffers() if b.dtype.is_floating_point]:
        h = heavy(seed, "head." + name, tuple(p.shape)).astype(np.float64)
        if p.dim() == 4:
            h = h / np.sqrt(p.shape[1] * p.shape[2] * p.shape[3])
        elif name.endswith("running_var"):
            h = 1.0 + 0.1 * np.abs(h)
        else:
            h = 0.1 * h + (1.0 if name in ("bn_a.weight", "bn_b.weight") else 0.0)
        out[name] = h.astype(np.float32)
    return out


def load_head(seed, dtype=torch.float32):
    m = Head(*HEAD[0])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in head_state(seed, m).items()}, strict=False)
    return m.to(dtype)


def head_case(seed):
    """x and dy fp32: the input and the cotangent of the head's output"""
    (_, _, cout), (B, cin, H, W) = HEAD
    return heavy(seed, "head.x", (B, cin, H, W)), heavy(seed, "head.dy", (B, cout, H, W))


def head_grads(module, forward, x, dy):
    """out = forward(x) on a leaf, the gradients of sum(out * dy) -> dict name -> tensor: out, dx and one per parameter"""
    module.zero_grad()
    x = x.clone().requires_grad_(True)
    with torch.enable_grad():
        out = forward(x)
        (out * dy).sum().backward()
    res = {"out": out.detach(), "dx": x.grad}
    res.update({name: p.grad.clone() for name, p in module.named_parameters()})
    return res


def head_buffers(module):
    """name -> float64 array of every buffer (running_mean, running_var, num_batches_tracked)"""
    return {n: b.detach().double().cpu().numpy() for n, b in module.named_buffers()}
