"""The project's own statement of what the kernels of csrc/conv3_train.hip compute: nn.Conv2d(Cin, Cout, 3, padding=1)
(superpoint/models/unet_parts.py:15, 18) and its derivative with respect to the input, the weight and the bias, as the closed forms of
DESIGN.md section 18 written out in torch on the CPU (float64 or fp32) as nine shifted products -- no autograd and no convolution
routine in batch_reference(); autograd() differentiates F.conv2d with torch.autograd for the cross-check.  Held to the fixtures the
reference's own double_conv wrote under torch.autograd (tests/golden/make_golden_conv3grad.py) by tests/test_conv3grad_host.py; the
kernels are held to it and to those fixtures by tests/test_gpu_conv3grad.py.  No bits are claimed between this file and the kernels: the
fp32 mode runs torch's summation orders, the kernels their own (fixed) ones.

Tensors are the reference's: x (B,Cin,H,W), w (Cout,Cin,3,3), bias (Cout) or None, y and dy (B,Cout,H,W).

The second half restates the reference's double_conv and down blocks (the same module tree, so the parameter names agree) for the block
fixtures and for the GPU tests, which cannot read the reference."""
import numpy as np
import torch

from tests.mhagrad_ref import heavy
from tests.otgrad_ref import bar  # noqa: F401  (the default bar, element-wise: max(1e-4 + 1e-4 |g64|, 2.5 |ref32 - g64|))


# ---------------------------------------------------------------------------------------------- seeded cases
def case(seed, B, Cout, Cin, H, W, wseed=None):
    """x (B,Cin,H,W), w (Cout,Cin,3,3), bias (Cout), dy (B,Cout,H,W) fp32: heavy-tailed activations and cotangent, weights
    heavy / sqrt(9 Cin), bias 0.1 heavy; wseed: another seed for w and bias"""
    wseed = seed if wseed is None else wseed
    w = (heavy(wseed, "c3.w", (Cout, Cin, 3, 3)).astype(np.float64) / np.sqrt(9 * Cin)).astype(np.float32)
    bias = (0.1 * heavy(wseed, "c3.bias", (Cout,)).astype(np.float64)).astype(np.float32)
    return heavy(seed, "c3.x", (B, Cin, H, W)), w, bias, heavy(seed, "c3.dy", (B, Cout, H, W))


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a)).to(dtype)


# ---------------------------------------------------------------------------------------------- the closed forms
def batch_reference(x, w, bias, dy, dtype=torch.float64):
    """everything the two entry points write, as a dict of float64 arrays: y, dx, dw, db.  Each tap (u, v) is one shifted product over
    the channels; x and dy are 0 outside the image."""
    x, w, dy = _t(x, dtype), _t(w, dtype), _t(dy, dtype)
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    xp, dyp = torch.zeros(B, Cin, H + 2, W + 2, dtype=dtype), torch.zeros(B, Cout, H + 2, W + 2, dtype=dtype)
    xp[:, :, 1:H + 1, 1:W + 1] = x
    dyp[:, :, 1:H + 1, 1:W + 1] = dy
    y = torch.zeros(B, Cout, H, W, dtype=dtype)
    dx, dw = torch.zeros_like(x), torch.zeros_like(w)
    for u in range(3):
        for v in range(3):
            xs = xp[:, :, u:u + H, v:v + W]                                 # x[b][c][i+u-1][j+v-1]
            y += torch.einsum("oc,bchw->bohw", w[:, :, u, v], xs)
            dx += torch.einsum("oc,bohw->bchw", w[:, :, u, v], dyp[:, :, 2 - u:2 - u + H, 2 - v:2 - v + W])   # dy[b][o][i-u+1][j-v+1]
            dw[:, :, u, v] = torch.einsum("bohw,bchw->oc", dy, xs)
    if bias is not None:
        y += _t(bias, dtype)[None, :, None, None]
    return {"y": y.double().numpy(), "dx": dx.double().numpy(), "dw": dw.double().numpy(), "db": dy.sum((0, 2, 3)).double().numpy()}


def autograd(x, w, bias, dy, dtype=torch.float64):
    """F.conv2d(x, w, bias, padding=1) differentiated by torch.autograd -> dict of float64 arrays: y, dx, dw, db"""
    with torch.enable_grad():
        leaves = [_t(a, dtype).requires_grad_(True) for a in (x, w, bias)]
        y = torch.nn.functional.conv2d(*leaves, padding=1)
        gx, gw, gb = torch.autograd.grad(y, leaves, _t(dy, dtype))
    return {"y": y.detach().double().numpy(), "dx": gx.double().numpy(), "dw": gw.double().numpy(), "db": gb.double().numpy()}


# ---------------------------------------------------------------------------------------------- the reference's blocks, restated
class DoubleConv(torch.nn.Module):
    """unet_parts.py:10-25 restated: twice (3 x 3 convolution with padding 1, BatchNorm2d, ReLU), held in .conv"""

    def __init__(self, cin, cout):
        super().__init__()
        layers = []
        for c in (cin, cout):
            layers += [torch.nn.Conv2d(c, cout, kernel_size=3, padding=1), torch.nn.BatchNorm2d(cout), torch.nn.ReLU(inplace=True)]
        self.conv = torch.nn.Sequential(*layers)

    def forward(self, x):
        return self.conv(x)


class Down(torch.nn.Module):
    """unet_parts.py:38-48 restated: 2 x 2 max-pooling, then a DoubleConv, held in .mpconv"""

    def __init__(self, cin, cout):
        super().__init__()
        self.mpconv = torch.nn.Sequential(torch.nn.MaxPool2d(2), DoubleConv(cin, cout))

    def forward(self, x):
        return self.mpconv(x)


# kind -> (constructor arguments, input shape)
BLOCKS = {"double_conv": ((3, 16), (2, 3, 10, 12)), "down": ((16, 32), (2, 16, 20, 24))}


def block_state(seed, module):
    """seeded values for the 8 parameters and 4 float buffers of a block (the reference's or the restated one: the names agree), name ->
    fp32 array: convolution weights heavy / sqrt(fan-in), convolution and BatchNorm biases 0.1 heavy, BatchNorm weight 1 + 0.1 heavy,
    running_mean 0.1 heavy, running_var 1 + 0.1 |heavy|"""
    out = {}
    for name, p in list(module.named_parameters()) + [(n, b) for n, b in module.named_buffers() if b.dtype.is_floating_point]:
        h = heavy(seed, "block." + name, tuple(p.shape)).astype(np.float64)
        if p.dim() == 4:
            h = h / np.sqrt(9 * p.shape[1])
        elif name.endswith("running_var"):
            h = 1.0 + 0.1 * np.abs(h)
        else:
            is_bn_weight = name.endswith(".weight")                       # (the only one-dimensional .weight of a block is a BatchNorm's)
            h = 0.1 * h + (1.0 if is_bn_weight else 0.0)
        out[name] = h.astype(np.float32)
    return out


def load_block(module, seed, dtype=torch.float32):
    """module with block_state(seed) loaded (num_batches_tracked stays 0), converted to dtype"""
    module.load_state_dict({k: torch.from_numpy(v) for k, v in block_state(seed, module).items()}, strict=False)
    return module.to(dtype)


def block_case(seed, kind):
    """x and dy fp32 for BLOCKS[kind]: the input and the cotangent of the block's output"""
    (cin, cout), shape = BLOCKS[kind]
    B, _, H, W = shape
    if kind == "down":
        H, W = H // 2, W // 2
    return heavy(seed, "block.x", shape), heavy(seed, "block.dy", (B, cout, H, W))


def block_grads(module, forward, x, dy):
    """out = forward(x) on a leaf, the gradients of sum(out * dy) -> dict name -> tensor: out, dx and one per parameter"""
    module.zero_grad()
    x = x.clone().requires_grad_(True)
    with torch.enable_grad():
        out = forward(x)
        (out * dy).sum().backward()
    res = {"out": out.detach(), "dx": x.grad}
    res.update({name: p.grad.clone() for name, p in module.named_parameters()})
    return res


def block_buffers(module):
    """name -> float64 array of every buffer (running_mean, running_var, num_batches_tracked)"""
    return {n: b.detach().double().cpu().numpy() for n, b in module.named_buffers()}


def bn2d_outputs(module, run):
    """run() with a hook on every BatchNorm2d of module -> the list of their outputs (the pre-activations of the ReLUs), as float64 arrays"""
    seen, hooks = [], []
    for m in module.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            hooks.append(m.register_forward_hook(lambda _m, _i, o: seen.append(o.detach().double().numpy().copy())))
    try:
        run()
    finally:
        for h in hooks:
            h.remove()
    return seen
