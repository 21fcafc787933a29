"""The project's own statement of what the kernels of csrc/sppool_train.hip compute: nn.MaxPool2d(2) as the scan
it is -- written out, not a call to torch -- with its backward, exact in any precision; and the descriptor normalisation
desc / ||desc||_2 (superpoint/models/superpoint_train.py:53-54) with its backward as closed forms in float64.  tests/test_sppool_host.py
holds both to torch (F.max_pool2d(return_indices=True) and its autograd bit for bit; torch.autograd of the reference's two lines and
central differences); the kernels are held to them by tests/test_gpu_sppool.py.

The second half restates the reference's network (superpoint_train.py:8-58) from the restated blocks of tests/conv3grad_ref.py and
torch's own modules, with the reference's module tree, so the parameter names agree -- for the fixtures of
tests/golden/make_golden_sppool.py and for the GPU tests, which cannot read the reference."""
import numpy as np
import torch

from tests import conv3grad_ref as R3
from tests.mhagrad_ref import heavy
from tests.otgrad_ref import bar  # noqa: F401  (the default bar, element-wise: max(1e-4 + 1e-4 |g64|, 2.5 |ref32 - g64|))

KINK = 1e-5          # a BatchNorm pre-activation this close to 0, or two positive leaders of a pooling window this close, may fall either way in fp32


# ---------------------------------------------------------------------------------------------- max-pooling
def pool_forward(x):
    """x (B,C,H,W) of any float dtype -> (y (B,C,H//2,W//2) of that dtype, idx uint8): every window scanned (0,0), (0,1), (1,0), (1,1)
    from its first element, a later one taken when v > best or v is NaN; idx = 2 row + col of the taken element"""
    x = np.asarray(x)
    B, C, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    best = x[:, :, 0:2 * Ho:2, 0:2 * Wo:2].copy()
    at = np.zeros(best.shape, np.uint8)
    for code, (i, j) in ((1, (0, 1)), (2, (1, 0)), (3, (1, 1))):
        v = x[:, :, i:2 * Ho:2, j:2 * Wo:2]
        with np.errstate(invalid="ignore"):
            take = (v > best) | np.isnan(v)
        best = np.where(take, v, best)
        at = np.where(take, np.uint8(code), at)
    return best, at


def pool_backward(idx, dy, shape):
    """dx of `shape` = (B,C,H,W): dy at the recorded element of each window, +0 everywhere else (the trailing row / column of an odd
    H / W too); a select, never a product"""
    idx, dy = np.asarray(idx), np.asarray(dy)
    B, C, H, W = shape
    Ho, Wo = H // 2, W // 2
    dx = np.zeros(shape, dy.dtype)
    for code, (i, j) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        dx[:, :, i:2 * Ho:2, j:2 * Wo:2] = np.where(idx == code, dy, dy.dtype.type(0))
    return dx


NAN, INF = np.float32(np.nan), np.float32(np.inf)
# the nine special windows, row-major (v00, v01, v10, v11) -> the index PyTorch records
SPECIAL_WINDOWS = (
    ("all equal", (0.0, 0.0, 0.0, 0.0), 0),
    ("tie 0 1", (2.0, 2.0, 1.0, 0.0), 0),
    ("tie 1 2", (1.0, 2.0, 2.0, 0.0), 1),
    ("tie 2 3", (0.0, 1.0, 2.0, 2.0), 2),
    ("nan first", (NAN, 5.0, 6.0, 7.0), 0),
    ("two nans", (1.0, NAN, 9.0, NAN), 3),
    ("nan before a larger value", (1.0, NAN, 9.0, 2.0), 1),
    ("all -inf", (-INF, -INF, -INF, -INF), 0),
    ("-0 before +0", (-0.0, 0.0, -0.0, 0.0), 0),
)


def pool_case(seed, B, C, H, W, relu_like=False):
    """x (B,C,H,W) and dy (B,C,H//2,W//2) fp32, heavy-tailed; relu_like: the negative half of x replaced by exact zeros"""
    x = heavy(seed, "pool.x", (B, C, H, W))
    if relu_like:
        x = np.maximum(x, np.float32(0))
    return x, heavy(seed, "pool.dy", (B, C, H // 2, W // 2))


def plant(x, where):
    """a copy of x (B,C,H,W) with the nine special windows planted, one per (image, channel) plane in turn, at the window position
    `where`(H, W) -> (row, col) of window coordinates"""
    x = x.copy()
    B, C, H, W = x.shape
    r, c = where(H, W)
    for n, (_, w, _) in enumerate(SPECIAL_WINDOWS):
        b, ch = (n // C) % B, n % C
        x[b, ch, 2 * r:2 * r + 2, 2 * c:2 * c + 2] = np.array(w, np.float32).reshape(2, 2)
    return x


# ---------------------------------------------------------------------------------------------- desc / ||desc||_2
def l2_case(seed, B, C, HW):
    """x and dy (B,C,HW) fp32, heavy-tailed"""
    return heavy(seed, "l2.x", (B, C, HW)), heavy(seed, "l2.dy", (B, C, HW))


def l2_reference(x, dy):
    """everything the two entry points write, as float64 arrays: norm (B,HW) = sqrt(sum_c x^2), y = x / norm, s = sum_c y dy,
    dx = (dy - y s) / norm.  No autograd."""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        norm = np.sqrt((x * x).sum(1))
        y = x / norm[:, None]
        s = (y * dy).sum(1)
        dx = (dy - y * s[:, None]) / norm[:, None]
    return {"y": y, "norm": norm, "dx": dx}


def l2_autograd(x, dy, dtype=torch.float64):
    """the reference's two lines (superpoint_train.py:53-54) under torch.autograd -> y, dx as float64 arrays"""
    with torch.enable_grad():
        xt = torch.as_tensor(np.asarray(x)).to(dtype).requires_grad_(True)
        dn = torch.norm(xt, p=2, dim=1)
        y = xt.div(torch.unsqueeze(dn, 1))
        gx, = torch.autograd.grad(y, xt, torch.as_tensor(np.asarray(dy)).to(dtype))
    return {"y": y.detach().double().numpy(), "dx": gx.double().numpy()}


# ---------------------------------------------------------------------------------------------- the reference's network, restated
class InConv(torch.nn.Module):
    """unet_parts.py:28-35 restated: a DoubleConv held in .conv"""

    def __init__(self, cin, cout):
        super().__init__()
        self.conv = R3.DoubleConv(cin, cout)

    def forward(self, x):
        return self.conv(x)


class Net(torch.nn.Module):
    """superpoint_train.py:8-58 restated: inconv, three downs, the two heads arranged as lines 20-28 and 47-51 arrange them, and the
    descriptor normalisation of lines 53-54.  `inconv` and `down` are the block classes: the restated ones here, the reference's own in
    tests/golden/make_golden_sppool.py."""

    def __init__(self, descriptor_length=256, inconv=InConv, down=R3.Down):
        super().__init__()
        c1, c2, c3, c4, c5 = 64, 64, 128, 128, 256
        det_h = 65
        self.inc = inconv(1, c1)
        self.down1 = down(c1, c2)
        self.down2 = down(c2, c3)
        self.down3 = down(c3, c4)
        self.relu = torch.nn.ReLU(inplace=True)
        self.convPa = torch.nn.Conv2d(c4, c5, kernel_size=3, stride=1, padding=1)
        self.bnPa = torch.nn.BatchNorm2d(c5)
        self.convPb = torch.nn.Conv2d(c5, det_h, kernel_size=1, stride=1, padding=0)
        self.bnPb = torch.nn.BatchNorm2d(det_h)
        self.convDa = torch.nn.Conv2d(c4, c5, kernel_size=3, stride=1, padding=1)
        self.bnDa = torch.nn.BatchNorm2d(c5)
        self.convDb = torch.nn.Conv2d(c5, descriptor_length, kernel_size=1, stride=1, padding=0)
        self.bnDb = torch.nn.BatchNorm2d(descriptor_length)

    def forward(self, x):
        x4 = self.down3(self.down2(self.down1(self.inc(x))))
        semi = self.bnPb(self.convPb(self.relu(self.bnPa(self.convPa(x4)))))
        desc = self.bnDb(self.convDb(self.relu(self.bnDa(self.convDa(x4)))))
        dn = torch.norm(desc, p=2, dim=1)
        desc = desc.div(torch.unsqueeze(dn, 1))
        return {'semi': semi, 'desc': desc}


D_NET = 128
NET_CASES = {"even": (2, 1, 16, 24), "odd": (2, 1, 18, 27)}      # odd: floor pooling drops a row or a column at every level
ADAM_STEPS, ADAM_LR = 4, 1e-3


def load_net(module, seed, dtype=torch.float32):
    """module with conv3grad_ref.block_state(seed) loaded -- the recipe of the block fixtures over every parameter and float buffer of the
    network; num_batches_tracked stays 0 -- converted to dtype"""
    return R3.load_block(module, seed, dtype)


def net_case(seed, name):
    """x, dy_s, dy_d, t_s, t_d fp32 for NET_CASES[name]: the images, the cotangents of semi and desc, and the targets of the Adam steps"""
    B, _, H, W = NET_CASES[name]
    hs, ws = H // 8, W // 8
    return (heavy(seed, "net.x", (B, 1, H, W)), heavy(seed, "net.dy_s", (B, 65, hs, ws)), heavy(seed, "net.dy_d", (B, D_NET, hs, ws)),
            heavy(seed, "net.t_s", (B, 65, hs, ws)), (0.1 * heavy(seed, "net.t_d", (B, D_NET, hs, ws)).astype(np.float64)).astype(np.float32))


def net_grads(module, x, dy_s, dy_d):
    """out = module(x) on a leaf, the gradients of sum(semi dy_s) + sum(desc dy_d) -> dict name -> tensor: semi, desc, dx and one per
    parameter"""
    module.zero_grad()
    x = x.clone().requires_grad_(True)
    with torch.enable_grad():
        out = module(x)
        ((out['semi'] * dy_s).sum() + (out['desc'] * dy_d).sum()).backward()
    res = {"semi": out['semi'].detach(), "desc": out['desc'].detach(), "dx": x.grad}
    res.update({name: p.grad.clone() for name, p in module.named_parameters()})
    return res


def net_buffers(module):
    """name -> float64 array of every buffer (running_mean, running_var, num_batches_tracked)"""
    return {n: b.detach().double().cpu().numpy() for n, b in module.named_buffers()}


def adam_losses(module, x, t_s, t_d, steps=ADAM_STEPS, lr=ADAM_LR):
    """the losses mean((semi - t_s)^2) + mean((desc - t_d)^2) of `steps` Adam steps from the module's state, as a list of floats"""
    opt = torch.optim.Adam(module.parameters(), lr=lr)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        with torch.enable_grad():
            out = module(x)
            loss = ((out['semi'] - t_s) ** 2).mean() + ((out['desc'] - t_d) ** 2).mean()
            loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses


def net_positions(index, size, n=400):
    """the fixed pseudo-random sample of flat positions of tensor `index` of a network fixture"""
    return np.sort(np.random.default_rng([53, int(index)]).choice(size, min(n, size), replace=False))


def unsafe(module, x):
    """what refuses a seed, counted in one float64 forward of `module` (train mode, on a copy of its buffers' effect: the caller reloads
    the state afterwards): (BatchNorm pre-activations a ReLU follows within KINK of 0, pooling windows whose two largest values are
    positive and closer than KINK, zero descriptor vectors)"""
    counts = [0, 0, 0]
    hooks = []

    def after_bn(_m, _i, o):
        counts[0] += int((o.detach().abs() < KINK).sum())

    def before_pool(_m, i):
        v = i[0].detach()
        B, C, H, W = v.shape
        w = v[:, :, :H // 2 * 2, :W // 2 * 2].reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)
        top = torch.sort(w, dim=-1, descending=True).values
        counts[1] += int(((top[..., 1] > 0) & (top[..., 0] - top[..., 1] < KINK)).sum())

    def after_db(_m, _i, o):
        counts[2] += int((o.detach().abs().sum(1) == 0).sum())

    mods = dict(module.named_modules())
    for name, m in mods.items():
        if isinstance(m, torch.nn.MaxPool2d):
            hooks.append(m.register_forward_pre_hook(before_pool))
        elif isinstance(m, torch.nn.BatchNorm2d) and name not in ("bnPb", "bnDb"):        # every other BatchNorm feeds a ReLU
            hooks.append(m.register_forward_hook(after_bn))
    hooks.append(mods["bnDb"].register_forward_hook(after_db))
    with torch.no_grad():
        module(x)
    for h in hooks:
        h.remove()
    return tuple(counts)
