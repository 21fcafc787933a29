"""Writes the BatchNorm2d [+ ReLU] forward / backward fixtures from the REFERENCE's own double_conv under torch.autograd (imported
unchanged; never runs where the reference is absent):

    python tests/golden/make_golden_bn2d.py --reference /path/to/reference

For every entry of CASES it builds the seeded x, gamma, beta and dy (tests/bn2d_ref.py: case, integer hashing), takes seq =
double_conv(C, C).conv of the reference (superpoint/models/unet_parts.py:10-25), loads gamma and beta into seq[1] (nn.BatchNorm2d), runs
seq[2](seq[1](x)) -- or seq[1](x) alone, the case without ReLU -- in fp32 and float64 on the CPU, differentiates sum(y * dy) with
torch.autograd, and writes bn2d_<case>.npz.  The inputs are NOT stored: the tests re-derive them from the seed.  Per tensor t of y, dx,
dgamma, dbeta, mean, rstd:

  seed, shape = (B, C, H, W), refused  the recipe's arguments and how many seeds the kink rule refused before this one
  t_g, t_d32                           the float64 value at sample_positions(), and the reference's fp32 value minus it at the same positions
  t_sum                                y and dx: a float64 sum per channel (C); the (C) vectors: their float64 total (1)
  running_mean, running_var, nbt       the float64 module's buffers after the step (evaluation mode: unchanged)

mean and rstd are not outputs of the module: they are torch.var_mean of its input over (0, 2, 3) (biased) and 1 / sqrt(var + eps) with
the module's eps, in the run's precision; in evaluation mode the module's running statistics.  `eval` runs the module in .eval() with
the seeded running statistics of tests/bngrad_ref.py: running.

bn2d_head.npz holds a two-layer head in .train() mode and its .eval() output: conv_a 16 -> 32 (3 x 3), bn_a, ReLU, conv_b 32 -> 9
(1 x 1), bn_b on (2, 16, 10, 12) with seeded state -- output, dx and the 8 parameter gradients at up to 400 positions per tensor with a
float64 total each, and the buffers after the step.  The reference's SuperPoint class cannot be imported (its utils need cv2), so
the head is tests/bn2d_ref.py: Head, torch's own modules arranged as superpoint_train.py:20-23 and 47-48 arrange them; only the
double_conv cases above come from reference code.

The kink: ReLU's derivative jumps at z = 0, and an element with |z64| < 1e-5 may fall on either side in fp32.  From each case's starting
seed upward the generator takes the first seed with no such element in a BatchNorm output that a ReLU follows, and records how many it
refused; a seed is also refused when a reference result holds a non-finite value."""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import bn2d_ref as R2   # noqa: E402
from tests import bngrad_ref as R   # noqa: E402

N_SAMPLE = 1000
N_SAMPLE_HEAD = 400
MAX_TRIES = 20
TENSORS = ("y", "dx", "dgamma", "dbeta", "mean", "rstd")
# file -> (starting seed, (B, C, H, W), training, relu)
CASES = {
    "c64": (1, (2, 64, 9, 33), True, True),
    "c128": (11, (1, 128, 15, 20), True, False),
    "c5": (21, (3, 5, 7, 5), True, True),
    "eval": (31, (2, 65, 8, 10), False, False),
    "slabs": (41, (2, 3, 70, 61), True, True),        # more than one slab of 4096 pixels per map, H W % 4 != 0
}
HEAD_SEED0 = 51


def sample_positions(name, tensor, size):
    """the fixed pseudo-random sample of flat positions of one tensor of one file (the tests call this too)"""
    return np.sort(np.random.default_rng([list(CASES).index(name), 43, TENSORS.index(tensor)]).choice(size, min(N_SAMPLE, size), replace=False))


def head_positions(index, size):
    return np.sort(np.random.default_rng([47, int(index)]).choice(size, min(N_SAMPLE_HEAD, size), replace=False))


def channel_sums(t, a):
    """a: the float64 array of tensor t"""
    return a.sum((0, 2, 3)) if t in ("y", "dx") else a.sum(keepdims=True).reshape(1)


def reference_bn2d(double_conv, seed, shape, training, relu, dtype):
    """seq[2](seq[1](x)) (relu) or seq[1](x) of the reference's double_conv(C, C).conv -> (dict of float64 arrays, the BatchNorm output,
    num_batches_tracked)"""
    B, C, H, W = shape
    x, gamma, beta, dy = R2.case(seed, B, C, H, W)
    seq = double_conv(C, C).conv.to(dtype)
    bn, act = seq[1], seq[2]
    assert isinstance(bn, torch.nn.BatchNorm2d) and isinstance(act, torch.nn.ReLU)
    state = {"weight": torch.from_numpy(gamma).to(dtype), "bias": torch.from_numpy(beta).to(dtype)}
    if not training:
        rm, rv = R.running(seed, C)
        state.update({"running_mean": torch.from_numpy(rm).to(dtype), "running_var": torch.from_numpy(rv).to(dtype)})
    bn.load_state_dict(state, strict=False)
    bn.train(training)
    xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
    if training:
        var, mean = torch.var_mean(xt.detach(), (0, 2, 3), unbiased=False)
    else:
        var, mean = bn.running_var.clone(), bn.running_mean.clone()
    z = bn(xt)
    zd = z.detach().double().numpy().copy()               # (the reference's ReLU works in place)
    y = act(z) if relu else z
    (y * torch.from_numpy(dy).to(dtype)).sum().backward()
    res = {"y": y.detach(), "dx": xt.grad, "dgamma": bn.weight.grad, "dbeta": bn.bias.grad, "mean": mean, "rstd": 1 / torch.sqrt(var + bn.eps),
           "running_mean": bn.running_mean, "running_var": bn.running_var}
    return {k: v.double().numpy() for k, v in res.items()}, zd, int(bn.num_batches_tracked)


def build(double_conv, name):
    seed0, shape, training, relu = CASES[name]
    for seed in range(seed0, seed0 + MAX_TRIES):
        r64, z64, nbt = reference_bn2d(double_conv, seed, shape, training, relu, torch.float64)
        r32, _, _ = reference_bn2d(double_conv, seed, shape, training, relu, torch.float32)
        if (relu and R2.kink(z64).any()) or not all(np.isfinite(a).all() for a in list(r32.values()) + list(r64.values())):
            continue
        fx = {"seed": np.int64(seed), "shape": np.array(shape, np.int64), "refused": np.int64(seed - seed0), "nbt": np.int64(nbt),
              "relu": np.int64(relu), "training": np.int64(training), "running_mean": r64["running_mean"], "running_var": r64["running_var"]}
        for t in TENSORS:
            pos = sample_positions(name, t, r64[t].size)
            fx.update({f"{t}_g": r64[t].reshape(-1)[pos], f"{t}_d32": (r32[t] - r64[t]).reshape(-1)[pos].astype(np.float32),
                       f"{t}_sum": channel_sums(t, r64[t])})
        return fx
    return f"no seed from {seed0} passed"


def run_head(seed, dtype):
    """one training step and one evaluation of the head from the same seeded state -> (dict of float64 arrays, bn_a's outputs of both runs,
    the buffers after the step, the evaluation output)"""
    x, dy = (torch.from_numpy(a).to(dtype) for a in R2.head_case(seed))
    zs = []

    def hooked(m):
        return m.bn_a.register_forward_hook(lambda _m, _i, o: zs.append(o.detach().double().numpy().copy()))

    m = R2.load_head(seed, dtype).train()
    hook = hooked(m)
    res = {k: v.double().numpy() for k, v in R2.head_grads(m, m, x, dy).items()}
    hook.remove()
    buffers = R2.head_buffers(m)
    e = R2.load_head(seed, dtype).eval()
    hook = hooked(e)
    with torch.no_grad():
        out = e(x.clone()).double().numpy()
    hook.remove()
    return res, zs, buffers, out


def build_head():
    refused = []
    for seed in range(HEAD_SEED0, HEAD_SEED0 + MAX_TRIES):
        r64, zs, buffers, e64 = run_head(seed, torch.float64)
        r32, _, _, e32 = run_head(seed, torch.float32)
        finite = all(np.isfinite(a).all() for a in list(r64.values()) + list(r32.values()) + [e64, e32])
        if any(R2.kink(z).any() for z in zs) or not finite:
            refused.append(seed)
            continue
        assert len(r64) == 2 + 8 and len(zs) == 2
        fx = {"seed": np.int64(seed), "refused": np.array(refused, np.int64), "names": np.array(list(r64))}
        for i, (name, a) in enumerate(r64.items()):
            pos = head_positions(i, a.size)
            fx.update({f"{name}_g": a.reshape(-1)[pos], f"{name}_d32": (r32[name] - a).reshape(-1)[pos].astype(np.float32),
                       f"{name}_sum": a.sum(keepdims=True).reshape(1)})
        fx["buffer_names"] = np.array(list(buffers))
        fx.update({f"buffer_{i}": b for i, b in enumerate(buffers.values())})
        pos = head_positions(0, e64.size)
        fx.update({"eval_g": e64.reshape(-1)[pos], "eval_d32": (e32 - e64).reshape(-1)[pos].astype(np.float32)})
        return fx
    return f"no seed from {HEAD_SEED0} passed: {refused}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(a.reference, "superpoint", "models"))
    import unet_parts                                   # noqa: E402  (the reference's, unchanged)
    failed = []
    for name, fx in [(n, build(unet_parts.double_conv, n)) for n in CASES] + [("head", build_head())]:
        if isinstance(fx, str):
            print(f"bn2d_{name}.npz REFUSED: {fx}")
            failed.append(name)
            continue
        path = os.path.join(HERE, f"bn2d_{name}.npz")
        np.savez_compressed(path, **fx)
        size = os.path.getsize(path)
        assert size < 200000, f"{path}: {size} bytes"
        print(f"bn2d_{name}.npz: {size} bytes, {len(fx)} arrays, seed {int(fx['seed'])}, refused {np.asarray(fx['refused']).tolist()}")
    assert not failed, f"committed cases were refused: {failed}"


if __name__ == "__main__":
    main()
