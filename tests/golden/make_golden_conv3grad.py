"""Writes the 3x3-convolution forward / backward fixtures from the REFERENCE's own double_conv and down under torch.autograd
(superpoint/models/unet_parts.py, imported unchanged: it needs torch only; never runs where the reference is absent):

    python tests/golden/make_golden_conv3grad.py --reference /path/to/reference

Single convolutions.  For every item of CASES it builds the seeded x, w, bias and dy (tests/conv3grad_ref.py: case, integer hashing),
loads w and bias into double_conv(Cin, Cout).conv[0] (exactly nn.Conv2d(Cin, Cout, 3, padding=1)), runs it in fp32 and float64 on the
CPU, differentiates sum(y * dy) with torch.autograd, and writes conv3grad_<case>.npz.  The inputs are NOT stored: the tests re-derive
them from the seed.  Per tensor t of y, dx, dw, db:

  seed, shape = (B, Cout, Cin, H, W)   the recipe's arguments
  t_g, t_d32                           the float64 value at sample_positions() (up to a thousand), and the reference's fp32 value minus it
  t_sum                                a float64 sum per channel: y (Cout) and dx (Cin) over images and pixels, dw (Cout) over each output
                                       channel's weights, db whole (1)

Blocks.  double_conv(3, 16) on (2, 3, 10, 12) and down(16, 32) on (2, 16, 20, 24) (conv3grad_ref.BLOCKS) in .train() mode with the
seeded parameters and running statistics of conv3grad_ref.block_state: conv3grad_block_<kind>.npz holds

  seed, refused                        the seed taken and the seeds the rule below refused before it
  names                                "out", "dx" and the 8 parameter names; per name t: t_g, t_d32 (up to 400 positions) and t_sum (1)
  buffer_names, buffer_<i>             every BatchNorm buffer of the float64 module after the step (num_batches_tracked is 1)
  eval_g, eval_d32                     the block's output in .eval() mode from the same starting state, at the positions of "out"

The seed rule, as in make_golden_sgmodel.py: ReLU's derivative jumps at 0, so from SEED0 upward the generator takes the first seed with no
BatchNorm pre-activation of the float64 run (training step and evaluation) within KINK = 1e-5 of 0 and no non-finite reference value;
main() prints the seeds it refused."""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import conv3grad_ref as R   # noqa: E402

N_SAMPLE = 1000
N_SAMPLE_BLOCK = 400
KINK = 1e-5
TENSORS = ("y", "dx", "dw", "db")
# file -> (seed, B, Cout, Cin, H, W)
CASES = {
    "first": (1, 2, 64, 1, 17, 37),
    "c64": (2, 2, 64, 64, 9, 33),
    "c128": (3, 1, 128, 64, 15, 20),
    "head": (4, 1, 256, 128, 9, 13),
    "odd": (5, 3, 5, 3, 7, 5),
}
SEED0 = {"double_conv": 11, "down": 21}
MAX_TRIES = 20


def sample_positions(seed, tensor, size):
    """the fixed pseudo-random sample of flat positions of one tensor of one file (the tests call this too)"""
    return np.sort(np.random.default_rng([int(seed), 31, TENSORS.index(tensor)]).choice(size, min(N_SAMPLE, size), replace=False))


def block_positions(seed, index, size):
    return np.sort(np.random.default_rng([int(seed), 37, int(index)]).choice(size, min(N_SAMPLE_BLOCK, size), replace=False))


def channel_sums(t, a):
    """a: the float64 array of tensor t"""
    return {"y": lambda: a.sum((0, 2, 3)), "dx": lambda: a.sum((0, 2, 3)), "dw": lambda: a.sum((1, 2, 3)), "db": lambda: a.sum(keepdims=True)}[t]()


def reference_conv(double_conv, x, w, bias, dy, dtype):
    """conv[0] of the reference's double_conv(Cin, Cout) with w and bias loaded -> y, dx, dw, db as float64 arrays"""
    conv = double_conv(w.shape[1], w.shape[0]).conv[0].to(dtype)
    assert isinstance(conv, torch.nn.Conv2d) and conv.kernel_size == (3, 3) and conv.padding == (1, 1) and conv.stride == (1, 1)
    conv.load_state_dict({"weight": torch.from_numpy(w).to(dtype), "bias": torch.from_numpy(bias).to(dtype)})
    xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
    y = conv(xt)
    (y * torch.from_numpy(dy).to(dtype)).sum().backward()
    return {"y": y.detach().double().numpy(), "dx": xt.grad.double().numpy(), "dw": conv.weight.grad.double().numpy(),
            "db": conv.bias.grad.double().numpy()}


def build(double_conv, item):
    seed, B, Cout, Cin, H, W = item
    x, w, bias, dy = R.case(seed, B, Cout, Cin, H, W)
    r32, r64 = reference_conv(double_conv, x, w, bias, dy, torch.float32), reference_conv(double_conv, x, w, bias, dy, torch.float64)
    if not all(np.isfinite(a).all() for a in list(r32.values()) + list(r64.values())):
        return f"seed {seed}: a result of the reference holds a non-finite value"
    fx = {"seed": np.int64(seed), "shape": np.array([B, Cout, Cin, H, W], np.int64)}
    for t in TENSORS:
        pos = sample_positions(seed, t, r64[t].size)
        fx.update({f"{t}_g": r64[t].reshape(-1)[pos], f"{t}_d32": (r32[t] - r64[t]).reshape(-1)[pos].astype(np.float32),
                   f"{t}_sum": channel_sums(t, r64[t])})
    return fx


def run_block(ctor, kind, seed, dtype):
    """one training step and one evaluation of the reference's block from the same seeded state -> (dict of float64 arrays, the BatchNorm
    outputs of both runs, the buffers after the step, the evaluation output)"""
    args, _ = R.BLOCKS[kind]
    x, dy = (torch.from_numpy(a).to(dtype) for a in R.block_case(seed, kind))
    m = R.load_block(ctor(*args), seed, dtype).train()
    res = {}
    zs = R.bn2d_outputs(m, lambda: res.update(R.block_grads(m, m, x, dy)))
    res = {k: v.double().numpy() for k, v in res.items()}
    buffers = R.block_buffers(m)
    e = R.load_block(ctor(*args), seed, dtype).eval()
    out = {}
    with torch.no_grad():
        zs += R.bn2d_outputs(e, lambda: out.update(y=e(x.clone())))
    return res, zs, buffers, out["y"].double().numpy()


def build_block(ctor, kind):
    refused = []
    for seed in range(SEED0[kind], SEED0[kind] + MAX_TRIES):
        r64, zs, buffers, e64 = run_block(ctor, kind, seed, torch.float64)
        r32, _, _, e32 = run_block(ctor, kind, seed, torch.float32)
        finite = all(np.isfinite(a).all() for a in list(r64.values()) + list(r32.values()) + [e64, e32])
        if any((np.abs(z) < KINK).any() for z in zs) or not finite:
            refused.append(seed)
            continue
        assert len(r64) == 2 + 8 and len(zs) == 4
        assert all(np.abs(a).max() > 0 for n, a in r64.items() if not n.endswith("0.bias") and not n.endswith("3.bias")), "a gradient of the reference is identically 0"
        fx = {"seed": np.int64(seed), "refused": np.array(refused, np.int64), "names": np.array(list(r64)),
              "min_preactivation": np.float64(min(np.abs(z).min() for z in zs))}
        for i, (name, a) in enumerate(r64.items()):
            pos = block_positions(seed, i, a.size)
            fx.update({f"{name}_g": a.reshape(-1)[pos], f"{name}_d32": (r32[name] - a).reshape(-1)[pos].astype(np.float32),
                       f"{name}_sum": a.sum(keepdims=True).reshape(1)})
        fx["buffer_names"] = np.array(list(buffers))
        fx.update({f"buffer_{i}": b for i, b in enumerate(buffers.values())})
        pos = block_positions(seed, 0, e64.size)
        fx.update({"eval_g": e64.reshape(-1)[pos], "eval_d32": (e32 - e64).reshape(-1)[pos].astype(np.float32)})
        return fx
    return f"no seed from {SEED0[kind]} passed: {refused}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(a.reference, "superpoint", "models"))
    import unet_parts                                   # noqa: E402  (the reference's, unchanged)
    failed = []
    for name, item in CASES.items():
        fx = build(unet_parts.double_conv, item)
        if isinstance(fx, str):
            print(f"conv3grad_{name}.npz REFUSED: {fx}")
            failed.append(name)
            continue
        path = os.path.join(HERE, f"conv3grad_{name}.npz")
        np.savez_compressed(path, **fx)
        print(f"conv3grad_{name}.npz: {os.path.getsize(path)} bytes, {len(fx)} arrays")
    for kind, ctor in (("double_conv", unet_parts.double_conv), ("down", unet_parts.down)):
        fx = build_block(ctor, kind)
        if isinstance(fx, str):
            print(f"conv3grad_block_{kind}.npz REFUSED: {fx}")
            failed.append(kind)
            continue
        path = os.path.join(HERE, f"conv3grad_block_{kind}.npz")
        np.savez_compressed(path, **fx)
        print(f"conv3grad_block_{kind}.npz: {os.path.getsize(path)} bytes, {len(fx)} arrays, seed {int(fx['seed'])}, refused {fx['refused'].tolist()}, "
              f"smallest |pre-activation| {float(fx['min_preactivation']):.3g}")
    assert not failed, f"committed cases were refused: {failed}"
    for f in os.listdir(HERE):
        if f.startswith("conv3grad_") and f.endswith(".npz"):
            assert os.path.getsize(os.path.join(HERE, f)) < 400000, f


if __name__ == "__main__":
    main()
