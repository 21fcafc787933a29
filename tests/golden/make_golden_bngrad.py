"""Writes the BatchNorm1d + ReLU forward / backward fixtures from the REFERENCE's own MLP and KeypointEncoder under torch.autograd
(imported unchanged; never runs where the reference is absent):

    python tests/golden/make_golden_bngrad.py --reference /path/to/reference

For every entry of CASES it builds the seeded x, gamma, beta and dy (tests/bngrad_ref.py: case, integer hashing), takes seq =
MLP([C, C, C]) of the reference (superglue/models/superglue_train.py:46-57), loads gamma and beta into seq[1] (nn.BatchNorm1d), runs
seq[2](seq[1](x)) in fp32 and float64 on the CPU, differentiates sum(y * dy) with torch.autograd, and writes bngrad_<case>.npz.  The
inputs are NOT stored: the tests re-derive them from the seed.  Per tensor t of y, dx, dgamma, dbeta:

  seed, shape = (B, C, N), refused     the recipe's arguments and how many seeds the kink rule refused before this one
  t_g, t_d32                           the float64 value at sample_positions(), and the reference's fp32 value minus it at the same positions
  t_sum                                y and dx: a float64 sum per channel (C); dgamma and dbeta: their float64 total (1)
  running_mean, running_var, nbt       the float64 module's buffers after the step (evaluation mode: unchanged)

`eval` runs the module in .eval() with the seeded running statistics of tests/bngrad_ref.py: running.  `ragged` is the reference's
BatchNorm on (1, 64, 94): the valid columns of three pairs of 60, 33 and 1 columns, concatenated -- what a NaN-padded batch of three in a
frame of 64 must reproduce.  bngrad_kenc.npz holds the reference's KeypointEncoder(128, [32, 64, 128]) in .train() mode with seeded
parameters on 70 keypoints: the output, dkpts, dscores and the gradients of all 14 parameters at up to 400 positions per tensor, a
float64 sum per channel (kenc_sums), and the three BatchNorm modules' buffers after the step.  The reference's AttentionalPropagation is
not imported here: its fixture is tests/golden/lingrad_layer.npz (make_golden_lingrad.py), whose seed tests/test_bngrad_host.py shows
to have no element at the kink, so the layer tests use it as it is and no bngrad_layer.npz is written.

The kink: ReLU's derivative jumps at z = 0, and an element with |z64| < 1e-5 (about a hundred times what fp32 puts on z) may fall on
either side in fp32.  From each case's starting seed upward the generator takes the first seed with no such element in any BatchNorm
output, and records how many it refused; a seed is also refused when a reference result holds a non-finite value."""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import bngrad_ref as R   # noqa: E402

N_SAMPLE = 1000
N_SAMPLE_KENC = 400
MAX_REFUSED = 3
TENSORS = ("y", "dx", "dgamma", "dbeta")
RAGGED_COUNTS, RAGGED_FRAME = (60, 33, 1), 64
# file -> (starting seed, (B, C, N), training)
CASES = {
    "c256": (1, (1, 256, 100), True),
    "c32": (11, (1, 32, 50), True),
    "b2": (21, (2, 64, 45), True),
    "eval": (31, (1, 128, 70), False),
    "ragged": (41, (1, 64, sum(RAGGED_COUNTS)), True),
}
KENC = (51, 128, (32, 64, 128), 70)               # starting seed, feature_dim, layers, keypoints


def sample_positions(name, tensor, size):
    """the fixed pseudo-random sample of flat positions of one tensor of one file (the tests call this too)"""
    return np.sort(np.random.default_rng([list(CASES).index(name), 31, TENSORS.index(tensor)]).choice(size, min(N_SAMPLE, size), replace=False))


def kenc_positions(index, size):
    return np.sort(np.random.default_rng([37, int(index)]).choice(size, min(N_SAMPLE_KENC, size), replace=False))


def channel_sums(t, a):
    """a: the float64 array of tensor t"""
    return a.sum((0, 2)) if t in ("y", "dx") else a.sum(keepdims=True).reshape(1)


def kenc_sums(name, a):
    """a float64 sum per channel of one tensor of the keypoint-encoder record: out (1,d,N) over the columns, a convolution weight
    (Cout,Cin,1) over each of its rows, dkpts (1,N,2) per coordinate; dscores and the (C) vectors whole (1)"""
    if name == "out":
        return a.sum((0, 2))
    if name == "dkpts":
        return a.sum((0, 1))
    return a.sum((1, 2)) if a.ndim == 3 else a.sum(keepdims=True).reshape(1)


def reference_bn_relu(MLP, seed, shape, training, dtype):
    """seq[2](seq[1](x)) of the reference's MLP([C, C, C]) -> (dict of float64 arrays, the pre-activation)"""
    B, C, N = shape
    x, gamma, beta, dy = R.case(seed, B, C, N)
    seq = MLP([C, C, C]).to(dtype)
    bn, relu = seq[1], seq[2]
    assert isinstance(bn, torch.nn.BatchNorm1d) and isinstance(relu, torch.nn.ReLU)
    state = {"weight": torch.from_numpy(gamma).to(dtype), "bias": torch.from_numpy(beta).to(dtype)}
    if not training:
        rm, rv = R.running(seed, C)
        state.update({"running_mean": torch.from_numpy(rm).to(dtype), "running_var": torch.from_numpy(rv).to(dtype)})
    bn.load_state_dict(state, strict=False)
    bn.train(training)
    xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
    z = bn(xt)
    y = relu(z)
    (y * torch.from_numpy(dy).to(dtype)).sum().backward()
    res = {"y": y.detach(), "dx": xt.grad, "dgamma": bn.weight.grad, "dbeta": bn.bias.grad, "running_mean": bn.running_mean,
           "running_var": bn.running_var}
    return {k: v.double().numpy() for k, v in res.items()}, z.detach().double().numpy(), int(bn.num_batches_tracked)


def build(MLP, name):
    seed0, shape, training = CASES[name]
    for seed in range(seed0, seed0 + 64):
        r64, z64, nbt = reference_bn_relu(MLP, seed, shape, training, torch.float64)
        r32, _, _ = reference_bn_relu(MLP, seed, shape, training, torch.float32)
        if R.kink(z64).any() or not all(np.isfinite(a).all() for a in list(r32.values()) + list(r64.values())):
            continue
        fx = {"seed": np.int64(seed), "shape": np.array(shape, np.int64), "refused": np.int64(seed - seed0), "nbt": np.int64(nbt),
              "running_mean": r64["running_mean"], "running_var": r64["running_var"]}
        for t in TENSORS:
            pos = sample_positions(name, t, r64[t].size)
            fx.update({f"{t}_g": r64[t].reshape(-1)[pos], f"{t}_d32": (r32[t] - r64[t]).reshape(-1)[pos].astype(np.float32),
                       f"{t}_sum": channel_sums(t, r64[t])})
        return fx
    return f"no seed from {seed0} passed"


def kenc_run(KeypointEncoder, seed, dtype):
    _, d, layers, N = KENC
    m = KeypointEncoder(d, list(layers)).train()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in R.kenc_parameters(seed, m).items()}, strict=False)
    m = m.to(dtype)
    kpts, scores, dy = (torch.from_numpy(a).to(dtype) for a in R.kenc_case(seed, N, d))
    res = {}
    zs = R.bn_outputs(m, lambda: res.update(R.kenc_grads(m, m, kpts, scores, dy)))
    bns = [mod for mod in m.encoder if isinstance(mod, torch.nn.BatchNorm1d)]
    return {k: v.double().numpy() for k, v in res.items()}, zs, bns


def build_kenc(KeypointEncoder):
    seed0 = KENC[0]
    for seed in range(seed0, seed0 + 64):
        r64, zs, bns = kenc_run(KeypointEncoder, seed, torch.float64)
        r32, _, _ = kenc_run(KeypointEncoder, seed, torch.float32)
        if any(R.kink(z.numpy()).any() for z in zs) or not all(np.isfinite(a).all() for a in list(r32.values()) + list(r64.values())):
            continue
        assert len(r64) == 3 + 14 and len(bns) == 3
        fx = {"seed": np.int64(seed), "refused": np.int64(seed - seed0), "names": np.array(list(r64)),
              "nbt": np.array([int(b.num_batches_tracked) for b in bns], np.int64)}
        for i, b in enumerate(bns):
            fx.update({f"running_mean_{i}": b.running_mean.numpy().copy(), f"running_var_{i}": b.running_var.numpy().copy()})
        for i, (name, a) in enumerate(r64.items()):
            pos = kenc_positions(i, a.size)
            fx.update({f"{name}_g": a.reshape(-1)[pos], f"{name}_d32": (r32[name] - a).reshape(-1)[pos].astype(np.float32),
                       f"{name}_sum": kenc_sums(name, a)})
        return fx
    return f"no seed from {seed0} passed"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    from superglue.models.superglue_train import MLP, KeypointEncoder     # noqa: E402  (the reference's, unchanged)
    refused = []
    for name, fx in [(n, build(MLP, n)) for n in CASES] + [("kenc", build_kenc(KeypointEncoder))]:
        if isinstance(fx, str):
            print(f"bngrad_{name}.npz REFUSED: {fx}")
            refused.append(name)
            continue
        path = os.path.join(HERE, f"bngrad_{name}.npz")
        np.savez_compressed(path, **fx)
        size = os.path.getsize(path)
        assert size < 75000, f"{path}: {size} bytes"
        assert int(fx["refused"]) <= MAX_REFUSED, f"{name}: {int(fx['refused'])} seeds refused"
        print(f"bngrad_{name}.npz: {size} bytes, {len(fx)} arrays, seed {int(fx['seed'])}, {int(fx['refused'])} seeds refused")
    assert not refused, f"committed cases were refused: {refused}"


if __name__ == "__main__":
    main()
