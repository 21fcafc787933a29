"""Writes the 1x1-convolution forward / backward fixtures from the REFERENCE's own MLP and AttentionalPropagation under torch.autograd
(imported unchanged; never runs where the reference is absent):

    python tests/golden/make_golden_lingrad.py --reference /path/to/reference

For every item of CASES it builds the seeded x0, x1, w, bias and dy (tests/lingrad_ref.py: case, integer hashing; the items of a file
share the weights of its first seed, so that `ragged` can run as one batch), loads w and bias into
the reference's MLP([C0+C1, Cout]) (superglue/models/superglue_train.py:45-57: exactly one nn.Conv1d with bias), runs it on
torch.cat([x0, x1], 1) in fp32 and float64 on the CPU, differentiates sum(y * dy) with torch.autograd, and writes lingrad_<case>.npz.
The inputs are NOT stored: the tests re-derive them from the seed.  Per item k of a file, and per tensor t of y, dx, dw, db:

  seed_k, shape_k = (Cout, C0, C1, N)  the recipe's arguments (B = 1)
  t_g_k, t_d32_k                       the float64 value at sample_positions(), and the reference's fp32 value minus it at the same positions
  t_sum_k                              a float64 sum per channel: y (Cout) and dx (C0+C1) over the columns, dw (Cout) over each of its rows,
                                       db whole (1)

The thousand positions per tensor of a file are shared out over its items; they are drawn from the file's first seed, so the items of
`ragged` (one shape of dw and db) are sampled at the same places and their float64 values can be added: the gradient is linear in the
pairs.  lingrad_layer.npz holds the reference's AttentionalPropagation(128, 4) in .train() mode with seeded parameters
(tests/lingrad_ref.py: layer_parameters, layer_case): the output, dx, dsource and the gradients of all 14 parameters, at up to 200
positions per tensor (t_g, t_d32) with one float64 sum per tensor (t_sum).  A seed is refused when any reference result holds a
non-finite value; main() asserts that no committed case was refused."""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import lingrad_ref as R   # noqa: E402

N_SAMPLE = 1000
N_SAMPLE_LAYER = 200
TENSORS = ("y", "dx", "dw", "db")
RAGGED_FRAME = 64                                 # the N the ragged batch is padded to
# file -> items (seed, Cout, C0, C1, N)
CASES = {
    "proj": [(1, 128, 128, 0, 70)],
    "mlp0": [(2, 256, 128, 128, 100)],
    "kenc0": [(3, 32, 3, 0, 50)],
    "d64": [(4, 64, 128, 0, 45)],
    "ragged": [(5, 128, 64, 64, 60), (6, 128, 64, 64, 33), (7, 128, 64, 64, 1)],
}
LAYER = (8, 128, 4, 70, 100)                      # seed, feature_dim, heads, N, M


def sample_positions(seed, tensor, size, n_items=1):
    """the fixed pseudo-random sample of flat positions of one tensor of one file (the tests call this too); seed = the file's first"""
    return np.sort(np.random.default_rng([int(seed), 23, TENSORS.index(tensor)]).choice(size, min(N_SAMPLE // n_items, size), replace=False))


def layer_positions(seed, index, size):
    return np.sort(np.random.default_rng([int(seed), 29, int(index)]).choice(size, min(N_SAMPLE_LAYER, size), replace=False))


def channel_sums(t, a):
    """a: the float64 array of tensor t of one item (B = 1)"""
    return {"y": lambda: a[0].sum(1), "dx": lambda: a[0].sum(1), "dw": lambda: a.sum(1), "db": lambda: a.sum(keepdims=True)}[t]()


def reference_conv(MLP, x0, x1, w, bias, dy, dtype):
    """the reference's MLP([Cin, Cout]) with w and bias loaded, on cat([x0, x1], 1) -> y, dx, dw, db as float64 arrays"""
    m = MLP([w.shape[1], w.shape[0]]).to(dtype)
    assert len(m) == 1 and isinstance(m[0], torch.nn.Conv1d)
    m.load_state_dict({"0.weight": torch.from_numpy(w)[:, :, None].to(dtype), "0.bias": torch.from_numpy(bias).to(dtype)})
    x = torch.from_numpy(x0 if x1 is None else np.concatenate([x0, x1], 1)).to(dtype).requires_grad_(True)
    y = m(x)
    (y * torch.from_numpy(dy).to(dtype)).sum().backward()
    return {"y": y.detach().double().numpy(), "dx": x.grad.double().numpy(), "dw": m[0].weight.grad[:, :, 0].double().numpy(),
            "db": m[0].bias.grad.double().numpy()}


def build(MLP, items):
    fx = {"n_items": np.int64(len(items))}
    for i, (seed, Cout, C0, C1, N) in enumerate(items):
        x0, x1, w, bias, dy = R.case(seed, 1, Cout, C0, C1, N, wseed=items[0][0])     # one file, one set of weights
        r32, r64 = reference_conv(MLP, x0, x1, w, bias, dy, torch.float32), reference_conv(MLP, x0, x1, w, bias, dy, torch.float64)
        if not all(np.isfinite(a).all() for a in list(r32.values()) + list(r64.values())):
            return f"seed {seed}: a result of the reference holds a non-finite value"
        fx.update({f"seed_{i}": np.int64(seed), f"shape_{i}": np.array([Cout, C0, C1, N], np.int64)})
        for t in TENSORS:
            pos = sample_positions(items[0][0], t, r64[t].size, len(items))
            fx.update({f"{t}_g_{i}": r64[t].reshape(-1)[pos], f"{t}_d32_{i}": (r32[t] - r64[t]).reshape(-1)[pos].astype(np.float32),
                       f"{t}_sum_{i}": channel_sums(t, r64[t])})
    return fx


def build_layer(AttentionalPropagation):
    seed, d, heads, N, M = LAYER
    res = {}
    for dtype in (torch.float32, torch.float64):
        m = AttentionalPropagation(d, heads).train()
        m.load_state_dict({k: torch.from_numpy(v) for k, v in R.layer_parameters(seed, m).items()}, strict=False)
        m = m.to(dtype)
        x, source, dy = (torch.from_numpy(a).to(dtype) for a in R.layer_case(seed, d, N, M))
        res[dtype] = {k: v.double().numpy() for k, v in R.layer_grads(m, m, x, source, dy).items()}
    r32, r64 = res[torch.float32], res[torch.float64]
    if not all(np.isfinite(a).all() for a in list(r32.values()) + list(r64.values())):
        return f"seed {seed}: a result of the reference holds a non-finite value"
    assert len(r64) == 3 + 14                      # out, dx, dsource and every parameter of the module (4 + 2 convolutions and the BatchNorm, weight and bias)
    fx = {"seed": np.int64(seed), "shape": np.array([d, heads, N, M], np.int64), "names": np.array(list(r64))}
    for i, (name, a) in enumerate(r64.items()):
        pos = layer_positions(seed, i, a.size)
        fx.update({f"{name}_g": a.reshape(-1)[pos], f"{name}_d32": (r32[name] - a).reshape(-1)[pos].astype(np.float32), f"{name}_sum": a.sum(keepdims=True).reshape(1)})
    return fx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    from superglue.models.superglue_train import MLP, AttentionalPropagation     # noqa: E402  (the reference's, unchanged)
    refused = []
    for name, fx in [(n, build(MLP, items)) for n, items in CASES.items()] + [("layer", build_layer(AttentionalPropagation))]:
        if isinstance(fx, str):
            print(f"lingrad_{name}.npz REFUSED: {fx}")
            refused.append(name)
            continue
        path = os.path.join(HERE, f"lingrad_{name}.npz")
        np.savez_compressed(path, **fx)
        size = os.path.getsize(path)
        assert size < 75000, f"{path}: {size} bytes"
        print(f"lingrad_{name}.npz: {size} bytes, {len(fx)} arrays")
    assert not refused, f"committed cases were refused: {refused}"


if __name__ == "__main__":
    main()
