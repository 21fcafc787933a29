"""Writes the attention forward / backward fixtures from the REFERENCE's own attention() under torch.autograd (imported unchanged; never
runs where the reference is absent):

    python tests/golden/make_golden_mhagrad.py --reference /path/to/reference

For every item of CASES it builds the seeded q, k, v and dout (tests/mhagrad_ref.py: case, integer hashing), runs the reference's
attention (superglue/models/superglue_train.py:82-86) on them in fp32 and float64 on the CPU, differentiates sum(out * dout) with
torch.autograd with respect to query, key and value, and writes mhagrad_<case>.npz.  The inputs are NOT stored: the tests re-derive them
from the seed.  Per item k of a file, and per tensor t of out, dq, dk, dv:

  seed_k, shape_k = (D, H, N, M)     the recipe's arguments (B = 1, gain 1)
  t_g_k, t_d32_k                     the float64 value at sample_positions(), and the reference's fp32 value minus it at the same positions
  t_sum_k (H)                        the float64 sum of t per head (an entry scattered to the wrong place shows)

The thousand positions per tensor of a file are shared out over its items.  A seed is refused when any reference result holds a
non-finite value; main() asserts that no committed case was refused."""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import mhagrad_ref as R   # noqa: E402

N_SAMPLE = 1000
TENSORS = ("out", "dq", "dk", "dv")
RAGGED_FRAME = (60, 64)                           # the (N, M) the ragged batch is padded to
# file -> items (seed, D, H, N, M)
CASES = {
    "d32": [(1, 32, 4, 70, 100)],
    "d64": [(2, 64, 4, 100, 130)],
    "d16": [(3, 16, 4, 50, 45)],
    "ragged": [(4, 32, 4, 60, 37), (5, 32, 4, 33, 64), (6, 32, 4, 1, 50)],
}


def sample_positions(seed, tensor, size, n_items=1):
    """the fixed pseudo-random sample of flat positions of one tensor of one item (the tests call this too)"""
    return np.sort(np.random.default_rng([int(seed), 17, TENSORS.index(tensor)]).choice(size, min(N_SAMPLE // n_items, size), replace=False))


def build(attention, items):
    fx = {"n_items": np.int64(len(items))}
    for i, (seed, D, H, N, M) in enumerate(items):
        q, k, v, dout = R.case(seed, 1, D, H, N, M)
        r32 = R.autograd(q, k, v, dout, torch.float32, fn=attention)
        r64 = R.autograd(q, k, v, dout, torch.float64, fn=attention)
        if not all(np.isfinite(a).all() for a in r32 + r64):
            return f"seed {seed}: a result of the reference holds a non-finite value"
        fx.update({f"seed_{i}": np.int64(seed), f"shape_{i}": np.array([D, H, N, M], np.int64)})
        for t, a32, a64 in zip(TENSORS, r32, r64):
            pos = sample_positions(seed, t, a64.size, len(items))
            fx.update({f"{t}_g_{i}": a64.reshape(-1)[pos], f"{t}_d32_{i}": (a32 - a64).reshape(-1)[pos].astype(np.float32),
                       f"{t}_sum_{i}": a64[0].sum(axis=(0, 2))})
    return fx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    from superglue.models.superglue_train import attention     # noqa: E402  (the reference's, unchanged)
    refused = []
    for name, items in CASES.items():
        fx = build(attention, items)
        if isinstance(fx, str):
            print(f"mhagrad_{name}.npz REFUSED: {fx}")
            refused.append(name)
            continue
        path = os.path.join(HERE, f"mhagrad_{name}.npz")
        np.savez_compressed(path, **fx)
        size = os.path.getsize(path)
        assert size < 75000, f"{path}: {size} bytes"
        print(f"mhagrad_{name}.npz: {size} bytes, {len(fx)} arrays")
    assert not refused, f"committed cases were refused: {refused}"


if __name__ == "__main__":
    main()
