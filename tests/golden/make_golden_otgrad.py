"""Writes the optimal-transport loss-gradient fixtures from the REFERENCE's own autograd (imported unchanged; never runs where the
reference is absent):

    python tests/golden/make_golden_otgrad.py --reference /path/to/reference

For every item of CASES it builds the seeded scores and match list (tests/otgrad_ref.py: case_scores, integer hashing), runs the
reference's log_optimal_transport (superglue/models/superglue_train.py:147-167) on them in fp32 and float64, forms the loss as
:289-299 write it (the mean of -log(exp(Z[x][y])) over the list), differentiates it with torch.autograd with respect to the scores and
bin_score, and writes otgrad_<case>.npz.  Per item k of a file:

  scores_k (m,n) fp32, bin_k, matches_k (2,K) int64, iters_k          the inputs (the scores are the recipe's, bit for bit)
  loss32_k, loss64_k                                                  the reference's value in either precision
  g_k, d32_k          the float64 gradient at sample_positions(), and the reference's fp32 gradient minus it at the same positions
  rows_k, cols_k      the float64 row sums and column sums of the full d scores (an entry scattered to the wrong place shows)
  gbin64_k, gbin32_k  d loss / d bin_score

A seed is refused when the reference's loss is not finite or its gradient holds a NaN (a listed entry whose exp underflows); main()
asserts that no committed case was refused."""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import otgrad_ref as O   # noqa: E402

N_SAMPLE = 1000
BIN_SCORE = 1.0                                   # the reference's initial bin_score Parameter
RAGGED_FRAME = (48, 44)                           # the (N0, N1) the ragged batch is padded to
# file -> items (seed, m, n, iters)
CASES = {
    "pair_s1": [(1, 120, 100, 30)],
    "pair_s2": [(2, 118, 101, 30)],
    "pair_s3": [(3, 123, 97, 30)],
    "iters": [(4, 33, 40, t) for t in (0, 1, 2, 3)],
    "ragged": [(5, 48, 30, 10), (6, 17, 44, 10), (7, 40, 41, 10)],
}


def sample_positions(seed, size):
    """the fixed pseudo-random sample of flat positions of one gradient (the tests call this too)"""
    return np.sort(np.random.default_rng([int(seed), 13]).choice(size, min(N_SAMPLE, size), replace=False))


def reference_grad(lot, scores, matches, iters, dtype):
    S = torch.from_numpy(scores).to(dtype)[None].requires_grad_(True)
    alpha = torch.tensor(BIN_SCORE, dtype=dtype, requires_grad=True)
    Z = lot(S, alpha, iters=iters)
    xs, ys = torch.from_numpy(matches[0]), torch.from_numpy(matches[1])
    loss = torch.mean(-torch.log(Z[0][xs, ys].exp()))
    gs, ga = torch.autograd.grad(loss, (S, alpha))
    return float(loss.detach()), gs[0].double().numpy(), float(ga)


def build(lot, items):
    fx = {"n_items": np.int64(len(items))}
    for k, (seed, m, n, iters) in enumerate(items):
        scores, matches = O.case_scores(seed, m, n)
        l32, g32, b32 = reference_grad(lot, scores, matches, iters, torch.float32)
        l64, g64, b64 = reference_grad(lot, scores, matches, iters, torch.float64)
        if not (np.isfinite(l32) and np.isfinite(l64)) or np.isnan(g32).any() or np.isnan(g64).any() or np.isnan([b32, b64]).any():
            return f"seed {seed}: the reference's loss is not finite or its gradient holds a NaN"
        pos = sample_positions(seed, g64.size)
        fx.update({f"seed_{k}": np.int64(seed), f"scores_{k}": scores, f"bin_{k}": np.float32(BIN_SCORE), f"matches_{k}": matches,
                   f"iters_{k}": np.int64(iters), f"loss32_{k}": np.float64(l32), f"loss64_{k}": np.float64(l64),
                   f"g_{k}": g64.reshape(-1)[pos], f"d32_{k}": (g32 - g64).reshape(-1)[pos].astype(np.float32),
                   f"rows_{k}": g64.sum(1), f"cols_{k}": g64.sum(0), f"gbin64_{k}": np.float64(b64), f"gbin32_{k}": np.float64(b32)})
    return fx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    from superglue.models.superglue_train import log_optimal_transport as lot     # noqa: E402  (the reference's, unchanged)
    refused = []
    for name, items in CASES.items():
        fx = build(lot, items)
        if isinstance(fx, str):
            print(f"otgrad_{name}.npz REFUSED: {fx}")
            refused.append(name)
            continue
        path = os.path.join(HERE, f"otgrad_{name}.npz")
        np.savez_compressed(path, **fx)
        size = os.path.getsize(path)
        assert size < 1000000, f"{path}: {size} bytes"
        print(f"otgrad_{name}.npz: {size} bytes, {len(fx)} arrays")
    assert not refused, f"committed cases were refused: {refused}"


if __name__ == "__main__":
    main()
