"""Writes the loss-gradient fixtures from the REFERENCE's own autograd (imported unchanged; never runs where the reference is absent):

    python tests/golden/make_golden_spgrad.py --reference /path/to/reference

For every committed sptrain_<H>x<W>_s<seed>.npz it imports the reference as make_golden_sptrain.py does (same stubs, same recorded
draws, same seeding seed 100 + si), reruns the reference's own descriptor_loss_sparse and Train_model_heatmap.detector_loss with
requires_grad inputs in fp32 and float64, asserts that the draws and loss values it sees equal the committed ones, and writes
spgrad_<H>x<W>_s<seed>.npz:

  g{a,b}_<si>_<d>_<method>        the float64 gradient of the image's total with respect to desc / desc_warp at sample_positions(), as fp32
  g{a,b}_<si>_<d>_<method>_d32    the reference's fp32 gradient minus the float64 one at the same positions, as fp32
  n{a,b}_<si>_<d>_<method>        the per-cell L1 norm of the float64 gradient, every cell (a row scattered to the wrong cell shows)
  gdet_<case>, gdet_<case>_d32, ndet_<case>   the same for d detector_loss / d semi; case 0 / 1: one image alone, b: the batch of both

Full maps are not committed.  A seed is refused by make_golden_sptrain.py's rules (they held when the sptrain fixture was written) and
by one more: |1 - <a_m, b_m>| < 1e-5 on any match, where the match hinge's decision could flip between evaluations."""
import argparse
import glob
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden.make_golden_sptrain import DIMS, LAMDA_D, MARGIN, SETTINGS, desc_maps, load_reference   # noqa: E402

N_SAMPLE = 1200                                   # positions per tensor (at most 2 000; the files stay under 1 MB)
METHODS = ("1d", "2d")
DET_CASES = ("0", "1", "b")


def sample_positions(seed, key, size):
    """the fixed pseudo-random sample of flat positions of one tensor, seeded by the combination (the tests call this too)"""
    return np.sort(np.random.default_rng([int(seed)] + [int(k) for k in key]).choice(size, min(N_SAMPLE, size), replace=False))


def desc_key(si, d, method, side):
    return (1, si, d, METHODS.index(method), side)


def det_key(case):
    return (2, DET_CASES.index(case))


def put(fx, name, norm_name, seed, key, g32, g64):
    g64, g32 = g64.double().numpy(), g32.double().numpy()
    pos = sample_positions(seed, key, g64.size)
    fx[name] = g64.reshape(-1)[pos].astype(np.float32)
    fx[name + "_d32"] = (g32 - g64).reshape(-1)[pos].astype(np.float32)
    fx[norm_name] = np.abs(g64).sum(-3).astype(np.float32)


def build(ref, path):
    U, DT, SL, SuperPoint, TM = ref
    from tests import spgrad_ref as G
    src = np.load(path)
    seed = int(src["seed"])
    H, W = (int(v) for v in src["size"])
    Hc, Wc = H // 8, W // 8
    hom_t = torch.from_numpy(src["homography"])
    fx = {"seed": np.int64(seed), "size": src["size"]}
    # ---- detector loss: the reference's own function, differentiated by autograd
    semi = torch.from_numpy(src["semi"])
    lab2 = torch.stack([torch.from_numpy(src["labels"]).float(), torch.from_numpy(src["warped_labels"]).float()])[:, None]
    msk2 = torch.stack([torch.ones(H, W), torch.from_numpy(src["warped_valid_mask"]).float()])[:, None]
    grads = {}
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        t3 = U.labels2Dto3D(lab2.to(dt), 8, add_dustbin=True)
        m3 = torch.prod(U.labels2Dto3D(msk2.to(dt), 8, add_dustbin=False), 1)
        vals = []
        for case, sl in (("0", slice(0, 1)), ("1", slice(1, 2)), ("b", slice(0, 2))):
            x = semi[sl].to(dt).clone().requires_grad_(True)
            loss = TM.detector_loss(None, x, t3[sl], m3[sl], "softmax")
            (grads[case, tag],) = torch.autograd.grad(loss, x)
            vals.append(float(loss.detach()))
        assert np.array_equal(np.array(vals, np.float64), src["det_loss_" + tag]), "the detector loss moved"
    for case in DET_CASES:
        put(fx, f"gdet_{case}", f"ndet_{case}", seed, det_key(case), grads[case, "f32"], grads[case, "f64"])
    # ---- sparse descriptor loss: the reference's own function on requires_grad maps, its draws recorded
    pa, pb = src["pair_a"], src["pair_b"]
    drawn = {}
    crop, nonc, gs = SL.crop_or_pad_choice, SL.correspondence_finder.create_non_correspondences, torch.nn.functional.grid_sample

    def rec_crop(*a, **k):
        drawn["choice"] = np.asarray(crop(*a, **k))
        return drawn["choice"]

    def rec_nonc(*a, **k):
        drawn["non"] = nonc(*a, **k)
        return drawn["non"]
    SL.crop_or_pad_choice, SL.correspondence_finder.create_non_correspondences = rec_crop, rec_nonc
    torch.nn.functional.grid_sample = lambda inp, grid, **k: gs(inp, grid.to(inp.dtype), **k)
    try:
        for si, (M, R_) in enumerate(SETTINGS):
            for d in DIMS:
                maps = desc_maps(seed, d, Hc, Wc)
                for method in METHODS:
                    g = {}
                    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
                        da, db = (torch.from_numpy(m).to(dt).requires_grad_(True) for m in maps)
                        np.random.seed(seed * 100 + si)
                        torch.manual_seed(seed * 100 + si)
                        out = SL.descriptor_loss_sparse(da, db, hom_t, device="cpu", lamda_d=LAMDA_D, num_matching_attempts=M,
                                                        num_masked_non_matches_per_match=R_, dist="cos", method=method)
                        choice = drawn["choice"].astype(np.int32)
                        non = (drawn["non"][0] + drawn["non"][1] * Wc).long().numpy().astype(np.int32)
                        assert np.array_equal(src[f"choice_{si}"], choice) and np.array_equal(src[f"nonmatch_{si}"], non), "the draws moved"
                        assert np.array_equal(np.array([float(v.detach()) for v in out], np.float64), src[f"loss_{si}_{d}_{method}_{tag}"]), "the loss moved"
                        g[tag] = torch.autograd.grad(out[0], (da, db))
                    dots = G.match_products(maps[0], maps[1], pa, pb, choice, method)
                    if (np.abs(1 - dots) < 1e-5).any():
                        return f"a match product within 1e-5 of 1 (d = {d}, M = {M}, method {method})"
                    for side, s in enumerate("ab"):
                        put(fx, f"g{s}_{si}_{d}_{method}", f"n{s}_{si}_{d}_{method}", seed, desc_key(si, d, method, side), g["f32"][side], g["f64"][side])
    finally:
        SL.crop_or_pad_choice, SL.correspondence_finder.create_non_correspondences, torch.nn.functional.grid_sample = crop, nonc, gs
    return fx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    a = ap.parse_args()
    ref = load_reference(a.reference)
    for path in sorted(glob.glob(os.path.join(HERE, "sptrain_*.npz"))):
        fx = build(ref, path)
        base = os.path.basename(path)
        if isinstance(fx, str):
            print(f"{base} REFUSED: {fx}")
            continue
        name = base.replace("sptrain_", "spgrad_")
        np.savez_compressed(os.path.join(HERE, name), **fx)
        size = os.path.getsize(os.path.join(HERE, name))
        assert size < 1000000, f"{name}: {size} bytes"
        print(f"{name}: {size} bytes, {len(fx)} arrays")


if __name__ == "__main__":
    main()
