"""SuperPoint descriptor training on the GPU (imx_warp_labels, imx_erode_mask, imx_detector_loss, imx_desc_pairs,
imx_desc_loss_sparse, Engine.sp_train_losses, the CLI) against the fixtures the reference wrote
(tests/golden/make_golden_sptrain.py) and the project's restatement (tests/sptrain_ref.py, itself held to the fixtures by
tests/test_sptrain_host.py).  Index outputs are compared for equality: the generator refused every seed with a decision closer
to flipping than two fp32 evaluation orders can differ.  Needs an MI355X; each test takes a few seconds at the most."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import sptrain_ref as R
from tests import util
from tests.golden.make_golden_sptrain import DIMS, LAMDA_D, MARGIN, SETTINGS, desc_maps

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ("sptrain_120x160_s1.npz", "sptrain_120x160_s2.npz")
ODD = ("sptrain_136x200_s2.npz", "sptrain_136x200_s3.npz")
D = 128


@pytest.fixture(scope="module")
def fx():
    return {n: util.golden(n) for n in SMALL + ODD}


def new_engine(weights=False, d=D):
    from image_matching_amd import _lib as L
    from image_matching_amd.engine import Engine
    eng = Engine(util.sp_config(d, 256), util.sg_config(d), "cuda")
    if weights:
        eng.load_state_dict(L.NET_SUPERPOINT, util.sp_sd(d))
    return eng


@pytest.fixture(scope="module")
def eng():
    return new_engine(weights=True)


def cuda(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def close(a, b):
    """the project's bar: |a - b| <= 1e-4 + 1e-4 |b|; NaN only where both are"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.all((np.abs(a - b) <= 1e-4 + 1e-4 * np.abs(b)) | (np.isnan(a) & np.isnan(b))))


def same_bits(a, b):
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------- imx_warp_labels
def labels_ref(pts_rows, mats_px, H, W):
    out = [R.warp_labels(p, m, H, W) for p, m in zip(pts_rows, mats_px)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def check_labels(eng, pts_rows, mats_px, H, W, tag):
    B, cap = len(pts_rows), max(1, max(len(p) for p in pts_rows)) + 3
    pts = np.full((B, cap, 2), np.nan, np.float32)                      # rows past the count: poisoned, never read
    for b, p in enumerate(pts_rows):
        pts[b, :len(p)] = p
    counts = torch.tensor([len(p) for p in pts_rows], dtype=torch.int32).cuda()
    labels, res, _ = eng.warp_labels(cuda(pts), counts, cuda(np.stack(mats_px)), H, W, pixel_space=True)
    want_l, want_r = labels_ref(pts_rows, mats_px, H, W)
    labels, res = labels.cpu().numpy(), res.cpu().numpy()
    assert np.array_equal(labels, want_l), f"{tag}: label map"
    assert np.array_equal(res != 0, want_r != 0), f"{tag}: residual support"
    xs, ys = np.broadcast_to(np.arange(W, dtype=np.float32), (B, H, W)), np.broadcast_to(np.arange(H, dtype=np.float32)[:, None], (B, H, W))
    coord = np.abs(np.stack([xs, ys], 1) + want_r)                      # the unrounded coordinate behind every residual
    ulp = np.abs(res.astype(np.float64) - want_r) / np.spacing(np.maximum(coord, np.float32(1e-30)).astype(np.float32))
    print(f"{tag}: {int(want_l.sum())} labels, residuals at most {ulp.max():.2f} ulp of the coordinate from the restatement")
    assert ulp.max() <= 1.0, f"{tag}: residual {ulp.max()} ulp of the coordinate away"
    return labels, res


@pytest.mark.parametrize("names", (SMALL, ODD))
def test_warp_labels_on_the_fixtures(eng, fx, names):
    ga, gb = fx[names[0]], fx[names[1]]
    H, W = (int(v) for v in ga["size"])
    ma, mb = R.scale_pixels(ga["homography"], H, W)[0], R.scale_pixels(gb["homography"], H, W)[0]
    one, _ = check_labels(eng, [ga["pts"]], [ma], H, W, names[0])
    assert np.array_equal(one[0], ga["warped_labels"]), "the reference's own label map"
    three, res3 = check_labels(eng, [ga["pts"], gb["pts"][:70], gb["pts"][:0]], [ma, mb, mb], H, W, "ragged batch of 3")
    assert np.array_equal(three[0], ga["warped_labels"]) and three[2].sum() == 0 and res3[2].any() == 0
    assert np.array_equal(res3[0][:, ga["warped_labels"] == 1], ga["warped_res"]), "the reference's own residuals, bit for bit"
    # the same through the normalised matrices (the host forms the pixel-space product with the reference's expression)
    lab, res, _ = eng.warp_labels(cuda(ga["pts"][None]), None, torch.from_numpy(ga["homography"][None]), H, W)
    assert np.array_equal(lab[0].cpu().numpy(), ga["warped_labels"]) and np.array_equal(res[0].cpu().numpy(), res3[0])


def test_warp_labels_crafted(eng):
    H, W = 24, 40
    eye = np.eye(3, dtype=np.float32)

    def shifted(dx, dy):
        m = eye.copy()
        m[0, 2], m[1, 2] = dx, dy
        return m
    grid = np.array([[x + 0.7, y + 0.2] for y in range(0, H, 3) for x in range(0, W, 3)], np.float32)
    lab, res = check_labels(eng, [grid], [shifted(3, 2)], H, W, "integer translation")
    assert lab[0, 2, 3] == 1 and not res.any()
    lab, res = check_labels(eng, [grid], [shifted(0.5, 1.5)], H, W, "half-pixel translation")
    assert lab[0, 2, 0] == 1 and lab[0, 2, 4] == 1 and lab[0, 2, 3] == 0          # 0.5 -> 0, 3.5 -> 4: half to even
    assert res[0, 0, 2, 0] == 0.5 and res[0, 0, 2, 4] == -0.5
    lab, _ = check_labels(eng, [grid], [shifted(30.25, -7.5)], H, W, "points that leave the image")
    assert 0 < lab.sum() < len(grid) / 2
    persp = eye.copy()
    persp[2, 0], persp[2, 2] = -1.0 / 12, 1.0                                        # w crosses zero inside the image: inf / NaN are dropped
    check_labels(eng, [grid], [persp], H, W, "perspective through w = 0")
    sc = eye.copy()
    sc[0, 0] = 0.25
    lab, res = check_labels(eng, [np.array([[4, 1], [7, 9], [5, 1], [6, 1]], np.float32)], [sc], H, W, "several points on one pixel")
    # x = 4, 5 -> 1.0, 1.25: both on pixel 1 of row 1, index 2 writes the residual; x = 6 -> 1.5 -> 2 (even); x = 7 -> 1.75 -> 2 on row 9
    assert lab.sum() == 3 and res[0, 0, 1, 1] == 0.25 and res[0, 0, 1, 2] == -0.5 and res[0, 0, 9, 2] == -0.25


def test_points_to_2d_and_the_flag(eng, fx):
    g = fx[SMALL[0]]
    H, W = (int(v) for v in g["size"])
    pts = np.full((2, len(g["pts"]) + 5, 2), np.nan, np.float32)
    pts[0, :len(g["pts"])] = g["pts"]
    pts[1, :4] = [[3.9, 2.1], [0.0, 0.0], [W - 0.5, H - 0.5], [W - 1.0, 5.0]]
    counts = torch.tensor([len(g["pts"]), 4], dtype=torch.int32).cuda()
    lab, res, flag = eng.warp_labels(cuda(pts), counts, None, H, W)
    lab = lab.cpu().numpy()
    assert int(flag) == 0 and np.array_equal(lab[0], g["labels"]) and not res.any()
    want, _ = R.points_to_2d(pts[1, :4], H, W)
    assert np.array_equal(lab[1], want) and lab[1].sum() == 4
    pts[1, 1] = [W, 3]                                                   # one pixel outside: flagged, written nowhere
    lab, _, flag = eng.warp_labels(cuda(pts), counts, None, H, W, want_res=False)
    want, f = R.points_to_2d(pts[1, :4], H, W)
    assert int(flag) == 1 == f and np.array_equal(lab[1].cpu().numpy(), want) and want.sum() == 3
    pts[1, 1] = [np.nan, 3]
    assert int(eng.warp_labels(cuda(pts), counts, None, H, W, want_res=False)[2]) == 1
    assert int(eng.warp_labels(cuda(pts[:1]), counts[:1], None, H, W, want_res=False)[2]) == 0     # the flag is zeroed by every call


# ---------------------------------------------------------------------------------------------- imx_erode_mask
def test_erode_mask(eng, fx):
    for names in (SMALL, ODD):
        masks = np.stack([fx[n]["warped_valid_mask"] for n in names]).astype(np.float32)
        assert 0 < masks.mean() < 1
        m = cuda(masks)
        assert torch.equal(eng.erode_mask(m, 0), m)
        for r in (1, 2, 3):
            got = eng.erode_mask(m, r).cpu().numpy()
            assert np.array_equal(got, R.erode(masks, r)), f"radius {r} at {masks.shape}"
            assert got.sum() < masks.sum()
    one = np.ones((1, 8, 8), np.float32)
    one[0, 4, 4] = 0
    for shape_mask in (one, np.pad(one, ((0, 0), (64, 64), (96, 96)), constant_values=1)):
        for r in (1, 3):
            assert np.array_equal(eng.erode_mask(cuda(shape_mask), r).cpu().numpy(), R.erode(shape_mask, r))
    corner = np.ones((1, 8, 8), np.float32)
    assert eng.erode_mask(cuda(corner), 3).min() == 1                    # pixels outside the image take no part
    grey = np.random.default_rng(0).random((2, 17, 23)).astype(np.float32)
    assert np.array_equal(eng.erode_mask(cuda(grey), 2).cpu().numpy(), R.erode(grey, 2))


# ---------------------------------------------------------------------------------------------- imx_detector_loss
def check_det(eng, semi, labels, mask, tag, ref32=None):
    got = eng.detector_loss(cuda(semi), cuda(labels), cuda(mask)).cpu().numpy().astype(np.float64)
    f64, msum = R.detector_loss(semi, labels, mask)
    if ref32 is None:
        ref32 = R.detector_loss(semi, labels, mask, torch.float32, conditioned=False)[0]
    bound = max(1e-4 + 1e-4 * abs(f64), 2.5 * abs(ref32 - f64))
    print(f"{tag}: hip {got[0]:.8f} f64 {f64:.8f} ref32 {ref32:.8f}: |hip - f64| = {abs(got[0] - f64):.3e} of a bound {bound:.3e} "
          f"(reference's own distance {abs(ref32 - f64):.3e})")
    assert abs(got[0] - f64) <= bound, tag
    assert abs(got[1] - msum) <= 1e-6 * max(msum, 1), tag
    return got


@pytest.mark.parametrize("names", (SMALL, ODD))
def test_detector_loss_on_the_fixtures(eng, fx, names):
    for n in names:
        g = fx[n]
        labels = np.stack([g["labels"], g["warped_labels"]]).astype(np.float32)
        mask = np.stack([np.ones_like(g["warped_valid_mask"]), g["warped_valid_mask"]]).astype(np.float32)
        got = check_det(eng, g["semi"], labels, mask, n, ref32=g["det_loss_f32"][2])
        assert abs(got[0] - g["det_loss_f64"][2]) <= 1e-4 + 1e-4 * abs(g["det_loss_f64"][2]), "the reference's own float64 value"
        for i in (0, 1):
            one = check_det(eng, g["semi"][i:i + 1], labels[i:i + 1], mask[i:i + 1], f"{n}[{i}]", ref32=g["det_loss_f32"][i])
            assert close(one[0], g["det_loss_f32"][i]) and close(one[0], g["det_loss_f64"][i])
    rng = np.random.default_rng(3)
    H, W = (int(v) for v in fx[names[0]]["size"])
    for scale in (1.0, 3.0, 6.0):
        semi = (rng.standard_normal((2, 65, H // 8, W // 8)) * scale).astype(np.float32)
        labels = (rng.random((2, H, W)) < 0.01).astype(np.float32)
        mask = np.ones((2, H, W), np.float32)
        mask[1, :, : W // 3] = 0
        check_det(eng, semi, labels, mask, f"random logits of scale {scale} at {H}x{W}")


def test_detector_loss_cells(eng):
    rng = np.random.default_rng(5)
    semi = (rng.standard_normal((1, 65, 1, 1)) * 3).astype(np.float32)
    ones = np.ones((1, 8, 8), np.float32)
    for k in (0, 1, 2, 3):                                               # a single cell with k labels
        labels = np.zeros((1, 8, 8), np.float32)
        labels.reshape(-1)[[5, 17, 60][:k]] = 1
        check_det(eng, semi, labels, ones, f"one cell, {k} labels")
    H, W = 24, 40
    semi = (rng.standard_normal((2, 65, 3, 5)) * 4).astype(np.float32)
    blurred = rng.random((2, H, W)).astype(np.float32) * (rng.random((2, H, W)) < 0.05)      # a non-binary label map
    check_det(eng, semi, blurred, np.ones((2, H, W), np.float32), "blurred labels")
    got = eng.detector_loss(cuda(semi), cuda(blurred), cuda(np.zeros((2, H, W), np.float32))).cpu().numpy()
    assert got[0] == 0 and got[1] == 0, "mask zero everywhere: exactly 0"
    holes = np.ones((2, H, W), np.float32)
    holes[:, 3::8, 4::8] = 0                                             # one zero pixel per cell
    got = eng.detector_loss(cuda(semi), cuda(blurred), cuda(holes)).cpu().numpy()
    assert got[0] == 0 and got[1] == 0
    part = np.ones((2, H, W), np.float32)
    part[0, :8] = 0
    part[1, 11, 20] = 0.5                                                # a grey mask value scales its cell
    check_det(eng, semi, blurred, part, "partial mask")


def test_detector_loss_large_gaps_follow_float64(eng):
    """gaps of exactly 0, 40, 120 and 200 below the maximum, held to the float64 value of the conditioned evaluation (the written
    softmax-BCE rounds p to 1 beyond a gap of ~36 in float64 too: tests/test_sptrain_host.py)"""
    semi = np.full((1, 65, 1, 4), -200.0, np.float32)
    semi[0, 0], semi[0, 1], semi[0, 2] = 0.0, -40.0, -120.0
    semi[0, :, 0, 3] += 17.0                                             # a shift of every logit changes nothing
    labels = np.zeros((1, 8, 32), np.float32)
    labels[0, 0, 0] = 1                                                  # cell 0: the label on the maximum
    labels[0, 0, 8 + 1] = 1                                              # cell 1: on the channel 40 below
    labels[0, 0, 16 + 2] = 1                                             # cell 2: on the channel 120 below (-log p clamps at 100; the maximum's complement is still e^-40)
    labels[0, 0, 24 + 1] = 1                                             # cell 3: as cell 1, shifted logits
    ones = np.ones((1, 8, 32), np.float32)
    for c, want in enumerate((0.0, 80.0, 140.0, 80.0)):
        sl = slice(8 * c, 8 * c + 8)
        f64, _ = R.detector_loss(semi[..., c:c + 1], labels[..., sl], ones[..., sl])
        got = float(eng.detector_loss(cuda(semi[..., c:c + 1]), cuda(labels[..., sl]), cuda(ones[..., sl]))[0])
        print(f"cell {c}: hip {got:.6f} f64 {f64:.6f}")
        assert abs(f64 - want) < 1e-6 and abs(got - f64) <= 1e-4 + 1e-4 * abs(f64)
    check_det(eng, semi, labels, ones, "all four cells", ref32=R.detector_loss(semi, labels, ones)[0])


# ---------------------------------------------------------------------------------------------- imx_desc_loss_sparse
def desc_case(g, d, si):
    H, W = (int(v) for v in g["size"])
    da, db = desc_maps(int(g["seed"]), d, H // 8, W // 8)
    return da, db, g[f"choice_{si}"].astype(np.int32), g[f"nonmatch_{si}"].astype(np.int32)


@pytest.mark.parametrize("name", SMALL + ODD)
def test_desc_loss_on_the_fixtures(eng, fx, name):
    g = fx[name]
    H, W = (int(v) for v in g["size"])
    Hc, Wc = H // 8, W // 8
    hom = torch.from_numpy(g["homography"][None])
    pairs, nv = eng.desc_pairs(hom, Hc, Wc)
    n = int(g["n_valid"])
    pairs = pairs[0].cpu().numpy()
    assert int(nv) == n and np.array_equal(pairs[:n, 0], g["pair_a"]) and np.array_equal(pairs[:n, 1], g["pair_b"]) and (pairs[n:] == -1).all()
    worst = 0.0
    for si, (M, Rn) in enumerate(SETTINGS):
        for d in DIMS:
            da, db, choice, non = desc_case(g, d, si)
            for method in ("1d", "2d"):
                out = eng.desc_loss_sparse(cuda(da[None]), cuda(db[None]), hom, cuda(choice[None], torch.int32), cuda(non[None], torch.int32),
                                           LAMDA_D, MARGIN, method, want_pairs=True)
                row, mean = out["out"][0].cpu().numpy(), out["mean"].cpu().numpy()
                tag = f"{name} M={M} R={Rn} d={d} {method}"
                assert int(out["flag"]) == 0 and row[4] == n and row[3] == int(g[f"hard_{si}_{d}"]), tag
                assert np.array_equal(out["pairs"][0].cpu().numpy(), pairs), tag
                for ref in (g[f"loss_{si}_{d}_{method}_f32"], g[f"loss_{si}_{d}_{method}_f64"]):
                    assert close(row[:3], ref) and close(mean, ref), f"{tag}: {row[:3]} vs {ref}"
                    worst = max(worst, float(np.max(np.abs(row[:3] - ref) / (1e-4 + 1e-4 * np.abs(ref)))))
    print(f"{name}: at most {worst:.3f} of the 1e-4 + 1e-4 |ref| bar over {len(SETTINGS) * len(DIMS) * 2} cases")


@pytest.mark.parametrize("names", (SMALL, ODD))
def test_desc_loss_batch_of_three(eng, fx, names):
    ga, gb = fx[names[0]], fx[names[1]]
    hom = torch.from_numpy(np.stack([ga["homography"], gb["homography"], ga["homography"]]))
    for si, d, method in ((0, 128, "2d"), (2, 64, "1d"), (1, 256, "2d")):
        cases = [desc_case(ga, d, si), desc_case(gb, d, si), desc_case(ga, d, si)]
        da, db, ch, non = (np.stack([c[k] for c in cases]) for k in range(4))
        out = eng.desc_loss_sparse(cuda(da), cuda(db), hom, cuda(ch, torch.int32), cuda(non, torch.int32), LAMDA_D, MARGIN, method)
        rows = out["out"].cpu().numpy()
        refs = np.stack([g[f"loss_{si}_{d}_{method}_f64"] for g in (ga, gb, ga)])
        assert close(rows[:, :3], refs) and close(out["mean"].cpu().numpy(), refs.mean(0))
        assert np.array_equal(rows[0], rows[2]) and list(rows[:, 4]) == [int(ga["n_valid"]), int(gb["n_valid"]), int(ga["n_valid"])]
        one = eng.desc_loss_sparse(cuda(da[1:2]), cuda(db[1:2]), hom[1:2], cuda(ch[1:2], torch.int32), cuda(non[1:2], torch.int32), LAMDA_D, MARGIN, method)
        assert torch.equal(one["out"][0], out["out"][1]), "an image's losses do not depend on its batch"


def one_hot_maps(d, Hc, Wc):
    m = np.zeros((d, Hc * Wc), np.float32)
    m[np.arange(Hc * Wc) % d, np.arange(Hc * Wc)] = 1
    return m.reshape(d, Hc, Wc)


def test_desc_loss_crafted(eng):
    Hc, Wc, d, M, Rn = 9, 13, 64, 100, 8
    N = Hc * Wc
    rng = np.random.default_rng(11)
    eye = np.eye(3, dtype=np.float32)
    maps = one_hot_maps(d, Hc, Wc)
    choice = rng.integers(0, N, (1, M)).astype(np.int32)
    non = rng.integers(0, N, (1, M, Rn)).astype(np.int32)
    run = lambda da, db, h, ch, nm, method="1d": eng.desc_loss_sparse(cuda(da), cuda(db), cuda(h), cuda(ch, torch.int32), cuda(nm, torch.int32), 1.0, MARGIN,
                                                                   method, want_pairs=True, cell_space=True)
    # identity: every cell matches itself; identical one-hot maps give a 1d match loss of exactly 0
    out = run(maps[None], maps[None], eye[None], choice, non)
    row = out["out"][0].cpu().numpy()
    pr = out["pairs"][0].cpu().numpy()
    assert row[4] == N and np.array_equal(pr[:, 0], np.arange(N)) and np.array_equal(pr[:, 1], np.arange(N)) and row[1] == 0.0
    ref = R.desc_loss(maps, maps, pr[:, 0], pr[:, 1], choice[0], non[0], 1.0, MARGIN, "1d")
    assert close(row[:3], ref[:3]) and row[3] == ref[3] and ref[3] > 0
    ref2 = R.desc_loss(maps, maps, pr[:, 0], pr[:, 1], choice[0], non[0], 1.0, MARGIN, "2d")
    assert close(run(maps[None], maps[None], eye[None], choice, non, "2d")["out"][0].cpu().numpy()[:3], ref2[:3]) and ref2[1] > 0
    # a translation by a cell and a half: x + 1.5 rounds half to even (1.5 -> 2, 2.5 -> 2, 12.5 -> 12), the last column leaves
    half = eye.copy()
    half[0, 2] = 1.5
    pa, pb = R.desc_pairs(half, Hc, Wc)
    out = run(maps[None], maps[None], half[None], choice % len(pa), non)
    pr = out["pairs"][0].cpu().numpy()
    assert out["out"][0, 4] == len(pa) < N and np.array_equal(pr[:len(pa), 0], pa) and np.array_equal(pr[:len(pa), 1], pb) and (pr[len(pa):] == -1).all()
    assert pb[0] == 2 and pb[1] == 2 and pb[11] == 12 and len(pa) == N - Hc
    # a matrix that sends every cell outside: NaN for that image only, its neighbours as if alone
    away = eye.copy()
    away[0, 2] = 1000.0
    da = rng.standard_normal((3, d, Hc, Wc)).astype(np.float32)
    da /= np.sqrt((da * da).sum(1, keepdims=True))
    db = np.roll(da, 1, 0).copy()
    ch3, nm3 = np.repeat(choice % len(pa), 3, 0), np.repeat(non, 3, 0)
    out = run(da, db, np.stack([half, away, eye]), ch3, nm3, "2d")
    rows = out["out"].cpu().numpy()
    assert int(out["flag"]) == 0 and rows[1, 4] == 0 and np.isnan(rows[1, :3]).all() and rows[1, 3] == 0 and np.isnan(out["mean"].cpu().numpy()).all()
    assert (out["pairs"][1] == -1).all()
    for b, h in ((0, half), (2, eye)):
        alone = run(da[b:b + 1], db[b:b + 1], h[None], ch3[b:b + 1], nm3[b:b + 1], "2d")
        assert torch.equal(alone["out"][0], out["out"][b]) and np.isfinite(rows[b]).all()
    # a choice index past n_valid and a non-match index outside the map: flagged, not read through
    bad = choice % len(pa)
    bad[0, 3] = len(pa)
    out = run(maps[None], maps[None], half[None], bad, non)
    assert int(out["flag"]) == 1 and np.isfinite(out["out"].cpu().numpy()).all()
    bad_nm = non.copy()
    bad_nm[0, 5, 2], bad_nm[0, 7, 0] = N, -1
    out = run(maps[None], maps[None], half[None], choice % len(pa), bad_nm)
    assert int(out["flag"]) == 2 and np.isfinite(out["out"].cpu().numpy()).all()
    assert int(run(maps[None], maps[None], half[None], choice % len(pa), non)["flag"]) == 0


# ---------------------------------------------------------------------------------------------- invariances
def stage_calls(fx):
    """name -> callable(engine) returning a tuple of device tensors; one small and one larger shape of every entry point"""
    calls = {}
    for tag, names in (("small", SMALL), ("odd", ODD)):
        g = fx[names[0]]
        H, W = (int(v) for v in g["size"])
        Hc, Wc = H // 8, W // 8
        hom = torch.from_numpy(np.stack([fx[n]["homography"] for n in names]))
        pts = cuda(np.stack([fx[n]["pts"] for n in names]))
        masks = cuda(np.stack([fx[n]["warped_valid_mask"] for n in names]).astype(np.float32))
        semi = cuda(np.concatenate([fx[n]["semi"][1:] for n in names]))
        labels = cuda(np.stack([fx[n]["warped_labels"] for n in names]).astype(np.float32))
        d = 128 if tag == "small" else 256
        cases = [desc_case(fx[n], d, 0) for n in names]
        da, db, ch, nm = (cuda(np.stack([c[k] for c in cases]), torch.int32 if k > 1 else torch.float32) for k in range(4))
        calls[f"warp_labels_{tag}"] = lambda e, pts=pts, hom=hom, H=H, W=W: e.warp_labels(pts, None, hom, H, W)[:2]
        calls[f"erode_mask_{tag}"] = lambda e, masks=masks: (e.erode_mask(masks, 3),)
        calls[f"detector_loss_{tag}"] = lambda e, semi=semi, labels=labels, masks=masks: (e.detector_loss(semi, labels, masks),)
        calls[f"desc_loss_{tag}"] = lambda e, da=da, db=db, hom=hom, ch=ch, nm=nm: tuple(
            e.desc_loss_sparse(da, db, hom, ch, nm, LAMDA_D, MARGIN, "2d", want_pairs=True)[k] for k in ("out", "mean", "pairs"))
    return calls


def test_results_do_not_depend_on_history(eng, fx):
    calls = stage_calls(fx)
    x = torch.cat(util.pair(3, 120, 160)).cuda()
    forward0 = eng.superpoint_dense(x)
    want = {k: tuple(t.clone() for t in f(eng)) for k, f in calls.items()}
    for k, f in calls.items():
        assert same_bits(f(eng), want[k]), f"{k}: twice"
    for order in (sorted(calls), sorted(calls, reverse=True)):            # after a larger call, and after a smaller one
        for k in order:
            assert same_bits(calls[k](eng), want[k]), f"{k}: after another shape"
    for poison in ("nan", "huge", "zero"):
        eng.set_option("debug_poison", poison)
        for k, f in calls.items():
            assert same_bits(f(eng), want[k]), f"{k}: after debug_poison = {poison}"
    eng.set_option("debug_poison", "off")
    fresh = new_engine()
    fresh.set_option("debug_poison", "nan")
    for k in sorted(calls, reverse=True):
        assert same_bits(calls[k](fresh), want[k]), f"{k}: on a second handle"
    assert same_bits(eng.superpoint_dense(x), forward0), "the dense forward after these calls"


# ---------------------------------------------------------------------------------------------- Engine.sp_train_losses
def test_sp_train_losses(eng, fx):
    names = SMALL
    g0 = fx[names[0]]
    H, W = (int(v) for v in g0["size"])
    Hc, Wc = H // 8, W // 8
    images = torch.cat([util.pair(int(fx[n]["seed"]), H, W)[0] for n in names]).cuda()
    hom = torch.from_numpy(np.stack([fx[n]["homography"] for n in names]))
    inv = torch.from_numpy(np.stack([fx[n]["inv_homography"] for n in names]))
    pts = cuda(np.stack([fx[n]["pts"] for n in names]))
    counts = torch.tensor([150, 90], dtype=torch.int32).cuda()
    ch = cuda(np.stack([fx[n]["choice_0"] for n in names]), torch.int32)
    nm = cuda(np.stack([fx[n]["nonmatch_0"] for n in names]), torch.int32)
    out = eng.sp_train_losses(images, pts, counts, hom, inv, ch, nm, erosion_radius=3, lamda_d=1.0, method="2d", lambda_loss=1.0)
    # the staged calls: bit-identical
    warped = eng.warp_homography(images[:, 0], inv.cuda())
    mask = eng.erode_mask(eng.warp_homography((H, W), inv.cuda(), mode="nearest"), 3)
    labels, _, _ = eng.warp_labels(pts, counts, None, H, W, want_res=False)
    wl, wres, _ = eng.warp_labels(pts, counts, hom, H, W)
    semi, desc = eng.superpoint_dense(torch.cat([images, warped[:, None]]))
    det = eng.detector_loss(semi[:2], labels, torch.ones_like(labels))
    det_w = eng.detector_loss(semi[2:], wl, mask)
    dl = eng.desc_loss_sparse(desc[:2], desc[2:], hom, ch, nm, 1.0, MARGIN, "2d")
    staged = (warped, mask, labels, wl, wres, semi[:2], semi[2:], det[0], det_w[0], dl["mean"][0], det[0] + det_w[0] + 1.0 * dl["mean"][0])
    fused = (out["warped_img"][:, 0], out["warped_valid_mask"], out["labels_2D"], out["warped_labels"], out["warped_res"], out["semi"],
             out["semi_warp"], out["loss_det"], out["loss_det_warp"], out["loss_desc"], out["loss"])
    assert same_bits([t.contiguous() for t in fused], [t.contiguous() for t in staged])
    assert int(out["flag"]) == 0 and 0 < float(mask.mean()) < 1
    # the restatement fed the library's own dense outputs, at the bars of the stage tests
    semi_h, desc_h, mask_h = semi.cpu().numpy(), desc.cpu().numpy(), mask.cpu().numpy()
    lab_h, wl_h = labels.cpu().numpy(), wl.cpu().numpy()
    for b, n in enumerate(names):
        k = int(counts[b])
        assert np.array_equal(lab_h[b], R.points_to_2d(fx[n]["pts"][:k], H, W)[0])
        assert np.array_equal(wl_h[b], R.warp_labels(fx[n]["pts"][:k], R.scale_pixels(fx[n]["homography"], H, W)[0], H, W)[0])
    plain = eng.warp_homography((H, W), inv.cuda(), mode="nearest").cpu().numpy()
    assert np.array_equal(mask_h, R.erode(plain, 3)) and np.mean(plain != np.stack([fx[n]["warped_valid_mask"] for n in names])) <= 1e-4
    for got, s, l, m in ((out["loss_det"], semi_h[:2], lab_h, np.ones_like(lab_h)), (out["loss_det_warp"], semi_h[2:], wl_h, mask_h)):
        f64 = R.detector_loss(s, l, m)[0]
        r32 = R.detector_loss(s, l, m, torch.float32, conditioned=False)[0]
        assert abs(float(got) - f64) <= max(1e-4 + 1e-4 * abs(f64), 2.5 * abs(r32 - f64))
    rows = []
    for b, n in enumerate(names):
        rows.append(R.desc_loss(desc_h[b], desc_h[2 + b], fx[n]["pair_a"], fx[n]["pair_b"], fx[n]["choice_0"], fx[n]["nonmatch_0"].astype(np.int64),
                                1.0, MARGIN, "2d")[:3])
        assert close(out["desc"]["out"][b, :3].cpu().numpy(), rows[-1])
    assert close(float(out["loss_desc"]), np.mean([r[0] for r in rows]))


# ---------------------------------------------------------------------------------------------- the draws and the CLI
def test_device_draws_are_valid(eng, fx):
    from image_matching_amd import sptrain
    g = fx[ODD[0]]
    H, W = (int(v) for v in g["size"])
    Hc, Wc = H // 8, W // 8
    away = np.eye(3, dtype=np.float32)
    away[0, 2] = 50.0
    hom = torch.from_numpy(np.stack([g["homography"], away]))
    gen = torch.Generator(device="cuda").manual_seed(1)
    n = int(g["n_valid"])
    for M in (64, 512):                                                  # crops, and pads with repeats
        choice, non = sptrain.draw(eng, hom, Hc, Wc, M, 10, gen)
        c = choice[0].cpu().numpy()
        assert choice.shape == (2, M) and non.shape == (2, M, 10) and c.min() >= 0 and c.max() < n
        assert len(set(c[:min(M, n)])) == min(M, n), "the first min(M, n_valid) entries are distinct: a permutation"
        assert int(non.min()) >= 0 and int(non.max()) < Hc * Wc
        da, db = desc_maps(1, 64, Hc, Wc)
        out = eng.desc_loss_sparse(cuda(np.stack([da, da])), cuda(np.stack([db, db])), hom, choice, non, 1.0, MARGIN, "2d")
        rows = out["out"].cpu().numpy()
        assert int(out["flag"]) == 0 and np.isfinite(rows[0]).all() and rows[1, 4] == 0 and np.isnan(rows[1, 0])


def test_cli_synthetic():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "superpoint_validate_descriptor.py"), "--synthetic", "2", "--size", "120", "160"],
                       capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    scalars = json.loads(r.stdout.strip().splitlines()[-1])
    assert set(scalars) == {"loss", "loss_det", "loss_det_warp", "positive_dist", "negative_dist", "precision", "recall"}
    assert all(np.isfinite(v) for v in scalars.values()), scalars
    assert 0 <= scalars["precision"] <= 1 and 0 <= scalars["recall"] <= 1 and scalars["loss_det"] > 0
