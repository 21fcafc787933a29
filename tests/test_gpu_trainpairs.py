"""SuperGlue training pairs on the GPU (imx_warp_perspective_u8, imx_gt_matches, imx_match_loss, Engine.train_pairs and the
drop-ins) against the fixtures the reference wrote (tests/golden/make_golden_trainpairs.py) and the project's restatement
(tests/trainpairs_ref.py, itself held to the fixtures by tests/test_trainpairs_host.py).  Index outputs are compared for equality
with no case left out: the generator refused every seed with a decision closer than 1e-6 to flipping, and the kernels evaluate the
restatement's float64 expressions operation by operation.  Needs an MI355X; each test takes a few seconds at the most."""
import numpy as np
import pytest
import torch

from tests import trainpairs_ref as R
from tests import util

pytestmark = pytest.mark.gpu
D, CAP = 128, 256
PIPE = ("trainpairs_small.npz", "trainpairs_ragged.npz")


@pytest.fixture(scope="module")
def fx():
    out = {n: util.golden(n) for n in PIPE + ("trainpairs_edge.npz",)}
    for n in PIPE:
        out[n].update(util.golden(n.replace(".npz", "_desc.npz")))
    return out


def new_engine(variant=None, K=CAP, sp=False):
    from image_matching_amd import _lib as L
    from image_matching_amd.engine import Engine
    eng = Engine(util.sp_config(D, K), util.sg_config(D), "cuda")
    if sp:
        eng.load_state_dict(L.NET_SUPERPOINT, util.sp_sd(D))
    if variant:
        eng.load_state_dict(L.NET_SUPERGLUE, util.sg_sd(D, variant=variant))
    return eng


@pytest.fixture(scope="module")
def eng():
    return new_engine("t", sp=True)


def padded(rows, cap, fill=np.nan, dtype=np.float32):
    """(B, cap, ...) from B arrays of differing length, rows past each length filled with `fill`; and the lengths"""
    out = np.full((len(rows), cap) + rows[0].shape[1:], fill, dtype)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return torch.from_numpy(out).cuda(), torch.tensor([len(r) for r in rows], dtype=torch.int32).cuda()


def check_gt(out, b, ref, n0, n1, N0, N1, tag):
    """pair b of Engine.gt_matches' output against gt_matches-style reference arrays"""
    n, na = ref["matches"].shape[1], ref["all_matches"].shape[1]
    assert int(out["n_matches"][b]) == n and int(out["n_all"][b]) == na == n0 + n1 - n, tag
    am = out["all_matches"][b].cpu().numpy()
    assert am.shape == (2, N0 + N1) and np.array_equal(am[:, :na], ref["all_matches"]) and (am[:, na:] == -1).all(), f"{tag}: all_matches"
    gt0, gt1 = np.full(N0, -1, np.int64), np.full(N1, -1, np.int64)
    gt0[ref["matches"][0]], gt1[ref["matches"][1]] = ref["matches"][1], ref["matches"][0]
    assert np.array_equal(out["gt0"][b].cpu().numpy(), gt0) and np.array_equal(out["gt1"][b].cpu().numpy(), gt1), f"{tag}: gt0 / gt1"


def ulp_apart(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b) / np.spacing(np.abs(b)).astype(np.float64)


# ---------------------------------------------------------------------------------------------- warp
@pytest.mark.parametrize("name", PIPE)
def test_warp_equals_the_restatement(eng, fx, name):
    g = fx[name]
    imgs = np.stack([g[f"image_{i}"] for i in range(3)])
    Ms = np.stack([g[f"M_{i}"] for i in range(3)])
    H, W = imgs.shape[1:]
    got = eng.warp_perspective_u8(torch.from_numpy(imgs), Ms).cpu().numpy()
    again = eng.warp_perspective_u8(torch.from_numpy(imgs).cuda(), np.stack([R.invert3(m) for m in Ms]), inverse=True).cpu().numpy()
    assert np.array_equal(got, again)
    for i in range(3):
        listed = {tuple(p) for p in g[f"boundary_{i}"].reshape(-1, 2)}
        assert len(listed) <= 1e-4 * H * W
        diff = {tuple(p) for p in np.argwhere(got[i] != g[f"warped_{i}"])}
        print(f"{name} image {i}: {len(diff)} pixels differ from the reference's warp, {len(listed)} listed on a rounding boundary")
        assert diff <= listed, f"{name} image {i}: pixels {sorted(diff - listed)[:5]} differ away from every rounding boundary (a wrong matrix shows here)"
        exact = R.warp_bilinear_f64(imgs[i], R.invert3(Ms[i]))
        assert np.abs(got[i].astype(np.float64) - exact).max() <= 1.0, f"{name} image {i}: more than one grey level from the exact bilinear value"


# ---------------------------------------------------------------------------------------------- ground truth
@pytest.mark.parametrize("name", PIPE)
def test_gt_matches_equal_the_reference_on_the_pipeline_fixtures(eng, fx, name):
    g = fx[name]
    k0, n0 = padded([g[f"kpts0_{i}"] for i in range(3)], CAP)
    k1, n1 = padded([g[f"kpts1_{i}"] for i in range(3)], CAP)
    Ms = np.stack([g[f"M_{i}"] for i in range(3)])
    out = eng.gt_matches(k0, k1, Ms, n0, n1, want_proj=True)
    for i in range(3):
        ref = {"matches": g[f"matches_{i}"], "all_matches": g[f"all_matches_{i}"]}
        check_gt(out, i, ref, int(n0[i]), int(n1[i]), CAP, CAP, f"{name} sample {i}")
        proj = out["projected"][i, :int(n0[i])].cpu().numpy()
        ulps = ulp_apart(proj, g[f"proj_{i}"]).max()
        print(f"{name} sample {i}: projection at most {ulps:.1f} float32 ulp from the reference's")
        assert ulps <= 1.0


def test_gt_matches_equal_the_reference_on_the_edge_fixture(eng, fx):
    g = fx["trainpairs_edge.npz"]
    for n in (str(x) for x in g["names"]):
        k0, k1 = g[f"kpts0_{n}"], g[f"kpts1_{n}"]
        out = eng.gt_matches(torch.from_numpy(k0)[None], torch.from_numpy(k1)[None], g[f"M_{n}"][None], want_proj=True)      # counts NULL, N0 != N1
        check_gt(out, 0, {"matches": g[f"matches_{n}"], "all_matches": g[f"all_matches_{n}"]}, len(k0), len(k1), len(k0), len(k1), f"edge {n}")
        assert ulp_apart(out["projected"][0].cpu().numpy(), g[f"proj_{n}"]).max() <= 1.0, n
    # a side without keypoints: the skip sample
    k1 = torch.from_numpy(g["kpts1_all"])[None]
    out = eng.gt_matches(torch.full((1, 5, 2), float("nan")), k1, np.eye(3)[None], torch.zeros(1, dtype=torch.int32).cuda(), None)
    assert int(out["n_matches"][0]) == 0 and int(out["n_all"][0]) == 0
    assert (out["gt0"] == -1).all() and (out["gt1"] == -1).all() and (out["all_matches"] == -1).all()


def crafted(counts0, counts1, seed):
    """pairs of scattered points: side 1 holds a shuffled subset of the projections of side 0, each moved by up to 2.5 px, and
    strangers; per pair the restatement's result on the cut arrays.  Refuses (in the test's own name) a draw with a decision within
    1e-6 of flipping -- none of the seeds used here has one."""
    rng = np.random.default_rng(seed)
    M = R.four_point_matrix([[0, 0], [0, 640], [480, 0], [480, 640]], [[14, -9], [-20, 610], [470, 25], [455, 661]])
    k0s, k1s, refs = [], [], []
    for n0, n1 in zip(counts0, counts1):
        p0 = (rng.random((n0, 2)) * [620, 460] + 10).astype(np.float32)
        m = min(n0, n1) * 2 // 3
        near = R.project(p0, M)[rng.permutation(n0)[:m]] + (rng.random((m, 2)) * 5 - 2.5)
        p1 = np.concatenate([near, rng.random((n1 - m, 2)) * [620, 460] + 10])[rng.permutation(n1)].astype(np.float32)
        ref = R.gt_matches(R.project(p0, M), p1)
        mg = R.margins(ref["dists"])
        assert min(v.min() for v in mg.values()) >= 1e-6
        k0s.append(p0), k1s.append(p1), refs.append(ref)
    return k0s, k1s, np.repeat(M[None], len(counts0), 0), refs


# a cap of 67 with a full, a partial and a single-point side in one call; past one 256-thread tile; past 1024; N0 != N1 throughout
SHAPES = {"cap67": (67, 61, (67, 40, 1), (40, 61, 33)), "cap300": (300, 280, (300, 257, 256), (280, 255, 1)), "cap1100": (1100, 1030, (1100, 1025), (1024, 1030))}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_gt_matches_at_the_shapes_where_the_kernels_change_path(eng, shape):
    cap0, cap1, c0, c1 = SHAPES[shape]
    k0s, k1s, Ms, refs = crafted(c0, c1, seed=len(shape))
    (k0, n0), (k1, n1) = padded(k0s, cap0), padded(k1s, cap1)
    out = eng.gt_matches(k0, k1, Ms, n0, n1)
    for b, ref in enumerate(refs):
        assert ref["matches"].shape[1] >= min(c0[b], c1[b]) // 3 or min(c0[b], c1[b]) == 1
        check_gt(out, b, ref, c0[b], c1[b], cap0, cap1, f"{shape} pair {b}")


def test_gt_matches_ignore_padding_poison_and_batching(fx):
    """NaN in the rows past the counts and a NaN-poisoned workspace change nothing; one call of three pairs equals three calls of one"""
    g = fx["trainpairs_ragged.npz"]
    rows0, rows1 = [g[f"kpts0_{i}"] for i in range(3)], [g[f"kpts1_{i}"] for i in range(3)]
    Ms = np.stack([g[f"M_{i}"] for i in range(3)])
    plain = new_engine()
    k0, n0 = padded(rows0, CAP, fill=0.0)
    k1, n1 = padded(rows1, CAP, fill=0.0)
    base = plain.gt_matches(k0, k1, Ms, n0, n1, want_proj=True)
    poisoned = new_engine().set_option("debug_poison", "nan")
    k0n, _ = padded(rows0, CAP)
    k1n, _ = padded(rows1, CAP)
    got = poisoned.gt_matches(k0n, k1n, Ms, n0, n1, want_proj=True)
    got2 = poisoned.gt_matches(k0n, k1n, Ms, n0, n1, want_proj=True)         # (the workspace now holds the first call's values)
    for key in ("gt0", "gt1", "all_matches", "n_matches", "n_all"):
        assert torch.equal(base[key], got[key]) and torch.equal(base[key], got2[key]), key
    for b in range(3):
        nb = int(n0[b])
        assert torch.equal(base["projected"][b, :nb].view(torch.int32), got["projected"][b, :nb].view(torch.int32))
        one = plain.gt_matches(k0n[b:b + 1], k1n[b:b + 1], Ms[b:b + 1], n0[b:b + 1].contiguous(), n1[b:b + 1].contiguous(), want_proj=True)
        for key in ("gt0", "gt1", "all_matches", "n_matches", "n_all"):
            assert torch.equal(one[key][0], base[key][b]), f"pair {b} alone: {key}"
        assert torch.equal(one["projected"][0, :nb].view(torch.int32), base["projected"][b, :nb].view(torch.int32))


# ---------------------------------------------------------------------------------------------- loss
def forward_inputs(g, H, W):
    k0, n0 = padded([g[f"kpts0_{i}"] for i in range(3)], CAP)
    k1, n1 = padded([g[f"kpts1_{i}"] for i in range(3)], CAP)
    s0, _ = padded([g[f"scores0_{i}"] for i in range(3)], CAP)
    s1, _ = padded([g[f"scores1_{i}"] for i in range(3)], CAP)
    d0, _ = padded([g[f"desc0_{i}"].T for i in range(3)], CAP)
    d1, _ = padded([g[f"desc1_{i}"].T for i in range(3)], CAP)
    return (k0, s0, d0.transpose(1, 2), (H, W), k1, s1, d1.transpose(1, 2), (H, W)), n0, n1


def columns(g):
    am = np.full((3, 2, 2 * CAP), -1, np.int64)
    for i in range(3):
        a = g[f"all_matches_{i}"]
        am[i, :, :a.shape[1]] = a
    return torch.from_numpy(am).cuda(), torch.tensor([g[f"all_matches_{i}"].shape[1] for i in range(3)], dtype=torch.int32).cuda()


@pytest.mark.parametrize("name", PIPE)
def test_loss_equals_the_reference(eng, fx, name):
    g = fx[name]
    H, W = g["image_0"].shape
    args, n0, n1 = forward_inputs(g, H, W)
    m0, _, _, _ = eng.superglue(*args, n0=n0, n1=n1)
    am, n_all = columns(g)
    gt0s = [R.gt_matches(g[f"proj_{i}"], g[f"kpts1_{i}"])["gt0"] for i in range(3)]
    gt0_dev, _ = padded(gt0s, CAP, fill=-1, dtype=np.int64)
    loss, stats = eng.match_loss(am, n_all, m0, gt0_dev)
    loss2 = eng.match_loss(am, n_all)
    assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32)), "the same call twice must give the same bits"
    loss, stats, m0 = loss.cpu().numpy(), stats.cpu().numpy(), m0.cpu().numpy()
    for i in range(3):
        ref, f64 = float(g[f"loss_t_{i}"][0]), float(g[f"loss_t_f64_{i}"][0])
        print(f"{name} sample {i}: loss {loss[i]:.6f}, reference fp32 {ref:.6f} (|diff| {abs(loss[i] - ref):.2e} of {1e-4 + 1e-4 * abs(ref):.2e} allowed), "
              f"|loss - float64| {abs(loss[i] - f64):.2e}, the reference's own |fp32 - float64| {abs(ref - f64):.2e}")
    for i in range(3):
        util.assert_close(loss[i:i + 1], g[f"loss_t_{i}"], f"{name} sample {i}: loss")
        nk = len(g[f"kpts0_{i}"])
        assert (m0[i, nk:] == -1).all()
        assert np.array_equal(stats[i], R.match_stats(m0[i, :nk], gt0s[i])), f"{name} sample {i}: stats {stats[i]}"
        assert stats[i][0] == g[f"matches_{i}"].shape[1]


def test_loss_underflow_empty_and_dustbins(fx):
    """With descriptors 32 times the unit length some entry of Z lies far below -200 (-350 on the host): a column there makes the pair's loss
    +inf, as -log(exp(Z)) does in the reference; a pair without columns has loss 0; every finite term equals the host evaluation of
    the same fp32 expression on the debug taps (tests/util.py::transport_Z)."""
    g = fx["trainpairs_ragged.npz"]
    H, W = g["image_0"].shape
    e = new_engine("default")
    e.set_debug(True)
    args, n0, n1 = forward_inputs(g, H, W)
    args = tuple(a * 32.0 if i in (2, 6) else a for i, a in enumerate(args))
    e.superglue(*args, n0=n0, n1=n1)
    S, u, v = e.fetch("scores_in"), e.fetch("u"), e.fetch("v")
    alpha = float(util.sg_sd(D)["bin_score"])
    am = np.full((3, 2, 2 * CAP), -1, np.int64)
    n_all, want = [], []
    for b in range(3):
        a, c = int(n0[b]), int(n1[b])
        Z = util.transport_Z(S[b], u[b], v[b], a, c, alpha)
        assert Z.shape == (a + 1, c + 1)
        if b == 0:            # one column far below the underflow of exp, among ordinary ones
            x, y = np.unravel_index(np.argmin(Z[:a, :c]), (a, c))
            assert Z[x, y] < -200, f"the test needs an entry of Z below -200 (lowest: {Z[x, y]})"
            cols = np.array([[0, x, a], [0, y, 1]])
            want.append(np.inf)
        elif b == 1:          # no columns
            cols = np.zeros((2, 0), np.int64)
            want.append(0.0)
        else:                 # the largest entry of the rows that have one where exp(Z) is a normal number, and of either dustbin
            rows = np.nonzero(Z[:a, :c].max(1) > -60)[0]
            assert len(rows) >= 10
            cols = np.concatenate([np.stack([rows, Z[rows, :c].argmax(1)]), [[a, Z[:a, c].argmax(), a], [Z[a, :c].argmax(), c, c]]], 1)
            cols = cols[:, Z[cols[0], cols[1]] > -80]
            assert (cols[0] == a).any() and (cols[1] == c).any(), "no dustbin entry left among the columns"
            want.append(float(R.match_loss(Z, cols)))
        am[b, :, :cols.shape[1]] = cols
        n_all.append(cols.shape[1])
    loss = e.match_loss(torch.from_numpy(am), torch.tensor(n_all, dtype=torch.int32)).cpu().numpy()
    print(f"losses {loss}, expected {want}")
    assert np.isposinf(loss[0]) and loss[1] == 0.0
    # (the same fp32 Z bits on both sides; exp and log are within a few ulp of each other, the mean is over at most 259 terms)
    assert abs(loss[2] - want[2]) <= 1e-5 * abs(want[2]) + 1e-6


def test_loss_refuses_what_it_cannot_read(eng, fx):
    from image_matching_amd.engine import ImxError
    g = fx["trainpairs_small.npz"]
    H, W = g["image_0"].shape
    am, n_all = columns(g)
    with pytest.raises(ImxError, match="no SuperGlue forward"):
        new_engine("t").match_loss(am, n_all)                                # a fresh handle
    args, n0, n1 = forward_inputs(g, H, W)
    eng.superglue(*args, n0=n0, n1=n1)
    eng.match_loss(am, n_all)
    one = tuple(a[:1] if torch.is_tensor(a) else a for a in args)
    eng.superglue(*one, n0=n0[:1].contiguous(), n1=n1[:1].contiguous())      # a forward of another shape
    with pytest.raises(ImxError, match="do not belong"):
        eng.match_loss(am, n_all)
    with pytest.raises(ImxError, match="do not belong"):
        eng.match_loss(am[:1, :, :CAP].contiguous(), n_all[:1])              # the right B, the wrong width
    assert np.isfinite(eng.match_loss(am[:1].contiguous(), n_all[:1]).cpu().numpy()).all()
    big = tuple(torch.cat([a, a], 0) if torch.is_tensor(a) else a for a in args)
    eng.knn_ratio_match(args[2], args[6], n0=n0, n1=n1)                       # a call on other buffers: the record stays
    eng.match_loss(am[:1].contiguous(), n_all[:1])
    eng.set_option("debug_poison", "zero")                                    # overwrites the workspaces
    try:
        with pytest.raises(ImxError, match="no SuperGlue forward"):
            eng.match_loss(am[:1].contiguous(), n_all[:1])
    finally:
        eng.set_option("debug_poison", "off")
    eng.superglue(*big, n0=torch.cat([n0, n0]), n1=torch.cat([n1, n1]))      # grows (frees) the score matrix: a loss of the OLD shape must not pass
    with pytest.raises(ImxError, match="do not belong"):
        eng.match_loss(am[:1].contiguous(), n_all[:1])


# ---------------------------------------------------------------------------------------------- end to end
def test_train_pairs_equals_the_stages_and_the_restatement(eng, fx):
    g = fx["trainpairs_small.npz"]
    imgs = torch.from_numpy(np.stack([g[f"image_{i}"] for i in range(3)]))
    Ms = np.stack([g[f"M_{i}"] for i in range(3)])
    out = eng.train_pairs(imgs, Ms)
    # stage by stage
    warped = eng.warp_perspective_u8(imgs, Ms)
    x = torch.cat([eng.ingest(imgs), eng.ingest(warped)], 0)
    kpts, scores, desc, counts = eng.superpoint_batch(x)
    gt = eng.gt_matches(kpts[:3], kpts[3:], Ms, counts[:3].contiguous(), counts[3:].contiguous())
    stage = {"warped": warped, "keypoints0": kpts[:3], "keypoints1": kpts[3:], "scores0": scores[:3], "scores1": scores[3:],
             "descriptors0": desc[:3], "descriptors1": desc[3:], "counts0": counts[:3], "counts1": counts[3:], **gt}
    assert set(stage) == set(out)
    for k, v in stage.items():
        a, b = out[k], v
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), k
    # its ground truth is the restatement's on the library's own keypoints
    for b in range(3):
        n0, n1 = int(out["counts0"][b]), int(out["counts1"][b])
        assert n0 > 0 and n1 > 0
        k0, k1 = out["keypoints0"][b, :n0].cpu().numpy(), out["keypoints1"][b, :n1].cpu().numpy()
        ref = R.gt_matches(R.project(k0, Ms[b]), k1)
        check_gt(out, b, ref, n0, n1, CAP, CAP, f"pair {b}")
        print(f"pair {b}: {n0} / {n1} keypoints, {ref['matches'].shape[1]} ground-truth matches (the reference on its own keypoints: {g[f'matches_{b}'].shape[1]})")
        assert ref["matches"].shape[1] >= 10


def test_dataset_and_training_module_dropins(fx, tmp_path):
    from image_matching_amd import hostops
    from image_matching_amd.datasets.GlueSparse import GlueSparse
    from image_matching_amd.superglue.models.superglue_train import SuperGlue
    g = fx["trainpairs_small.npz"]
    hostops.imwrite(str(tmp_path / "im0.png"), g["image_0"])          # (one file: which file is index 0 is the directory's order, as in the reference)
    ds = GlueSparse(str(tmp_path), util.sp_config(D, CAP), (160, 120), "cuda")
    ds.superpoint.load_state_dict(util.sp_sd(D))
    assert len(ds) == 1
    s = ds[0]
    assert sorted(s) == [str(k) for k in g["keys"]]

    def kind(v):
        if isinstance(v, list):
            return "list/" + type(v[0]).__name__ + "/" + str(getattr(v[0], "dtype", ""))
        return type(v).__name__ + "//" + str(getattr(v, "dtype", "")).replace("torch.", "")
    assert [kind(s[k]) for k in sorted(s)] == [str(t) for t in g["types"]]
    n0, n1 = len(s["keypoints0"][0]), len(s["keypoints1"][0])
    assert len(s["descriptors0"]) == D and s["descriptors0"][0].shape == (n0,) and len(s["scores1"]) == n1
    assert s["image0"].shape == (1, 120, 160) and s["image0"].dtype == torch.float64 and s["image0"].is_cuda
    am = np.stack(s["all_matches"])
    assert am.shape == (2, n0 + n1 - s["matches"].shape[1]) and np.array_equal(am[:, :s["matches"].shape[1]], s["matches"])
    again = ds[0]
    assert np.array_equal(np.stack(again["all_matches"]), am), "the sampler's stream is seeded per index"
    bt = ds.batch([0, 0])
    assert bt["all_matches"].shape == (2, 2, 2 * CAP) and bt["all_matches"].is_cuda and np.array_equal(bt["all_matches"][0, :, :am.shape[1]].cpu().numpy(), am)
    # the training module on the sample, as the reference's loop hands it over (batch-1 DataLoader, superpoint_glue_train.py:106-112)
    pred = torch.utils.data.default_collate([s])
    for k in pred:
        if k not in ("file_name", "image0", "image1"):
            pred[k] = pred[k].cuda().float() if isinstance(pred[k], torch.Tensor) else torch.stack(pred[k]).cuda()
    sg = SuperGlue(util.sg_config(D), _shared=ds.superpoint._shared).to("cuda")
    sg.load_state_dict(util.sg_sd(D, variant="t"))
    out = sg(pred)
    assert set(out) == {"matches0", "matches1", "matching_scores0", "matching_scores1", "loss", "skip_train"} and out["skip_train"] is False
    assert out["matches0"].shape == (n0,) and out["matches0"].dtype == torch.int64 and out["matching_scores1"].shape == (n1,)
    # (the loss of a sample may be +inf, in the reference too -- an exp(Z) that underflows; this sample's is finite)
    assert out["loss"].shape == (1,) and out["loss"].dtype == torch.float32 and float(out["loss"][0]) > 0
    # ... and the same value from the engine's batched path on the same pair
    eng = ds.superpoint._shared.get_engine([0, 1])
    m0, _, _, _ = eng.superglue(bt["keypoints0"][:1], bt["scores0"][:1], bt["descriptors0"][:1].transpose(1, 2), (120, 160),
                                bt["keypoints1"][:1], bt["scores1"][:1], bt["descriptors1"][:1].transpose(1, 2), (120, 160),
                                n0=bt["counts0"][:1].contiguous(), n1=bt["counts1"][:1].contiguous())
    loss = eng.match_loss(bt["all_matches"][:1].contiguous(), bt["n_all"][:1].contiguous())
    print(f"loss of the sample: {float(out['loss'][0]):.6f} alone, {float(loss[0]):.6f} padded to the cap")
    if np.isfinite(float(out["loss"][0])):
        util.assert_close(loss.cpu().numpy(), out["loss"].cpu().numpy(), "loss: padded to the cap vs the sample alone")
    else:
        assert np.isposinf(float(out["loss"][0])) and np.isposinf(float(loss[0]))


def test_cli_writes_one_file_per_synthetic_image(tmp_path, capsys):
    import superglue_export_pairs
    superglue_export_pairs.main(["--synthetic", "2", "--out_dir", str(tmp_path), "--batch", "2", "--seed", "4"])
    files = sorted(p.name for p in tmp_path.iterdir())
    assert files == ["synthetic_0000.npz", "synthetic_0001.npz"]
    z = np.load(tmp_path / files[0])
    assert {"image0", "image1", "M", "keypoints0", "keypoints1", "scores0", "scores1", "descriptors0", "descriptors1", "matches", "all_matches"} == set(z.files)
    n0, n1, n = len(z["keypoints0"]), len(z["keypoints1"]), z["matches"].shape[1]
    assert z["descriptors0"].shape == (D, n0) and z["all_matches"].shape == (2, n0 + n1 - n) and z["image1"].dtype == np.uint8
    ref = R.gt_matches(R.project(z["keypoints0"], z["M"]), z["keypoints1"])
    assert np.array_equal(ref["all_matches"], z["all_matches"])
    text = capsys.readouterr().out
    assert "wrote 2 samples" in text and "precision" in text and "recall" in text
