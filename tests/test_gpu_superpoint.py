"""SuperPoint parity: HIP path (through the C ABI / ctypes) vs golden vectors of the reference and
vs the oracle on the same seeded inputs.  Needs an MI355X."""
import numpy as np
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu


def _engine(d=128, K=1024, variant=0, align_corners=None, **kw):
    from image_matching_amd import _lib as L
    from image_matching_amd.engine import Engine
    eng = Engine(util.sp_config(d, K, **kw), util.sg_config(d), "cuda", variant, align_corners)
    return eng, L


def _nchw(a):
    return np.transpose(a, (0, 3, 1, 2))


def _check_against(eng, x, ref_kp, ref_sc, ref_desc, exact_order=True):
    kpts, scores, desc, n = eng.superpoint(x.cuda())
    for b in range(x.shape[0]):
        km, sm, dm = kpts[b, :n[b]].cpu(), scores[b, :n[b]].cpu(), desc[b, :n[b]].t().cpu()
        kr, sr, dr = ref_kp[b], ref_sc[b], ref_desc[b]
        assert n[b] == len(kr), f"image {b}: {n[b]} keypoints vs reference {len(kr)}"
        if exact_order:
            # the reference's order (torch.topk: score descending), except that keypoints whose REFERENCE scores are closer than 2e-5
            # -- the fp32 noise of the score map is ~6e-6 -- may trade places
            pos = {tuple(p): i for i, p in enumerate(np.asarray(kr).astype(int).tolist())}
            srn = np.asarray(sr, np.float64)
            for i, p in enumerate(km.numpy().astype(int).tolist()):
                assert tuple(p) in pos, f"image {b}: keypoint {p} is not in the reference's set"
                j = pos[tuple(p)]
                assert j == i or abs(srn[i] - srn[j]) < 2e-5, f"image {b}: keypoint {p} at position {i}, reference position {j} (scores {srn[i]:.7f} / {srn[j]:.7f})"
            order = [pos[tuple(p)] for p in km.numpy().astype(int).tolist()]
            util.assert_close(sm, np.asarray(sr)[order], "scores")
            util.assert_close(dm, np.asarray(dr)[:, order], "descriptors")
        else:   # near-tied scores may legally swap under top-k: compare as sets, order canonicalised
            a, r = util.canon_keypoints(km, sm, dm), util.canon_keypoints(kr, sr, dr)
            assert np.array_equal(a[0], r[0]), f"image {b}: keypoint sets differ"
            util.assert_close(a[1], r[1], "scores")
            util.assert_close(a[2], r[2], "descriptors")
    return kpts, scores, desc, n


@pytest.mark.parametrize("name", ["sp_small.npz", "sp_ragged.npz"])
def test_dense_stages_and_keypoints_vs_reference_golden(name):
    g = util.golden(name)
    H, W, seed, K = int(g["H"]), int(g["W"]), int(g["seed"]), int(g["max_keypoints"])
    eng, L = _engine(128, K)
    eng.load_state_dict(L.NET_SUPERPOINT, util.sp_sd(128))
    x = torch.cat(util.pair(seed, H, W))
    _check_against(eng, x, [g["keypoints0"], g["keypoints1"]], [g["scores0"], g["scores1"]],
                   [g["descriptors0"], g["descriptors1"]])
    util.assert_close(_nchw(eng.fetch("x4")), g["x4"], "x4")
    a3_ref = torch.nn.functional.max_pool2d(torch.from_numpy(g["x3"]), 2).numpy()     # golden x3 holds channels ::2
    util.assert_close(_nchw(eng.fetch("a3"))[:, ::2], a3_ref, "pool(x3)")
    util.assert_close(_nchw(eng.fetch("semi")), g["semi"], "semi")
    raw = _nchw(eng.fetch("desc_raw"))
    util.assert_close(raw / np.linalg.norm(raw, axis=1, keepdims=True), g["desc"], "dense descriptors")
    util.assert_close(eng.fetch("score_map"), g["score_map"], "score map", atol=1e-5)
    # NMS is compare-only: bit-exact given the reference's own pre-NMS map
    out = eng.op_nms(torch.from_numpy(g["score_map"]), 4).cpu().numpy()
    assert np.array_equal(out, g["nms"]), "simple_nms not bit-exact on the reference score map"
    # and the mask of the end-to-end map selects the same pixels
    assert np.array_equal(eng.fetch("nms") > 0, g["nms"] > 0)


@pytest.mark.parametrize("name", ["c3_pair_s59.npz", "c3_pair_s55.npz", "c5_pair_s19.npz"])
def test_c3_full_size_vs_reference_golden(name):
    g = util.golden(name)
    H, W, d, K, seed = (int(g[k]) for k in ("H", "W", "d", "K", "seed"))
    eng, L = _engine(d, K)
    eng.load_state_dict(L.NET_SUPERPOINT, util.sp_sd(d))
    x = torch.cat(util.pair(seed, H, W))
    kpts, scores, desc, n = eng.superpoint(x.cuda())
    assert n == [K, K]
    for b in range(2):
        km, sm = kpts[b].cpu().numpy(), scores[b].cpu().numpy()
        a = util.canon_keypoints(km, sm, desc[b].t().cpu().numpy())
        r = util.canon_keypoints(g[f"keypoints{b}"], g[f"scores{b}"])
        assert np.array_equal(a[0], r[0]), "keypoint set differs from the reference"
        util.assert_close(a[1], r[1], "scores")
        assert np.all(np.diff(sm) <= 0), "top-k output must be sorted by descending score"
        # descriptors: golden holds every 16th keypoint in reference order
        idx = {tuple(k): i for i, k in enumerate(km.astype(int))}
        sel = [idx[tuple(k)] for k in g[f"keypoints{b}"][::16].astype(int)]
        util.assert_close(desc[b].cpu().numpy()[sel].T, g[f"descriptors{b}_sub"], "descriptors")


def test_c3_properties_and_batch_consistency():
    d, K, H, W = 128, 1024, 480, 640
    eng, L = _engine(d, K)
    eng.load_state_dict(L.NET_SUPERPOINT, util.sp_sd(d))
    xs = [util.pair(s, H, W)[0] for s in (3, 4)]
    x = torch.cat([xs[0], xs[1], xs[0]]).cuda()
    kpts, scores, desc, n = eng.superpoint(x)
    assert n == [K, K, K]
    k, s, dsc = kpts.cpu().numpy(), scores.cpu().numpy(), desc.cpu().numpy()
    assert np.array_equal(k[0], k[2]) and np.array_equal(s[0], s[2]) and np.array_equal(dsc[0], dsc[2]), \
        "same image in two batch slots must give bit-identical results"
    single = eng.superpoint(xs[1].cuda())
    assert np.array_equal(single[0][0].cpu().numpy(), k[1]) and np.array_equal(single[2][0].cpu().numpy(), dsc[1]), \
        "batched and single-image results must be bit-identical"
    for b in range(2):
        assert (k[b][:, 0] >= 4).all() and (k[b][:, 0] < W - 4).all() and (k[b][:, 1] >= 4).all() and (k[b][:, 1] < H - 4).all()
        assert (s[b] > 0.005).all() and np.all(np.diff(s[b]) <= 0)
        np.testing.assert_allclose(np.linalg.norm(dsc[b], axis=1), 1.0, atol=1e-5)
        # NMS property: no two keypoints with distinct scores closer than the radius (Chebyshev)
        kk = k[b]
        dist = np.abs(kk[:, None, :] - kk[None, :, :]).max(-1)
        np.fill_diagonal(dist, 99)
        close = np.argwhere(dist <= 4)
        assert all(s[b][i] == s[b][j] for i, j in close), "two keypoints inside one NMS window with different scores"


def test_align_corners_true_mode_vs_oracle():
    from oracle import superpoint_ref
    eng, L = _engine(128, 207, align_corners=True)
    sd = util.sp_sd(128)
    eng.load_state_dict(L.NET_SUPERPOINT, sd)
    x = util.pair(12, 120, 160)[0]
    ref = superpoint_ref.superpoint_forward(x, sd, util.sp_config(128, 207), align_corners=True)
    ref_f = superpoint_ref.superpoint_forward(x, sd, util.sp_config(128, 207), align_corners=False)
    assert (ref["descriptors"][0] - ref_f["descriptors"][0]).abs().max() > 0.05
    _check_against(eng, x, ref["keypoints"], ref["scores"], ref["descriptors"])


def test_official_variant_vs_oracle():
    from image_matching_amd import synth
    from oracle import superpoint_ref
    d = 256
    sd = util.to_torch(synth.synth_state_dict(synth.superpoint_official_shapes(d), 77))
    eng, L = _engine(d, 300, variant=1)
    eng.load_state_dict(L.NET_SUPERPOINT, sd)
    x = util.pair(5, 128, 192)[0]
    ref = superpoint_ref.superpoint_forward(x, sd, util.sp_config(d, 300), variant="official", return_dense=True)
    kpts, scores, desc, n = eng.superpoint(x.cuda())
    util.assert_close(_nchw(eng.fetch("x4")), ref["x4"], "x4 (official)")
    util.assert_close(_nchw(eng.fetch("semi")), ref["semi"], "semi (official)")
    _check_against(eng, x, ref["keypoints"], ref["scores"], ref["descriptors"], exact_order=False)


@pytest.mark.parametrize("K", [-1, 50])
def test_constant_image_all_ties(K):
    """A constant image gives a constant score map: every pixel ties as a 9x9 maximum and the
    reference keeps them all (equality test, no tie-break)."""
    from oracle import superpoint_ref
    sd = util.sp_sd(128)
    eng, L = _engine(128, K)
    eng.load_state_dict(L.NET_SUPERPOINT, sd)
    x = torch.full((1, 1, 64, 96), 0.25)
    ref = superpoint_ref.superpoint_forward(x, sd, util.sp_config(128, K), return_dense=True)
    kpts, scores, desc, n = eng.superpoint(x.cuda())
    assert n[0] == len(ref["scores"][0])
    if K < 0:
        assert np.array_equal(kpts[0].cpu().numpy(), ref["keypoints"][0].numpy())


def test_empty_result_when_threshold_is_high():
    eng, L = _engine(128, 100, keypoint_threshold=2.0)
    eng.load_state_dict(L.NET_SUPERPOINT, util.sp_sd(128))
    kpts, scores, desc, n = eng.superpoint(util.pair(1, 64, 64)[0].cuda())
    assert n == [0] and kpts.shape == (1, 0, 2) and desc.shape == (1, 0, 128)


def test_dense_forward_for_label_export_vs_reference_golden():
    """superpoint/models/superpoint_train.py:31-57: {'semi','desc'} dense tensors in the reference layout."""
    from image_matching_amd.superpoint.models.superpoint_train import SuperPoint as DenseSuperPoint
    g = util.golden("sp_small.npz")
    H, W, seed = int(g["H"]), int(g["W"]), int(g["seed"])
    net = DenseSuperPoint(descriptor_length=128).eval().to("cuda")
    net.load_state_dict(util.sp_sd(128))
    out = net(torch.cat(util.pair(seed, H, W)).cuda())
    assert set(out) == {"semi", "desc"} and net.output is out
    assert out["semi"].shape == g["semi"].shape and out["desc"].shape == g["desc"].shape
    util.assert_close(out["semi"], g["semi"], "semi")
    util.assert_close(out["desc"], g["desc"], "desc")


@pytest.mark.parametrize("mode,form", [("direct", "conv3x3_direct"), ("wino32", "conv3x3_wino24:f32"), ("wino", "conv3x3_wino24h:f16x2")])
def test_every_conv_form_vs_reference_golden(monkeypatch, mode, form):
    """"conv" (here seeded through IMX_CONV, which imx_create reads once): "direct" puts every 3x3 layer on the direct implicit-GEMM
    kernel (the fallback for shapes the Winograd kernels reject), "wino32" on Winograd F(2x4,3x3) with fp32-MFMA products, "wino" (the
    default since round 4) runs the products of the layers after the first on the fp16 matrix pipe -- two planes per transformed
    operand, scaled by a power of two from the producing layer's per-image maximum.  Each must reproduce the reference's dense stages
    and keypoints on the ragged fixture (123x165: partial tiles on both axes) and on the 120x160 one."""
    monkeypatch.setenv("IMX_CONV", mode)
    for name in ("sp_ragged.npz", "sp_small.npz"):
        g = util.golden(name)
        H, W, seed, K = int(g["H"]), int(g["W"]), int(g["seed"]), int(g["max_keypoints"])
        eng, L = _engine(128, K)
        assert eng.get_option("conv") == mode
        eng.load_state_dict(L.NET_SUPERPOINT, util.sp_sd(128))
        x = torch.cat(util.pair(seed, H, W))
        eng.timing_reset()
        eng.set_timing(True)
        _check_against(eng, x, [g["keypoints0"], g["keypoints1"]], [g["scores0"], g["scores1"]],
                       [g["descriptors0"], g["descriptors1"]])
        forms = {r[0]: r[3] for r in eng.timing_report(forms=True)}
        eng.set_timing(False)
        assert forms["conv3b_pool"].startswith(form) and forms["convPaDa"].startswith(form), forms
        assert forms["conv1ab_pool"] == {"direct": "conv3x3_direct:f32", "wino32": "conv1ab_wino24:f32", "wino": "conv1ab_wino24h:f16x2"}[mode], forms
        util.assert_close(_nchw(eng.fetch("x4")), g["x4"], f"x4 ({mode})")
        util.assert_close(_nchw(eng.fetch("semi")), g["semi"], f"semi ({mode})")


@pytest.mark.parametrize("reps", [1, 6])
def test_fp16_plane_convolutions_on_inputs_that_stress_their_scales(reps):
    """(reps = 6, round 6 / VERDICT r5 weak 1b: the same eight images six times in one batch of 48, which selects the PAIR forms the bench
    times -- conv1ab_wino24p, conv3x3_wino24p on the first levels -- asserted; every replica must equal the first bit for bit.)
    conv = wino: the Winograd products run on two fp16 planes per operand, scaled by powers of two taken from the tile's image patch
    (first layer) and from the producing layer's per-image maximum (the others).  Inputs that stress exactly that, each held ELEMENT-WISE
    to 1e-4 + 1e-4|ref| against the oracle (round 5: no tolerance scaled by the tensor's range; the two tensors on which the fp32
    reference arithmetic itself leaves that tolerance are float64-anchored, see below): an all-black image (maxima of zero /
    bias-only activations); images of very different magnitudes in ONE batch (x 255, x 1e-3: every image carries its own scale); an
    image that is black except for one bright corner; and large dynamic range INSIDE one image, which is the case a per-image scale can
    hurt -- texture at x 1 next to a x 255 block, and a x 1e-3 image with a single saturated pixel (the dim texture sits 2^8 / 2^10
    below the image's maximum)."""
    from oracle import superpoint_ref
    from image_matching_amd import _lib as L
    from image_matching_amd.engine import Engine
    H, W, d = 72, 104, 128
    cfg = util.sp_config(d, 64)
    sd = util.sp_sd(d)
    eng = Engine(cfg, util.sg_config(d), "cuda")
    eng.load_state_dict(L.NET_SUPERPOINT, sd)
    base = [util.pair(900 + i, H, W)[i & 1] for i in range(8)]
    corner = torch.zeros(1, 1, H, W)
    corner[..., :9, :13] = base[4][..., :9, :13]
    block = base[5].clone()
    block[..., 20:44, 30:70] *= 255.0
    pixel = base[6] * 1e-3
    pixel[..., 40, 50] = 1.0
    xs = torch.cat([torch.zeros(1, 1, H, W), base[0], base[1] * 255.0, base[2] * 1e-3, corner, base[3], block, pixel])
    what = ["black", "plain", "x255", "x1e-3", "black with one bright corner", "plain", "texture next to a x255 block", "x1e-3 with one saturated pixel"]
    eng.timing_reset()
    eng.set_timing(True)
    semi, desc = eng.superpoint_dense(xs.repeat(reps, 1, 1, 1).cuda())
    forms = {r[0]: r[3] for r in eng.timing_report(forms=True)}
    eng.set_timing(False)
    if reps == 1:
        assert forms["conv1ab_pool"] == "conv1ab_wino24h:f16x2" and forms["conv4b"] == "conv3x3_wino24h:f16x2", forms
    else:
        assert forms["conv1ab_pool"] == "conv1ab_wino24p:f16x2" and forms["conv2a"] == forms["conv2b_pool"] == forms["conv3a"] == "conv3x3_wino24p:f16x2", forms
        for r in range(1, reps):
            assert torch.equal(semi[8 * r:8 * r + 8], semi[:8]) and torch.equal(desc[8 * r:8 * r + 8], desc[:8]), f"replica {r} of the stress batch differs from the first"
    ref = superpoint_ref.superpoint_forward(xs, sd, cfg, return_dense=True)
    # the same oracle in float64: where the REFERENCE arithmetic itself (fp32) leaves the element-wise tolerance of its float64
    # evaluation -- semi of the two images that hold x 255 values: its absolute error scales with the input, the 1e-4 does not -- no
    # fp32 implementation can be held element-wise, and the HIP result must instead be as close to float64 as the fp32 oracle is
    # (util.assert_fp64_anchored: rms within 2 x, maximum within 2.5 x); a property of the reference alone decides which rule applies
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    s64, d64 = superpoint_ref.heads_bn(superpoint_ref.encoder_bn(xs.double(), sd64), sd64)
    f64 = {"semi": s64, "desc": d64}
    used, anchored = [], []
    for b in range(xs.shape[0]):
        for name, mine in (("semi", semi[b].cpu().numpy()), ("desc", desc[b].cpu().numpy())):
            want, exact = ref[name][b].numpy(), f64[name][b].numpy()
            assert np.isfinite(mine).all(), f"image {b} ({what[b]}) {name}: non-finite values"
            if util.tolerance_used(want, exact) <= 1.0:
                util.assert_close(mine, want, f"image {b} ({what[b]}): {name}, element-wise")
                used.append(f"{what[b]} {name} {util.tolerance_used(mine, want):.3f}")
            else:
                util.assert_fp64_anchored(mine, want, exact, f"image {b} ({what[b]}): {name}")
                anchored.append(f"{what[b]} {name} (the fp32 oracle itself uses {util.tolerance_used(want, exact):.1f} x the tolerance against float64)")
    assert len(anchored) <= 2, anchored
    print(f"[scales] ({'pair' if reps > 1 else 'tile'} forms) fraction of the element-wise tolerance used: " + ", ".join(used) + "; float64-anchored instead: " + "; ".join(anchored))


def test_an_image_of_a_260_image_batch_equals_the_same_image_alone():
    """The per-image maxima behind the fp16 scales live in 256 slots per layer: a batch of more than 256 images runs its 3x3 layers in
    slices of 256 images with separate tables (imx_superpoint.cpp: sp_detect), so an image's scales never depend on which other images share the call --
    image b of a 260-image batch is BIT-IDENTICAL to the same image in a call of its own (different kernels run: the batch takes the
    tile-pair form, the single image the tile-per-workgroup form, which agree bit for bit)."""
    from image_matching_amd import _lib as L
    from image_matching_amd.engine import Engine
    H, W, d = 72, 104, 128
    eng = Engine(util.sp_config(d, 64), util.sg_config(d), "cuda")
    eng.load_state_dict(L.NET_SUPERPOINT, util.sp_sd(d))
    eng.set_option("latency_forms", "off")        # (the 1x1 heads of a single image would otherwise take their latency form: another summation order)
    base = [util.pair(900 + i, H, W)[i & 1] for i in range(6)]
    big = torch.cat([base[i % 6] * (1.0 + (i % 7)) for i in range(260)]).cuda()
    semi, desc = eng.superpoint_dense(big)
    semi, desc = semi.clone(), desc.clone()
    # (187..190: where the short second slice's pixel-major a2a would land inside the first slice's tile-swizzled a2a if the slices of a
    # tensor were spaced by each slice's own image size -- found and fixed in round 5)
    for b in (0, 5, 187, 188, 189, 190, 255, 256, 259):
        s1, d1 = eng.superpoint_dense(big[b:b + 1])
        assert torch.equal(s1[0], semi[b]), f"image {b} of 260: semi differs from the same image alone"
        assert torch.equal(d1[0], desc[b]), f"image {b} of 260: descriptors differ from the same image alone"


@pytest.mark.parametrize("H,W,B", [(120, 160, 24), (80, 96, 35), (123, 165, 40)])
def test_tile_pair_winograd_form_is_bit_identical_to_the_tile_per_workgroup_form(H, W, B, monkeypatch):
    """Round 5: conv3x3_wino24p.hip runs the fp16-plane Winograd layers on PAIRS of tiles, the 24 positions split over two waves whose
    accumulators meet through LDS before conv3x3_wino24h's epilogue -- chosen per layer where there is at least one item per CU
    ("conv" = "wino"), the tile-per-workgroup kernel otherwise ("conv" = "wino_h": always).  Every output of the pair form sees
    conv3x3_wino24h's arithmetic in the same order, so the two settings must agree BIT FOR BIT on semi and the descriptors -- which
    carries every parity statement made for conv3x3_wino24h over to the pair form.  Shapes: whole tiles; 80x96 with 35 images (an odd
    number of tiles at the second level: the last pair has a dead tile); ragged 123x165 (partial tiles, masked stores).
    Between two pair-form layers without a pool between them (conv2a -> conv2b, ...) the tensor is TILE-SWIZZLED (the accumulators' own
    lane order, 1 KB per store instruction; whole padded tiles, the consumer zeroes what lies outside the image): pure data movement, so
    the same bits again -- also against "conv_swizzle" = "off", which keeps the pixel-major blocked layout.
    These three shapes never run conv4a / conv4b as a pair and reach few of the FASTW variants: tests/test_gpu_superpoint_tiles.py holds
    the pair form to the tile form on every tap at shapes that do."""
    from image_matching_amd import _lib as L
    from image_matching_amd.engine import Engine
    d = 128
    eng = Engine(util.sp_config(d, 64), util.sg_config(d), "cuda")
    eng.load_state_dict(L.NET_SUPERPOINT, util.sp_sd(d))
    xs = torch.cat([util.pair(700 + i, H, W)[i & 1] * (1.0 + (i % 5)) for i in range(B)]).cuda()
    got = {}
    for mode in ("wino_h", "wino", "wino/blocked"):
        eng.set_option("conv_swizzle", "off" if mode == "wino/blocked" else "on")
        eng.set_option("conv", mode.split("/")[0])
        assert eng.get_option("conv") == mode.split("/")[0]
        eng.timing_reset()
        eng.set_timing(True)
        semi, desc = eng.superpoint_dense(xs)
        torch.cuda.synchronize()
        got[mode] = (semi.clone(), desc.clone(), {r[0]: r[3] for r in eng.timing_report(forms=True)})
        eng.set_timing(False)
    fh, fp = got["wino_h"][2], got["wino"][2]
    layers = ("conv2a", "conv2b_pool", "conv3a", "conv3b_pool", "conv4a", "conv4b", "convPaDa")
    assert all(fh[k] == "conv3x3_wino24h:f16x2" for k in layers) and fh["conv1ab_pool"] == "conv1ab_wino24h:f16x2", fh
    assert fp["conv1ab_pool"] == "conv1ab_wino24p:f16x2", fp            # (the fused first layer has a pair form too: conv1ab_wino24p.hip)
    assert fp["conv2a"] == "conv3x3_wino24p:f16x2" and fp["convPaDa"] == "conv3x3_wino24p:f16x2", fp
    assert all(fp[k] in ("conv3x3_wino24p:f16x2", "conv3x3_wino24h:f16x2") for k in layers), fp
    assert torch.equal(got["wino"][0], got["wino_h"][0]), "semi differs between the pair form and the tile-per-workgroup form"
    assert torch.equal(got["wino"][1], got["wino_h"][1]), "descriptors differ between the pair form and the tile-per-workgroup form"
    assert torch.equal(got["wino"][0], got["wino/blocked"][0]) and torch.equal(got["wino"][1], got["wino/blocked"][1]), "tile-swizzled vs blocked tensors between the pair-form layers"
    assert torch.isfinite(got["wino"][0]).all()


@pytest.mark.parametrize("radius", [1, 2, 3, 4, 5, 6, 9, 13])
def test_nms_every_radius_bit_exact_vs_oracle(radius):
    """simple_nms is compare-only, so both forms (radius <= 4: the staged three-kernel form with bit-row masks; any other radius:
    the generic separable passes -- the reference accepts any --nms_radius, superpoint_test.py:7-22) must reproduce the oracle bit
    for bit on the reference's own score map, on partial tiles too -- and on a batch of wider maps whose width is not a multiple
    of the 64-column tile or of the 32-bit mask words."""
    from oracle import superpoint_ref
    g = util.golden("sp_ragged.npz")
    eng, L = _engine(128, -1)
    sm = torch.from_numpy(g["score_map"])
    out = eng.op_nms(sm, radius).cpu().numpy()
    ref = superpoint_ref.simple_nms(sm, radius).numpy()
    assert np.array_equal(out, ref), f"radius {radius}: {(out != ref).sum()} pixels differ"
    rng = np.random.RandomState(radius)
    big = np.round(rng.rand(3, 77, 203).astype(np.float32) * 8) / 8          # many exact ties
    big[rng.rand(*big.shape) < 0.5] = 0.0
    t = torch.from_numpy(big)
    out = eng.op_nms(t, radius).cpu().numpy()
    ref = superpoint_ref.simple_nms(t, radius).numpy()
    assert np.array_equal(out, ref), f"radius {radius} (3 x 77 x 203, ties): {(out != ref).sum()} pixels differ"


def test_max_keypoints_beyond_the_lds_sort_vs_oracle():
    """The reference takes any max_keypoints (superpoint_test.py:33-37, :146-149).  Above 16384 the top-k sort of kp_topk no longer
    fits LDS and runs out of HBM: with nms_radius 1 and a low threshold a 480x640 image has > 25000 candidates, of which the
    best 20000 are kept -- same set and scores as the oracle's torch.topk (order canonicalised: near-tied scores may swap)."""
    from oracle import superpoint_ref
    d, K, H, W = 128, 20000, 480, 640
    cfg = util.sp_config(d, K, nms_radius=1, keypoint_threshold=0.0005)
    from image_matching_amd import _lib as L
    from image_matching_amd.engine import Engine
    eng = Engine(cfg, util.sg_config(d), "cuda")
    sd = util.sp_sd(d)
    eng.load_state_dict(L.NET_SUPERPOINT, sd)
    x = util.pair(59, H, W)[0]
    ref = superpoint_ref.superpoint_forward(x, sd, cfg)
    assert len(ref["keypoints"][0]) == K, "the case must exercise the top-k (more candidates than max_keypoints)"
    _check_against(eng, x, [ref["keypoints"][0]], [ref["scores"][0]], [ref["descriptors"][0]], exact_order=False)


def test_descriptor_dim_not_a_multiple_of_32_superpoint_alone_vs_oracle():
    """The reference's SuperPoint takes any descriptor_dim (superpoint_test.py:57-63, :83); only SuperGlue needs 4 heads.  A 100-wide
    descriptor head (convDb N = 100: a partial 64-column tile, 400-byte rows) against the oracle: same keypoints, descriptors at
    1e-4; and SuperGlue weights for that width are refused with a message, not mis-computed."""
    from oracle import superpoint_ref
    from image_matching_amd import _lib as L
    from image_matching_amd.engine import Engine, ImxError
    d, K, H, W = 100, 300, 120, 160
    cfg = util.sp_config(d, K)
    eng = Engine(cfg, {"descriptor_dim": d, "keypoint_encoder": [32, 64], "weights": None, "sinkhorn_iterations": 10, "match_threshold": 0.2}, "cuda")
    sd = util.sp_sd(d)
    eng.load_state_dict(L.NET_SUPERPOINT, sd)
    x = torch.cat(util.pair(21, H, W))
    ref = superpoint_ref.superpoint_forward(x, sd, cfg)
    _check_against(eng, x, ref["keypoints"], ref["scores"], ref["descriptors"])
    from image_matching_amd import synth
    with pytest.raises(ImxError):
        eng.load_state_dict(L.NET_SUPERGLUE, util.to_torch(synth.synth_state_dict(synth.superglue_shapes(d, [32, 64]), 5)))


@pytest.mark.parametrize("seed", util.fuzz_seeds([0, 1, 2, 3, 4, 5, 6, 7]))
def test_superpoint_random_shapes_and_configs_vs_oracle(seed):
    """Random image sizes (not multiples of 8: the pools floor, superpoint_test.py:113-116), batch sizes,
    nms_radius, remove_borders, keypoint_threshold and max_keypoints.  The dense stages against the oracle on the same input at
    1e-4 (score map 1e-5); then the compare-only tail -- simple_nms, threshold, border removal, top-k, descriptor sampling -- must
    equal the oracle's tail run on the LIBRARY's own score map and dense descriptors exactly (keypoint sets and scores; sampled
    descriptors at 1e-4), so a near-tie in the map cannot excuse a difference."""
    from oracle import superpoint_ref
    from image_matching_amd import _lib as L
    from image_matching_amd.engine import Engine
    rng = np.random.RandomState(4321 + seed)
    d = 128
    B = int(rng.randint(1, 4))
    H, W = int(rng.randint(24, 331)), int(rng.randint(24, 421))
    if seed % 4 == 0:
        H, W = int(rng.randint(8, 41)), int(rng.randint(8, 41))           # down to one 8x8 cell
    radius = int(rng.choice([0, 1, 2, 3, 4, 4, 4, 5, 7]))
    border = int(rng.choice([0, 2, 4, 4, 8, 16]))
    thr = float(rng.choice([0.0005, 0.002, 0.005, 0.005, 0.015]))
    K = int(rng.choice([-1, 1, 30, 200, 1024, 5000]))
    official = seed % 5 == 3              # the no-BN network of superglue/models/superpoint.py (d = 256)
    ac = seed % 7 == 5                    # the torch < 1.10 branch of sample_descriptors (superpoint_test.py:47)
    if official:
        from image_matching_amd import synth
        d = 256
        sd = util.to_torch(synth.synth_state_dict(synth.superpoint_official_shapes(d), 77))
    else:
        sd = util.sp_sd(d)
    cfg = util.sp_config(d, K, nms_radius=radius, remove_borders=border, keypoint_threshold=thr)
    eng = Engine(cfg, util.sg_config(d), "cuda", 1 if official else 0, True if ac else None)
    eng.load_state_dict(L.NET_SUPERPOINT, sd)
    eng.set_debug(True)
    x = torch.cat([util.pair(300 + 7 * seed + b, H, W)[b & 1] for b in range(B)])
    what = f"seed {seed}: B={B} {H}x{W} r={radius} border={border} thr={thr} K={K}{' official' if official else ''}{' align_corners' if ac else ''}"
    kpts, scores, desc, n = eng.superpoint(x.cuda())
    ref = superpoint_ref.superpoint_forward(x, sd, cfg, variant="official" if official else "bn", align_corners=ac, return_dense=True)
    H8, W8 = (H // 8) * 8, (W // 8) * 8
    util.assert_close(_nchw(eng.fetch("semi")), ref["semi"].numpy(), what + " semi")
    raw = _nchw(eng.fetch("desc_raw"))
    dense = raw / np.linalg.norm(raw, axis=1, keepdims=True)
    util.assert_close(dense, ref["desc"].numpy(), what + " dense descriptors")
    # the dense export of the training / label-export forward (superpoint_train.py:31-57): the reference's channel-major layout
    semi_d, desc_d = eng.superpoint_dense(x.cuda())
    util.assert_close(semi_d.cpu().numpy(), ref["semi"].numpy(), what + " dense-export semi")
    util.assert_close(desc_d.cpu().numpy(), ref["desc"].numpy(), what + " dense-export descriptors")
    kpts, scores, desc, n = eng.superpoint(x.cuda())          # (the dense call overwrote the detection state: run it again)
    own_map = eng.fetch("score_map")
    assert own_map.shape == (B, H8, W8), what
    util.assert_close(own_map, ref["score_map"].numpy(), what + " score map", atol=1e-5)
    # the tail, on the library's own map
    own_nms = superpoint_ref.simple_nms(torch.from_numpy(own_map), radius)
    assert np.array_equal(eng.fetch("nms"), own_nms.numpy()), what + ": NMS differs from simple_nms on the library's own score map"
    for b in range(B):
        k_ref, s_ref = superpoint_ref.extract_keypoints(own_nms[b], thr, border, K)
        assert n[b] == len(k_ref), f"{what} image {b}: {n[b]} keypoints, oracle tail {len(k_ref)}"
        if n[b] == 0:
            continue
        km, sm, dm = kpts[b, :n[b]].cpu().numpy(), scores[b, :n[b]].cpu().numpy(), desc[b, :n[b]].t().cpu().numpy()
        d_ref = superpoint_ref.sample_descriptors(k_ref[None], torch.from_numpy(dense[b:b + 1]), 8, ac)[0].numpy()
        a, r = util.canon_keypoints(km, sm, dm), util.canon_keypoints(k_ref.numpy(), s_ref.numpy(), d_ref)
        if not np.array_equal(a[0], r[0]):
            # legal only as a tie at the top-k boundary: every keypoint on one side only carries the boundary score
            sa, sr = {tuple(p) for p in a[0].tolist()}, {tuple(p) for p in r[0].tolist()}
            lowest = float(s_ref.min())
            odd = [p for p in sa ^ sr if float(own_nms[b][int(p[1]), int(p[0])]) != lowest]
            assert not odd, f"{what} image {b}: keypoint sets differ beyond a top-k boundary tie: {odd[:5]}"
            continue
        assert np.array_equal(a[1], r[1]), f"{what} image {b}: scores are not the map's values"
        util.assert_close(a[2], r[2], f"{what} image {b} descriptors")
        if 0 <= K < 10 ** 9 and n[b] == K:
            assert np.all(np.diff(sm) <= 0), what + ": top-k output must be sorted by descending score"


@pytest.mark.parametrize("H,W", [(226, 192), (193, 197), (294, 388), (130, 66)])
def test_odd_sizes_whose_pooled_sizes_are_whole_tiles(H, W):
    """Round-3 regression (found by the shape fuzz above).  With floor pooling an input of 113x96 pools to 56x48 and one of 48x49 to
    24x24: whole numbers of pooled tiles although the INPUT has a partial last tile row / column.  conv3x3_wino24's unmasked store
    path keyed on the pooled size, so the partial tiles' outputs landed in the next channel plane (rows) or wrapped into the next
    image row (columns).  x4 and semi against the oracle at 1e-4 on such sizes."""
    from oracle import superpoint_ref
    eng, L = _engine(128, 100)
    sd = util.sp_sd(128)
    eng.load_state_dict(L.NET_SUPERPOINT, sd)
    eng.set_debug(True)
    x = torch.cat(util.pair(77, H, W))
    eng.superpoint(x.cuda())
    ref = superpoint_ref.superpoint_forward(x, sd, util.sp_config(128, 100), return_dense=True)
    util.assert_close(_nchw(eng.fetch("x4")), ref["x4"].numpy(), f"{H}x{W} x4")
    util.assert_close(_nchw(eng.fetch("semi")), ref["semi"].numpy(), f"{H}x{W} semi")


@pytest.mark.parametrize("H,W,radius,border,thr,K", [(480, 640, 4, 4, 0.005, 1024), (123, 165, 2, 0, 0.0005, -1), (40, 2216, 4, 8, 0.002, 300),
                                                     (64, 72, 1, 16, 0.015, 30), (96, 128, 3, 4, 0.0, 5000)])
def test_keypoints_from_candidate_bit_rows_equal_the_dense_form(H, W, radius, border, thr, K):
    """Round 6: NMS + threshold + remove_borders leave the detector as candidate BIT rows and the keypoint kernels count
    and scatter from those ("keypoints" = bits, the default where the staged NMS applies) instead of three passes over the dense
    where(max_mask, scores, 0) map ("keypoints" = dense).  Compare-only work either way: keypoints, scores, descriptors and counts must
    agree bit for bit -- on a row of more than 64 mask words (W = 2216), a zero threshold, a border wider than the NMS radius and an
    image smaller than one NMS tile."""
    from image_matching_amd import _lib as L
    from image_matching_amd.engine import Engine
    d = 128
    cfg = util.sp_config(d, K, nms_radius=radius, remove_borders=border, keypoint_threshold=thr)
    eng = Engine(cfg, util.sg_config(d), "cuda")
    eng.load_state_dict(L.NET_SUPERPOINT, util.sp_sd(d))
    x = torch.cat([util.pair(900 + i, H, W)[i & 1] for i in range(3)]).cuda()
    got = {}
    for mode in ("dense", "bits", "auto"):
        eng.set_option("keypoints", mode)
        assert eng.get_option("keypoints") == mode
        eng.timing_reset()
        eng.set_timing(True)
        kpts, scores, desc, n = eng.superpoint(x)
        torch.cuda.synchronize()
        forms = {r[0]: r[3] for r in eng.timing_report(forms=True)}
        eng.set_timing(False)
        assert forms["nms"] == ("nms_staged:hbm" if mode == "dense" else "nms_staged_bits:hbm"), forms
        got[mode] = (kpts.clone(), scores.clone(), desc.clone(), list(n))
    assert sum(got["dense"][3]) > 0, "the case must produce keypoints"
    for mode in ("bits", "auto"):
        assert got[mode][3] == got["dense"][3], (mode, got[mode][3], got["dense"][3])
        for a, b, name in zip(got[mode][:3], got["dense"][:3], ("keypoints", "scores", "descriptors")):
            assert torch.equal(a, b), f"{name} differ between keypoints = {mode} and dense"
