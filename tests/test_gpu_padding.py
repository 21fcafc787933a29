"""Padding independence at the ABI boundary: with device-side counts, rows past a pair's count belong to the caller and may hold
anything.  Every case runs the same call three times on one engine -- the padding rows of keypoints, scores and descriptors filled
with zeros, with NaN, and with +Inf (descriptors) / 3e38 (keypoints, scores) -- and the results over the valid rows must be the same
BITS: matches, matching scores, the taps kenc / gnn17 / scores_in / u / v, and the (side, pair) q / k / v maxima that scale the fp16
planes (the direct check that a padding row stays out of them).  The zero-padded run is held to the oracle on the cut tensors at the
project's 1e-4 + 1e-4|ref|, which anchors the bit identity to the reference.  Each case asserts the kernel forms it ran
(imx_timing_form), so a case cannot silently test another kernel.  Also imx_knn_ratio_match and imx_estimate_affine_partial with
poisoned rows past their counts.  Needs an MI355X.
Wall time on an MI355X: this file 14 s and tests/test_gpu_history.py 22 s, each run alone; the whole GPU suite with both 540 s of its
1200 s limit, so about 505 s for the parent commit's tests on the same box (530 s in the last recorded run of the parent)."""
import numpy as np
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu
KEYS = ("keypoints0", "keypoints1", "scores0", "scores1", "descriptors0", "descriptors1")
H, W = 240, 320
PATTERNS = ("zero", "nan", "inf")
TAPS = ("kenc", "x", "scores_in", "u", "v")

# three pairs: counts that differ per pair and are no multiple of 32; a single keypoint; an empty side inside the batch
def _three(N0, N1):
    return [N0 - 19, 1, 64], [N1, 33, 0]


# 17 pairs (the smallest batch whose 256-keypoint pairs leave the key-split attention and the 4096-row latency forms under "auto")
N0_17 = [256, 255, 128, 1, 77, 0, 129, 200, 31, 256, 97, 160, 224, 3, 250, 64, 193]
N1_17 = [256, 129, 97, 200, 0, 50, 256, 1, 255, 33, 128, 161, 7, 256, 100, 192, 65]

# id -> (descriptor_dim, N0, N1, counts0, counts1, options, forms that must have run (None: must NOT appear))
CASES = {
    "keysplit_d128_b1": (128, 256, 200, [129], [97], {},
                         {"attention": "attention_split:f32", "qkv_proj": "gemm_small:f32", "gnn_layer": "gnn_layer_small:f32", "gnn_tail": None}),
    # n0 = 128 of N0 = 160: the padding is one whole 32-row tile
    "latency_d128_b3": (128, 160, 96, [128, 1, 64], [96, 33, 0], {},
                        {"attention": "attention_h2:f16x2", "qkv_proj": "gemm_small:f32", "gnn_layer": "gnn_layer_small:f32", "qkv_amax": "", "gnn_tail": None}),
    "latency_d128_b2": (128, 200, 150, [137, 200], [150, 45], {},
                        {"attention": "attention_h2:f16x2", "qkv_proj": "gemm_small:f32", "gnn_layer": "gnn_layer_small:f32"}),
    "latency_d64_b2": (64, 100, 70, [77, 33], [70, 5], {},
                       {"attention": "attention:f32", "qkv_proj": "gemm_small:f32", "gnn_layer": "gnn_layer_small:f32"}),
    "throughput_d64_off": (64, 100, 70, *_three(100, 70), {"latency_forms": "off"},
                           {"attention": "attention:f32", "gnn_layer": None, "gnn_tail": None, "gnn_mlp1": ""}),
    "keysplit_d256_b1": (256, 256, 160, [255], [130], {},
                         {"attention": "attention_split:f32", "qkv_proj": "gemm_small:f32", "gnn_layer": "gnn_layer_small:f32"}),
    "linear_h2_d256_off": (256, 256, 256, [250, 129], [128, 1], {"latency_forms": "off"},
                           {"attention": "attention_h2:f16x2", "qkv_proj": "gemm_h2:f16x2", "gnn_mlp1": "gemm_h2:f16x2", "gnn_mlp2": "gemm_h2:f16x2",
                            "final_proj": "gemm_h2:f16x2", "rows_amax": "", "gnn_tail": None}),
    "attention_bf16x3_d256_off": (256, 256, 128, *_three(256, 128), {"latency_forms": "off", "attention": "bf16x3"},
                                  {"attention": "attention_x3:bf16x3", "qkv_proj": "gemm_x3:bf16x3", "gnn_mlp1": "gemm_x3:bf16x3"}),
    "throughput_d128_b17_auto": (128, 256, 256, N0_17, N1_17, {},
                                 {"attention": "attention_h2:f16x2", "qkv_proj": "gemm_h2:f16x2", "gnn_tail": "gnn_tail_h2:f16x2", "rows_amax": "",
                                  "gnn_layer": None, "gnn_mlp1": None, "qkv_amax": None}),
    "two_query_blocks_fused_tail_off": (128, 256, 256, *_three(256, 256), {"latency_forms": "off", "attention_qblocks": "2", "gnn_tail": "fused", "attention": "f16x2"},
                                        {"attention": "attention_h2:f16x2", "qkv_proj": "gemm_h2:f16x2", "gnn_tail": "gnn_tail_h2:f16x2"}),
    "attention_bf16x3_off": (128, 256, 128, *_three(256, 128), {"latency_forms": "off", "attention": "bf16x3"},
                             {"attention": "attention_x3:bf16x3", "qkv_proj": "gemm_x3:bf16x3", "gnn_tail": "gnn_tail_x3:bf16x3"}),
    "mfma_f32_off": (128, 200, 150, *_three(200, 150), {"latency_forms": "off", "mfma": "f32"},
                     {"attention": "attention:f32", "qkv_proj": "gemm_tiled:f32", "gnn_mlp1": "gemm_tiled:f32", "gnn_tail": None}),
    "unfused_tail_linear_bf16x3_off": (128, 256, 128, *_three(256, 128), {"latency_forms": "off", "gnn_tail": "unfused", "linear": "bf16x3"},
                                       {"attention": "attention_h2:f16x2", "qkv_proj": "gemm_x3:bf16x3", "gnn_mlp1": "gemm_x3:bf16x3", "gnn_tail": None}),
    "unfused_tail_linear_auto_off": (128, 256, 128, *_three(256, 128), {"latency_forms": "off", "gnn_tail": "unfused"},
                                     {"attention": "attention_h2:f16x2", "qkv_proj": "gemm_h2:f16x2", "gnn_mlp1": "gemm_h2:f16x2", "gnn_tail": None}),
    "tail_bf16x3_ragged_tiles_off": (128, 200, 150, *_three(200, 150), {"latency_forms": "off", "gnn_tail": "bf16x3"},
                                     {"attention": "attention_h2:f16x2", "qkv_proj": "gemm_x3:bf16x3", "gnn_tail": "gnn_tail_x3:bf16x3", "qkv_amax": ""}),
    "sinkhorn_group_1_off": (128, 200, 150, *_three(200, 150), {"latency_forms": "off", "sinkhorn_group": "1"}, {"gnn_tail": "gnn_tail_h2:f16x2"}),
    "sinkhorn_group_2_fused_merge_off": (128, 200, 150, *_three(200, 150), {"latency_forms": "off", "sinkhorn_group": "2", "sinkhorn_merge": "fused"},
                                         {"gnn_tail": "gnn_tail_h2:f16x2"}),
    "sinkhorn_group_4_off": (128, 200, 150, *_three(200, 150), {"latency_forms": "off", "sinkhorn_group": "4"}, {"gnn_tail": "gnn_tail_h2:f16x2"}),
}


def sg_weights(d):
    """The weight set per width whose forms the suite already pins: the default set at 64 / 128, the "t" set at 256 (the linear layers
    on fp16 planes: tests/test_gpu_batch_invariance.py)."""
    return util.sg_sd(d, variant="t" if d == 256 else "default")


_SP = {}


def make_inputs(d, B, N0, N1, seed):
    """B pairs of SuperGlue inputs: the ORACLE's SuperPoint on synthetic image pairs (the second image a shifted, noisy copy: real
    correspondences, decisive matches), the N0 / N1 strongest keypoints per side.  On these the oracle's own fp32 evaluation sits
    within 0.2 of the project's tolerance of its float64 evaluation (matching scores; measured on the CPU), so the tolerance can
    see the kernels.  Random unit descriptors are NOT used: there the oracle's fp32 result is itself 2.5 - 5 tolerances from
    float64 and a single-keypoint side ties 129 rows within 1e-8."""
    from oracle import superpoint_ref
    per = []
    for b in range(B):
        key = (d, seed % 7 * 100 + b)
        if key not in _SP:
            sd = util.sp_sd(d)
            _SP[key] = [superpoint_ref.superpoint_forward(x, sd, util.sp_config(d, 256)) for x in util.pair(300 + key[1], H, W)]
        per.append(_SP[key])
    out = {}
    for side, N in ((0, N0), (1, N1)):
        assert all(len(p[side]["keypoints"][0]) >= N for p in per), "the images must yield N keypoints"
        out[f"keypoints{side}"] = torch.stack([p[side]["keypoints"][0][:N] for p in per]).float()
        out[f"scores{side}"] = torch.stack([p[side]["scores"][0][:N] for p in per]).float()
        out[f"descriptors{side}"] = torch.stack([p[side]["descriptors"][0][:, :N] for p in per]).float()
    return out


def poison_padding(t, n0, n1, pattern):
    """A copy of the inputs whose rows past the counts hold the pattern; the valid rows are untouched."""
    kp, de = {"zero": (0.0, 0.0), "nan": (float("nan"), float("nan")), "inf": (3e38, float("inf"))}[pattern]
    out = {k: v.clone() for k, v in t.items()}
    for side, n in (("0", n0), ("1", n1)):
        for b, nb in enumerate(n):
            out["keypoints" + side][b, nb:] = kp
            out["scores" + side][b, nb:] = kp
            out["descriptors" + side][b, :, nb:] = de
    return out


def run_with_counts(eng, t, n0, n1, want_amax):
    """One imx_superglue_forward with device-side counts; the outputs and the taps' VALID regions per pair (bit patterns of amax)."""
    c0 = torch.tensor(n0, dtype=torch.int32, device="cuda")
    c1 = torch.tensor(n1, dtype=torch.int32, device="cuda")
    tc = {k: v.cuda() for k, v in t.items()}
    out = eng.superglue(tc["keypoints0"], tc["scores0"], tc["descriptors0"], (1, 1, H, W),
                        tc["keypoints1"], tc["scores1"], tc["descriptors1"], (1, 1, H, W), c0, c1)
    torch.cuda.synchronize()
    m0, m1, ms0, ms1 = (o.cpu() for o in out)
    taps = {k: eng.fetch(k) for k in TAPS}
    B, N0p, N1p = taps["scores_in"].shape
    res = {"tail": (m0, m1, ms0, ms1)}
    for b in range(B):
        a, c = n0[b], n1[b]
        r = {"matches0": m0[b, :a], "matches1": m1[b, :c], "matching_scores0": ms0[b, :a], "matching_scores1": ms1[b, :c]}
        for k in ("kenc", "x"):
            r[k + "/side0"] = torch.from_numpy(taps[k][b * N0p:b * N0p + a].copy())
            r[k + "/side1"] = torch.from_numpy(taps[k][B * N0p + b * N1p:B * N0p + b * N1p + c].copy())
        r["scores_in"] = torch.from_numpy(taps["scores_in"][b, :a, :c].copy())
        if a > 0 and c > 0:                  # (u[a], v[c]: the dustbin entries; a pair with an empty side has no transport problem)
            r["u"] = torch.from_numpy(taps["u"][b, :a + 1].copy())
            r["v"] = torch.from_numpy(taps["v"][b, :c + 1].copy())
        res[b] = r
    if want_amax:
        res["amax"] = torch.from_numpy(eng.fetch("amax").view(np.int32).copy())
    return res


def check_forms(forms, want, tag):
    for name, form in want.items():
        if form is None:
            assert name not in forms, f"{tag}: {name} ran ({forms[name]}), the case is about the form without it"
        elif form == "":
            assert name in forms, f"{tag}: no {name} launch: {forms}"
        else:
            assert forms.get(name) == form, f"{tag}: {name} ran as {forms.get(name)!r}, the case is about {form!r}: {forms}"


def superglue_padding_case(eng, d, N0, N1, n0, n1, opts, want_forms, tag, sd):
    """The three padding patterns on `eng` (weights loaded, options set); returns the zero-padded run's result."""
    from oracle import superglue_ref
    B = len(n0)
    t = make_inputs(d, B, N0, N1, seed=1000 + d + N0 + 7 * B)
    want_amax = opts.get("mfma") != "f32" and opts.get("attention") != "bf16x3"
    res = {}
    for pattern in PATTERNS:           # the NaN run second: the first pattern that can show a read of a padding row
        eng.timing_reset()
        eng.set_timing(True)
        res[pattern] = run_with_counts(eng, poison_padding(t, n0, n1, pattern), n0, n1, want_amax)
        forms = {}
        for r in eng.timing_report(forms=True):                 # (a name whose launches took two forms: "a+b")
            forms[r[0]] = "+".join(sorted(set(filter(None, forms.get(r[0], "").split("+"))) | {r[3]}))
        eng.set_timing(False)
        check_forms(forms, want_forms, f"{tag} ({pattern} padding)")
    print(f"\n[padding] {tag}: forms " + ", ".join(f"{k}={v}" for k, v in sorted(forms.items()) if k in ("attention", "qkv_proj", "gnn_tail", "gnn_layer", "gnn_mlp1", "final_proj", "qkv_amax", "rows_amax")))
    base = res["zero"]
    for b in range(B):
        for k, v in base[b].items():
            if v.dtype.is_floating_point:
                assert torch.isfinite(v).all(), f"{tag}: pair {b}: {k} has non-finite values over its valid region with zero padding"
    m0, m1, ms0, ms1 = base["tail"]
    for b in range(B):
        empty = n0[b] == 0 or n1[b] == 0
        a, c = (0, 0) if empty else (n0[b], n1[b])
        assert (m0[b, a:] == -1).all() and (m1[b, c:] == -1).all(), f"{tag}: pair {b}: matches past the counts {n0[b]}, {n1[b]} are not -1"
        assert (ms0[b, a:] == 0).all() and (ms1[b, c:] == 0).all(), f"{tag}: pair {b}: matching scores past the counts are not 0"
    for pattern in PATTERNS[1:]:
        for i, (x, y) in enumerate(zip(res[pattern]["tail"], base["tail"])):
            assert torch.equal(x, y), f"{tag}: output {i} (whole tensor) differs between {pattern} and zero padding"
        for b in range(B):
            for k, v in base[b].items():
                got = res[pattern][b][k]
                bad = int((got.view(torch.int32) != v.view(torch.int32)).sum()) if v.dtype == torch.float32 else int((got != v).sum())
                assert bad == 0, (f"{tag}: pair {b} (n0 = {n0[b]}, n1 = {n1[b]}): {k} differs over its valid region between {pattern} and zero padding "
                                  f"({bad} of {v.numel()} elements; non-finite: {int((~torch.isfinite(got.float())).sum())})")
        if want_amax:
            assert torch.equal(res[pattern]["amax"], base["amax"]), f"{tag}: the q / k / v maxima differ between {pattern} and zero padding: a padding row reached the fp16 scales"
    # the zero-padded run against the oracle on the cut tensors
    cfg = util.sg_config(d)
    for b in range(B):
        a, c = n0[b], n1[b]
        if a == 0 or c == 0:
            continue
        cut = {"keypoints0": t["keypoints0"][b:b + 1, :a], "keypoints1": t["keypoints1"][b:b + 1, :c], "scores0": t["scores0"][b:b + 1, :a], "scores1": t["scores1"][b:b + 1, :c],
               "descriptors0": t["descriptors0"][b:b + 1, :, :a], "descriptors1": t["descriptors1"][b:b + 1, :, :c], "image_shape0": (1, 1, H, W), "image_shape1": (1, 1, H, W)}
        ref = superglue_ref.superglue_forward(cut, sd, cfg)
        for k in ("matching_scores0", "matching_scores1"):
            print(f"[padding] {tag}: pair {b}: {k} uses {util.tolerance_used(base[b][k].numpy(), ref[k][0].numpy()):.3f} of the tolerance")
        for k in ("matches0", "matches1"):
            assert np.array_equal(base[b][k].numpy(), ref[k][0].numpy()), f"{tag}: pair {b}: {k} differ from the oracle's on the cut tensors"
        for k in ("matching_scores0", "matching_scores1"):
            util.assert_close(base[b][k], ref[k][0], f"{tag}: pair {b}: {k} vs the oracle on the cut tensors")
    return res


def make_engine(d, opts, sd=None):
    from image_matching_amd import _lib as L
    from image_matching_amd.engine import Engine
    eng = Engine(util.sp_config(d, 1024), util.sg_config(d), "cuda")
    sd = sg_weights(d) if sd is None else sd
    eng.load_state_dict(L.NET_SUPERGLUE, sd)
    for k, v in opts.items():
        eng.set_option(k, v)
        assert eng.get_option(k) == v
    eng.set_debug(True)
    return eng, sd


@pytest.mark.parametrize("case", sorted(CASES))
def test_superglue_results_do_not_depend_on_what_the_padding_rows_hold(case):
    d, N0, N1, n0, n1, opts, want_forms = CASES[case]
    assert len(n0) == len(n1) and max(n0) <= N0 and max(n1) <= N1
    eng, sd = make_engine(d, opts)
    superglue_padding_case(eng, d, N0, N1, n0, n1, opts, want_forms, case, sd)
    if opts.get("sinkhorn_merge") == "fused":
        assert eng.fetch("sk_merge_cnt").view(np.uint32)[len(n0)] == 0, "a merging Sinkhorn workgroup gave up waiting"


def test_padding_on_a_layer_whose_attention_the_guard_moves_to_bf16x3():
    """The weights-derived guard (arith_guard) runs one layer's attention on three bf16 planes inside a chain whose linear layers stay on
    the fp16 planes (the weight set of tests/test_gpu_batch_invariance.py): the bf16x3 kernel masks the SCORES of keys past the count
    and still multiplies their V rows by the zero weights, so those rows must be finite whatever the caller's padding held."""
    from tests.test_gpu_batch_invariance import GUARD_LAYER, _guarded_superglue
    d = 256
    sd = util.to_torch(_guarded_superglue(d))
    eng, _ = make_engine(d, {"latency_forms": "off"}, sd)
    guard = eng.get_option("arith_guard")
    assert guard.split("attention bf16x3 layers:")[1].split("(")[0].split() == [str(GUARD_LAYER)], guard
    superglue_padding_case(eng, d, 256, 256, [250, 129, 1], [128, 256, 33], {"latency_forms": "off"},
                           {"attention": "attention_h2:f16x2+attention_x3:bf16x3", "qkv_proj": "gemm_h2:f16x2", "gnn_mlp1": "gemm_h2:f16x2"}, "guarded_layer_d256_off", sd)


def test_knn_ratio_match_ignores_rows_past_the_counts():
    """imx_knn_ratio_match with n0 / n1: poisoned descriptor columns past the counts change nothing, and every pair equals the call on
    its cut tensors (matches, both distances), bit for bit."""
    from image_matching_amd.engine import Engine
    d, B, N0, N1 = 128, 3, 200, 150
    n0, n1 = [137, 200, 1], [150, 45, 97]
    eng = Engine(util.sp_config(d, 1024), util.sg_config(d), "cuda")
    t = make_inputs(d, B, N0, N1, seed=77)
    noise = torch.randn(B, d, N1, generator=torch.Generator().manual_seed(78))
    t["descriptors1"] = torch.nn.functional.normalize(t["descriptors0"][:, :, :N1] + 0.03 * noise, dim=1)      # side 1: noisy copies, so the ratio test passes somewhere
    c0 = torch.tensor(n0, dtype=torch.int32, device="cuda")
    c1 = torch.tensor(n1, dtype=torch.int32, device="cuda")
    res = {}
    for pattern in PATTERNS:
        p = poison_padding(t, n0, n1, pattern)
        out = eng.knn_ratio_match(p["descriptors0"].cuda(), p["descriptors1"].cuda(), 0.9, c0, c1)
        torch.cuda.synchronize()
        res[pattern] = [o.cpu() for o in out]
    for pattern in PATTERNS[1:]:
        for name, x, y in zip(("matches", "dist1", "dist2"), res[pattern], res["zero"]):
            assert torch.equal(x, y), f"knn: {name} differs between {pattern} and zero padding"
    m, d1, d2 = res["nan"]
    matched = 0
    for b in range(B):
        cm, cd1, cd2 = (o.cpu() for o in eng.knn_ratio_match(t["descriptors0"][b:b + 1, :, :n0[b]].cuda(), t["descriptors1"][b:b + 1, :, :n1[b]].cuda(), 0.9))
        assert torch.equal(m[b, :n0[b]], cm[0]) and torch.equal(d1[b, :n0[b]], cd1[0]) and torch.equal(d2[b, :n0[b]], cd2[0]), f"knn: pair {b} differs from the call on its cut tensors"
        assert (m[b, n0[b]:] == -1).all()
        # the exact search in float64 on the cut tensors: the nearest neighbour's distance at the project's tolerance
        a64, b64 = t["descriptors0"][b, :, :n0[b]].double().T, t["descriptors1"][b, :, :n1[b]].double().T
        util.assert_close(d1[b, :n0[b]], torch.cdist(a64, b64).min(1).values.float(), f"knn: pair {b}: nearest distance vs float64")
        matched += int((cm >= 0).sum())
    assert matched > 0, "the case must produce matches"


def test_estimate_affine_partial_ignores_rows_past_counts0():
    """imx_estimate_affine_partial with counts0: keypoints0 rows past the count poisoned (NaN / 3e38) and their matches0 entries set to
    a VALID index (0: if the kernel read them, a poisoned correspondence would enter the fit -- never a wild address) give the model,
    inlier mask and inlier count of the same batch with clean padding (matches -1) and no counts."""
    from image_matching_amd.engine import Engine
    B, K = 3, 160
    cnt = [160, 97, 33]
    eng = Engine(util.sp_config(128, 1024), util.sg_config(128), "cuda")
    g = torch.Generator().manual_seed(5)
    k0 = torch.rand(B, K, 2, generator=g) * torch.tensor([W - 1.0, H - 1.0])
    ang, s = 0.1, 1.05
    R = torch.tensor([[np.cos(ang) * s, -np.sin(ang) * s], [np.sin(ang) * s, np.cos(ang) * s]], dtype=torch.float32)
    k1 = k0 @ R.T + torch.tensor([12.0, -7.0]) + torch.randn(B, K, 2, generator=g)
    perm = torch.stack([torch.randperm(K, generator=g) for _ in range(B)])
    k1p = torch.empty_like(k1)
    for b in range(B):
        k1p[b, perm[b]] = k1[b]                 # keypoint i of side 0 matches keypoint perm[b][i] of side 1
    m0 = perm.clone()
    m0[:, ::5] = -1                             # some unmatched
    clean_k0, clean_m0 = k0.clone(), m0.clone()
    for b in range(B):
        clean_k0[b, cnt[b]:] = 0
        clean_m0[b, cnt[b]:] = -1
    ref = [o.cpu() for o in eng.estimate_affine_partial(clean_k0.cuda(), k1p.cuda(), clean_m0.cuda())]
    assert (ref[2] > 10).all(), ref[2]
    c0 = torch.tensor(cnt, dtype=torch.int32, device="cuda")
    for fill in (float("nan"), 3e38):
        pk0, pm0 = k0.clone(), m0.clone()
        for b in range(B):
            pk0[b, cnt[b]:] = fill
            pm0[b, cnt[b]:] = 0
        got = [o.cpu() for o in eng.estimate_affine_partial(pk0.cuda(), k1p.cuda(), pm0.cuda(), counts0=c0)]
        for name, x, y in zip(("M", "inliers", "n_inliers"), got, ref):
            assert torch.equal(x, y), f"affine: {name} with padding {fill} and counts0 differs from the clean batch"
