"""SuperGlue on network shapes other than the shipped one, the part that needs no GPU: the oracle against the reference's own forward on
other layer lists and encoders (tests/golden/sg_layers.npz), the reference's own fp32 distance from its float64 self on every net the
GPU tests use (the bar of tests/test_gpu_sg_shapes.py is one a correct fp32 implementation can keep), and the refusals."""
import ctypes

import numpy as np
import pytest
import torch

from image_matching_amd import _lib
from tests import sg_shapes as G
from tests import util


@pytest.mark.parametrize("net", G.GOLDEN_NETS, ids=lambda n: n[0] + ("-" + n[1] if n[1] else ""))
def test_oracle_equals_the_reference_on_its_own_layer_lists(net):
    """oracle/superglue_ref.py on `[]`, c, ss, ssccs, c x 18 and the 8-entry encoder against the reference's SuperGlue built with that
    configuration (make_golden.py --sg-layers; "t" weights, sg_small's inputs): samples of kenc, of every layer's output, of scores_in
    and of Z at 1e-5 in fp32 and in float64, match indices equal, matching scores at 1e-5."""
    from oracle import superglue_ref
    lname, ename = net
    g, gs = util.golden("sg_layers.npz"), util.golden("sg_small.npz")
    tag = lname + ("_" + ename if ename else "")
    sd, cfg = G.state(128, lname, ename), G.config(128, lname, ename)
    data = {k: torch.from_numpy(gs[k]) for k in G.KEYS}
    sk, sc, ss = G.GOLDEN_STRIDE_K, G.GOLDEN_STRIDE_C, G.GOLDEN_STRIDE_S
    for dtype in (torch.float32, torch.float64):
        r = superglue_ref.superglue_forward({**{k: v.to(dtype) for k, v in data.items()}, "image_shape0": G.SHAPE, "image_shape1": G.SHAPE},
                                            {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}, cfg, return_dense=True)
        dn = r["dense"]
        mine = {"kenc": torch.stack([dn["kenc0"][0, ::sc, ::sk], dn["kenc1"][0, ::sc, ::sk]]), "scores_in": dn["scores_in"][0, ::ss, ::ss], "Z": dn["Z"][0, ::ss, ::ss]}
        if G.LISTS[lname]:
            mine["gnn"] = torch.stack([torch.stack([dn["gnn_taps"][l][0][0, ::sc, ::sk], dn["gnn_taps"][l][1][0, ::sc, ::sk]]) for l in range(len(G.LISTS[lname]))])
        assert (f"{tag}/gnn" in g) == bool(G.LISTS[lname])
        for k, v in mine.items():
            want = g[f"{tag}/{k}"].astype(np.float64) + (g[f"{tag}/{k}_d64"].astype(np.float64) if dtype == torch.float64 else 0.0)
            util.assert_close(v.numpy(), want, f"{tag} {k} ({dtype})", atol=1e-5, rtol=1e-5)
        if dtype == torch.float32:
            for side in "01":
                assert np.array_equal(r["matches" + side].numpy(), g[f"{tag}/matches{side}"]), f"{tag}: matches{side}"
                util.assert_close(r["matching_scores" + side].numpy(), g[f"{tag}/matching_scores{side}"], f"{tag} matching_scores{side}", atol=1e-5, rtol=1e-5)
        else:
            Zi = dn["Z"][:, :-1, :-1]
            assert np.array_equal(Zi.max(2).indices.numpy(), g[f"{tag}/idx0_f64"]) and np.array_equal(Zi.max(1).indices.numpy(), g[f"{tag}/idx1_f64"]), f"{tag}: float64 argmaxes"


@pytest.mark.parametrize("net", G.NETS, ids=G.case_id)
def test_the_bar_is_one_the_reference_keeps(net):
    """For every (d, list, encoder) of the GPU tests: the oracle's fp32 result uses at most half of 1e-4 + 1e-4 |x64| against its own
    float64 evaluation on kenc, every layer's output, scores_in and Z, on all three pairs of the frame, and its match indices equal
    the float64 ones -- with no excuse (index_excuses is what the library's result may use; the oracle's fp32 run needs none)."""
    d, lname, ename = net
    thr = G.config(d, lname, ename)["match_threshold"]
    worst = 0.0
    for b, (r32, r64) in enumerate(G.oracle(d, lname, ename)):
        fr = G.dense_fractions(r32, r64)
        print(f"[sg-shapes host] {G.case_id(net)} pair {b}: the oracle's fp32 forward uses kenc {fr['kenc']:.3f}, gnn {fr['gnn']:.3f} (layer {fr['gnn_layer']}), "
              f"scores_in {fr['scores_in']:.3f}, Z {fr['Z']:.3f} of the bar")
        worst = max(worst, *(fr[q] for q in G.QUANTITIES))
        for side in "01":
            assert np.array_equal(r32["matches" + side], r64["matches" + side]), f"{G.case_id(net)} pair {b}: fp32 and float64 match indices differ"
            util.assert_close(r32["matching_scores" + side], r64["matching_scores" + side], f"{G.case_id(net)} pair {b} matching_scores{side}")
            e, bad = G.index_excuses(r64["Z"], thr, r32["matches" + side], r64["matches" + side], r32["matching_scores" + side], r64["matching_scores" + side],
                                     int(side), G.case_id(net))
            assert e == 0 and not bad
    assert worst <= 0.5, f"{G.case_id(net)}: the oracle's own fp32 forward uses {worst:.3f} of the bar against float64"


@pytest.mark.parametrize("net", G.TV_NETS, ids=lambda n: f"d{n[0]}-{n[1]}-tv")
def test_the_bar_holds_with_a_small_v_projection(net):
    """The "tv" weight set (sg_shapes.VARIANT_GAINS) of the GPU test of the max |x'| hand-off: the oracle's fp32 forward uses at most
    half the bar against float64 on every quantity and pair, indices equal; and max |v| is indeed far below max |x| in every layer."""
    d, lname = net
    from oracle import superglue_ref as R
    sd = G.state(d, lname, None, "tv")
    for b, (r32, r64) in enumerate(G.oracle(d, lname, None, "tv")):
        fr = G.dense_fractions(r32, r64)
        print(f"[sg-shapes host] d{d}-{lname}-tv pair {b}: {fr}")
        assert max(fr[q] for q in G.QUANTITIES) <= 0.5, fr
        for side in "01":
            assert np.array_equal(r32["matches" + side], r64["matches" + side])
        n0 = G.COUNTS[b][0]
        for l, x in enumerate([r64["kenc"]] + r64["gnn"][:-1]):
            v = R._conv1(torch.from_numpy(x.T[None]), {k: t.double() for k, t in sd.items() if t.is_floating_point()}, f"gnn.layers.{l}.attn.proj.2")[0].T.numpy()
            for rows in (slice(0, n0), slice(n0, None)):
                assert np.abs(v[rows]).max() * 16 < np.abs(x[rows]).max(), (l, np.abs(v[rows]).max(), np.abs(x[rows]).max())


@pytest.mark.parametrize("net", G.LOPSIDED_NETS, ids=lambda n: f"d{n[0]}-{n[1]}-lopsided")
def test_the_bar_holds_on_the_lopsided_pair(net):
    """The lopsided pair (sg_shapes.lopsided_pair) with the "tq" weights: the two sides' v-maxima differ by more than a factor of 16
    in the first layer, and the oracle's fp32 forward keeps kenc and every layer's output inside the bar of its float64 self (measured
    0.21 to 0.55; asserted below 0.75, which leaves a correct fp32 implementation the room the reference itself needs).  scores_in and
    Z are printed only: there the reference's own fp32 forward is outside (the scores reach several thousand)."""
    d, lname = net
    from oracle import superglue_ref as R
    sd, cfg, p = G.state(d, lname, None, "tq"), G.config(d, lname), G.lopsided_pair(d)
    r32, r64 = G.oracle_run(sd, cfg, p, torch.float32), G.oracle_run(sd, cfg, p, torch.float64)
    fr = G.dense_fractions(r32, r64)
    print(f"[sg-shapes host] d{d}-{lname}-lopsided: {fr}")
    assert fr["kenc"] <= 0.75 and fr["gnn"] <= 0.75, fr
    v = R._conv1(torch.from_numpy(r64["kenc"].T[None]), {k: t.double() for k, t in sd.items() if t.is_floating_point()}, "gnn.layers.0.attn.proj.2")[0].T.numpy()
    assert np.abs(v[G.K:]).max() > 16 * np.abs(v[:G.K]).max()


def test_tables_cover_what_the_issue_names():
    S, C = G.S, G.C
    assert G.LISTS["sc18"] == [S, C] * 9 and G.LISTS["sc17"] == G.LISTS["sc18"][:17] and G.LISTS["alt19"][:18] == G.LISTS["sc18"] and G.LISTS["alt64"][:19] == G.LISTS["alt19"]
    assert len(G.LISTS["alt64"]) == _lib.IMX_MAX_GNN_LAYERS and len(G.ENCODERS["k8"]) == _lib.IMX_MAX_KENC
    d128 = {c[1:] for c in G.CASES if c[0] == 128 and c[2] is None}
    assert all((l, None, o) in d128 for l in G.ALL for o in "AB") and all((l, None, o) in d128 for l in G.FEW for o in "CDE")
    assert {c[1:] for c in G.CASES if c[0] == 256} == {(l, None, o) for l in G.FEW for o in "ABD"}
    assert {c[1:] for c in G.CASES if c[0] == 64} == {(l, None, o) for l in G.FEW for o in "AB"}
    assert {c[1:] for c in G.CASES if c[2]} == {("sc", e, o) for e in G.ENCODERS for o in "AB"}
    inp, n0, n1 = G.frame(128)
    assert inp["descriptors0"].shape == (3, 128, 256) and torch.isnan(inp["keypoints1"][2, 97:]).all() and not torch.isnan(inp["keypoints1"][2, :97]).any()
    assert n0.tolist() == [256, 200, 256] and n1.tolist() == [256, 131, 97]


def test_create_refuses_shapes_past_the_limits():
    """imx_create: 65 GNN layers, and a keypoint encoder of 0 or 9 entries, return an error with a message that names the field
    (the checks come before the device is looked for: they run without one)."""
    lib = _lib.load_library()
    for layers, kenc_n, what in ((65, 3, b"num_gnn_layers 65"), (18, 0, b"keypoint_encoder length 0"), (18, 9, b"keypoint_encoder length 9")):
        h, cfg = ctypes.c_void_p(), _lib.ImxConfig()
        cfg.descriptor_dim, cfg.kenc_n, cfg.num_gnn_layers = 128, kenc_n, layers
        assert lib.imx_create(0, ctypes.byref(cfg), ctypes.byref(h)) != 0 and not h.value
        assert what in lib.imx_last_error(None), lib.imx_last_error(None)


def test_engine_refuses_shapes_past_the_limits(monkeypatch):
    """The Engine constructor on 65 layers, and on an empty or 9-entry keypoint_encoder (which must not reach the fixed-size arrays of
    the configuration struct): ImxError.  Without a device the constructor stops at its GPU check first (test_host.py:
    test_no_gpu_fails_loudly), so that one check is answered for it here; nothing past the refusals touches a device."""
    from image_matching_amd.engine import Engine, ImxError
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    with pytest.raises(ImxError, match="at most 64 GNN layers"):
        Engine(util.sp_config(128, 256), util.sg_config(128, GNN_layers=["self"] * 65), "cuda:0")
    for kenc in ([], [32] * 9):
        with pytest.raises(ImxError, match="keypoint_encoder needs 1 to 8 entries"):
            Engine(util.sp_config(128, 256), util.sg_config(128, keypoint_encoder=kenc), "cuda:0")
