"""SuperGlue forward on network shapes other than the shipped ['self', 'cross'] * 9: GNN layer lists from none to 64 layers with
every neighbourhood of 'self' and 'cross' (first and last included), keypoint encoders of 1 and 8 entries, descriptor_dim 64 / 128 /
256, under five option sets -- against the oracle's float64 evaluation, element-wise on every layer's output.  The tables and helpers
are tests/sg_shapes.py; what is pinned and what was measured is DESIGN.md section 26.  Needs an MI355X.

Wall time on an MI355X, all 96 tests: 31 s alone (imports and collection included); 26 s of the whole suite's 663 s."""
import ctypes

import numpy as np
import pytest
import torch

from tests import sg_shapes as G
from tests import util

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def frames():
    return {d: G.frame(d) for d in (64, 128, 256)}


_SHIPPED = {}


def shipped_forms(d, ename, opts, frames):
    """The (launch name, kernel form) pairs of the shipped 18-layer list on the same frame and options: the forms that are meant."""
    key = (d, ename, opts)
    if key not in _SHIPPED:
        eng = G.engine(d, "sc18", ename, opts)
        t, n0, n1 = frames[d]
        _SHIPPED[key] = G.forward(eng, t, n0, n1, forms=True)[1]
    return _SHIPPED[key]


def check_forms(tag, seen, want, d, lname, opts):
    """The case's (name, form) pairs are the shipped run's.  With no GNN layer final_proj is a launch of its own -- which the shipped
    run, whose last fused tail computes it, may not have: its form must then be the one the shipped run's plain q|k|v projection took
    (the same linear() of plan_superglue chooses both)."""
    extra = seen - want
    if not G.LISTS[lname]:
        qkv = {f for n, f in want if n == "qkv_proj"}
        extra = {(n, f) for n, f in extra if not (n == "final_proj" and not any(w == "final_proj" for w, _ in want) and f in qkv)}
    assert not extra, f"{tag}: launches in forms the shipped list does not take at this shape and options: {sorted(extra)} (shipped: {sorted(want)})"
    if d == 128 and G.LISTS[lname] and opts in "AB":
        name = "gnn_layer" if opts == "A" else "gnn_tail"
        tail = {(n, f) for n, f in want if n == name}
        assert tail and tail <= seen, f"{tag}: the shipped run's {name} form {sorted(tail)} did not run: {sorted(seen)}"


@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_every_layer_against_the_float64_oracle(case, frames):
    """kenc, every gnn{l} tap, scores_in, Z and the matching scores element-wise at 1e-4 + 1e-4 |x64| on the valid rows of the three
    pairs of the frame (counts (256, 256), (200, 131), (256, 97); NaN past them), -1 / 0 past the counts, match indices equal to the
    float64 oracle's (index_excuses: at most 1 % of the keypoints, each printed); and the kernel forms are the shipped list's."""
    d, lname, ename, opts = case
    tag = G.case_id(case)
    cfg = G.config(d, lname, ename)
    eng = G.engine(d, lname, ename, opts)
    t, n0, n1 = frames[d]
    outs, seen = G.forward(eng, t, n0, n1, forms=True)
    dense = G.library_dense(eng, len(G.LISTS[lname]), G.COUNTS, float(G.state(d, lname, ename)["bin_score"]))
    if not G.LISTS[lname]:        # nothing projected a q|k|v and no layer has maxima: the taps are withdrawn
        from image_matching_amd.engine import ImxError
        for name in ("qkv", "amax"):
            with pytest.raises(ImxError, match="no tap named"):
                eng.fetch(name)
    G.check_against_oracle(tag, dense, outs, G.oracle(d, lname, ename), G.COUNTS, cfg["match_threshold"])
    check_forms(tag, seen, shipped_forms(d, ename, opts, frames), d, lname, opts)


BODY = ("rows_amax", "qkv_proj", "qkv_amax", "attention", "gnn_layer", "gnn_tail", "gnn_mlp1", "gnn_mlp2")
CHAINS = (("s", "ss", "sss"), ("c", "cs", "cs9"), ("sc17", "sc18", "alt19", "alt64"))


@pytest.mark.parametrize("d,opts", [(128, "A"), (128, "B"), (128, "C"), (256, "B")], ids=lambda v: str(v))
@pytest.mark.parametrize("chain", CHAINS, ids=lambda c: "<".join(c))
def test_a_layer_does_not_depend_on_what_follows_it(chain, d, opts, frames):
    """Same inputs, same options: gnn{l} of list P equals, bit for bit, gnn{l} of every list Q with Q[:l + 1] == P[:l + 1] -- whether
    layer l is the last one (its fused tail computes final_proj) or not (the next layer's q|k|v), and however many slots the tables
    have.  Should the timing report show another kernel form for a launch the two lists share (a chain-wide guard), it is printed and
    the taps are compared at the bar instead."""
    t, n0, n1 = frames[d]
    taps, forms = {}, {}
    longest = max(len(G.LISTS[n]) for n in chain[:-1])
    for name in chain:
        eng = G.engine(d, name, None, opts)
        _, seen = G.forward(eng, t, n0, n1, forms=True)
        forms[name] = {n: {f for m, f in seen if m == n} for n in BODY}
        taps[name] = [eng.fetch(f"gnn{l}") for l in range(min(len(G.LISTS[name]), longest))]
    for i, p in enumerate(chain):
        for q in chain[i + 1:]:
            P, Q = G.LISTS[p], G.LISTS[q]
            assert Q[:len(P)] == P
            other = {n: (forms[p][n], forms[q][n]) for n in BODY if forms[p][n] and forms[q][n] and forms[p][n] != forms[q][n]}
            for l in range(len(P)):
                a, b = taps[p][l], taps[q][l]
                if other:
                    print(f"[sg-shapes prefix] d{d} {opts}: {p} and {q} ran shared launches in different forms: {other}; gnn{l} compared at the bar")
                    util.assert_close(a, b, f"d{d} {opts}: gnn{l} of {p} vs {q}")
                else:
                    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), \
                        f"d{d} {opts}: gnn{l} of {p} differs from gnn{l} of {q} ({int((a != b).sum())} elements, max {np.abs(a - b).max():.3e})"


@pytest.mark.parametrize("opts", ["A", "B"])
def test_self_layers_do_not_see_the_other_side(opts):
    """Pairs (A, X) and (A, Y): with 'self' layers only (s x 18, sss) every gnn tap of side 0 has the same bits whatever side 1 holds;
    with one 'cross' layer it does not."""
    d = 128
    ax, ay = G.pair_inputs(d), G.pair_inputs(d, G.SEED, G.SEED_Y)
    assert torch.equal(ax["descriptors0"], ay["descriptors0"]) and not torch.equal(ax["descriptors1"], ay["descriptors1"])
    for lname in ("s18", "sss", "c"):
        eng = G.engine(d, lname, None, opts)
        side0 = []
        for t in (ax, ay):
            G.forward(eng, t)
            side0.append([eng.fetch(f"gnn{l}")[:G.K].copy() for l in range(len(G.LISTS[lname]))])
        for l, (a, b) in enumerate(zip(*side0)):
            if lname == "c":
                assert not np.array_equal(a, b), "a 'cross' layer must see the other side"
            else:
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{lname} {opts}: gnn{l} of side 0 depends on side 1 ({int((a != b).sum())} elements)"


@pytest.mark.parametrize("lname", ["cs9", "c18"])
def test_default_weights_anchored_on_float64(lname, frames):
    """The default weight set (heavy-tailed scores: the reference's own fp32 forward uses 0.7 of the bar at 18 layers) on cross-first
    and all-cross lists under "latency_forms" = off: the last tap, scores_in and Z as close to the oracle's float64 evaluation as the
    oracle's fp32 one is (util.assert_fp64_anchored, its constants), over the valid entries of the three pairs; indices by the rule
    of the element-wise test."""
    d = 128
    cfg = G.config(d, lname)
    eng = G.engine(d, lname, None, "B", variant="default")
    t, n0, n1 = frames[d]
    outs, _ = G.forward(eng, t, n0, n1)
    dense = G.library_dense(eng, 18, G.COUNTS, float(G.state(d, lname, None, "default")["bin_score"]))
    ref = G.oracle(d, lname, None, "default")
    flat = lambda rows: np.concatenate([np.asarray(r, np.float64).ravel() for r in rows])
    for what, pick in (("gnn17", lambda r: r["gnn"][17]), ("scores_in", lambda r: r["scores_in"]), ("Z", lambda r: r["Z"])):
        util.assert_fp64_anchored(flat(pick(x) for x in dense), flat(pick(r32) for r32, _ in ref), flat(pick(r64) for _, r64 in ref), f"{lname} default weights: {what}")
    G.check_against_oracle(f"d128-{lname}-default-B", dense, outs, ref, G.COUNTS, cfg["match_threshold"], anchored=True)


def test_create_serves_64_layers_and_refuses_65():
    from image_matching_amd import _lib
    lib = _lib.load_library()
    for layers, kenc_n, what in ((64, 3, None), (65, 3, b"num_gnn_layers 65"), (18, 0, b"keypoint_encoder length 0"), (18, 9, b"keypoint_encoder length 9")):
        h, cfg = ctypes.c_void_p(), _lib.ImxConfig()
        cfg.descriptor_dim, cfg.kenc_n, cfg.num_gnn_layers = 128, kenc_n, layers
        for i in range(min(kenc_n, _lib.IMX_MAX_KENC)):
            cfg.kenc_channels[i] = 32
        rc = lib.imx_create(0, ctypes.byref(cfg), ctypes.byref(h))
        if what is None:
            assert rc == 0 and h.value
            lib.imx_destroy(h)
        else:
            assert rc != 0 and not h.value and what in lib.imx_last_error(None), lib.imx_last_error(None)


def test_dropin_superglue_takes_the_list_and_names_a_missing_key():
    """The drop-in SuperGlue with GNN_layers = ssccs and a five-layer state dict gives the Engine-direct matches bit for bit; a state
    dict short of a layer raises an ImxError that names the first missing key."""
    from image_matching_amd import _lib as L
    from image_matching_amd.engine import Engine, ImxError
    from image_matching_amd.superglue.models.superglue_test import SuperGlue
    d, lname = 128, "ssccs"
    sd, data = G.state(d, lname), {k: v.cuda() for k, v in G.pair_inputs(d).items()}
    sg = SuperGlue(G.config(d, lname)).eval().to("cuda")
    sg.load_state_dict(sd)
    img = torch.zeros(G.SHAPE)
    pred = sg({**data, "image0": img, "image1": img})
    direct, _ = G.forward(G.engine(d, lname, debug=False), G.pair_inputs(d))
    for k, a in zip(("matches0", "matches1", "matching_scores0", "matching_scores1"), direct):
        assert np.array_equal(pred[k].cpu().numpy(), a), k
    assert int((pred["matches0"] > -1).sum()) > 20
    short = {k: v for k, v in sd.items() if not k.startswith("gnn.layers.4.")}
    eng = Engine(util.sp_config(d, G.K), G.config(d, lname), "cuda")
    with pytest.raises(ImxError, match=r"Missing key in state_dict: \"gnn\.layers\.4\."):
        eng.load_state_dict(L.NET_SUPERGLUE, short)
    with pytest.raises(RuntimeError, match=r"Missing key\(s\) in state_dict: \"gnn\.layers\.4\."):
        sg.load_state_dict(short)


def test_matching_from_images_with_three_self_layers():
    """One Matching forward from images with GNN_layers = sss against oracle/matching_ref.py: the keypoint sets equal the oracle's, and
    the SuperGlue half is held by the end-to-end rule of test_gpu_matching.py -- the oracle on the call's own features, matching scores
    at 1e-4 where the indices agree, an index may differ only where the oracle's transport matrix has a margin below 2e-3."""
    from image_matching_amd.superglue.models.matching_test import Matching
    from oracle import matching_ref, superglue_ref
    d, lname = 128, "sss"
    cfg = {"superpoint": util.sp_config(d, G.K), "superglue": G.config(d, lname)}
    sd_sp, sd_sg = util.sp_sd(d), G.state(d, lname)
    m = Matching(cfg).eval().to("cuda")
    m.superpoint.load_state_dict(sd_sp)
    m.superglue.load_state_dict(sd_sg)
    x0, x1 = util.pair(G.SEED, G.H, G.W)
    pred = m({"image0": x0.cuda(), "image1": x1.cuda()})
    ref = matching_ref.matching_forward({"image0": x0, "image1": x1}, sd_sp, sd_sg, cfg)
    for side in "01":
        mine, want = pred["keypoints" + side][0].cpu().numpy().astype(int), ref["keypoints" + side][0].numpy().astype(int)
        assert set(map(tuple, mine)) == set(map(tuple, want)), f"keypoint set of image {side}"
    data = {k: (pred[k][0][None].cpu()) for k in G.KEYS}
    own = superglue_ref.superglue_forward({**data, "image_shape0": G.SHAPE, "image_shape1": G.SHAPE}, sd_sg, cfg["superglue"], return_dense=True)
    Z = own["dense"]["Z"][0].numpy()[:-1, :-1]
    r0, mine0 = own["matches0"][0].numpy(), pred["matches0"][0].cpu().numpy()
    thr = np.log(cfg["superglue"]["match_threshold"])
    srt_r, srt_c = np.sort(Z, axis=1), np.sort(Z, axis=0)
    gap_r, gap_c = srt_r[:, -1] - srt_r[:, -2], srt_c[-1] - srt_c[-2]
    for i in np.nonzero(mine0 != r0)[0]:
        j = int(Z[i].argmax())
        assert gap_r[i] < 2e-3 or gap_c[j] < 2e-3 or abs(Z[i, j] - thr) < 2e-3, f"matches0[{i}] = {mine0[i]}, oracle {r0[i]}"
    same = mine0 == r0
    util.assert_close(pred["matching_scores0"][0].cpu().numpy()[same], own["matching_scores0"][0].numpy()[same], "matching_scores0")
    assert int((mine0 > -1).sum()) > 20
    mp = lambda p, k0, k1: {(tuple(np.asarray(k0[i]).astype(int)), tuple(np.asarray(k1[j]).astype(int))) for i, j in enumerate(p) if j >= 0}
    both = mp(mine0, pred["keypoints0"][0].cpu().numpy(), pred["keypoints1"][0].cpu().numpy()) ^ mp(ref["matches0"][0].numpy(), ref["keypoints0"][0].numpy(), ref["keypoints1"][0].numpy())
    print(f"[sg-shapes] Matching with sss: {int((mine0 > -1).sum())} matches, {len(both)} matched pairs differ from oracle/matching_ref's on its own features")
    assert len(both) <= 0.01 * 2 * G.K


def test_a_trained_two_layer_state_loads_into_the_inference_class():
    """What superpoint_glue_train.py writes: the state dict of a two-layer ['self', 'cross'] SuperGlueTrainable (PyTorch's
    initialisation, seeded) loaded into the inference SuperGlue, at 256 keypoints under "latency_forms" = off, against the oracle at the
    bar."""
    from image_matching_amd import _lib as L
    from image_matching_amd.sgtrain_model import SuperGlueTrainable
    from image_matching_amd.superglue.models.superglue_test import SuperGlue
    d, lname = 128, "sc"
    cfg = G.config(d, lname)
    torch.manual_seed(5)
    sd = {k: v.detach().clone() for k, v in SuperGlueTrainable({**cfg, "weights": ""}).state_dict().items()}
    sg = SuperGlue(cfg).eval().to("cuda")
    sg.load_state_dict(sd)
    eng = sg._shared.get_engine([L.NET_SUPERGLUE])
    eng.set_option("latency_forms", "off")
    eng.set_debug(True)
    data = G.pair_inputs(d)
    img = torch.zeros(G.SHAPE)
    pred = sg({**{k: v.cuda() for k, v in data.items()}, "image0": img, "image1": img})
    torch.cuda.synchronize()
    outs = [pred[k].cpu().numpy() for k in ("matches0", "matches1", "matching_scores0", "matching_scores1")]
    sdf = {k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")}
    ref = [(G.oracle_run(sdf, cfg, data, torch.float32), G.oracle_run(sdf, cfg, data, torch.float64))]
    dense = G.library_dense(eng, 2, ((G.K, G.K),), float(sd["bin_score"]))
    G.check_against_oracle("trained sc, 256 keypoints, B", dense, outs, ref, ((G.K, G.K),), cfg["match_threshold"])


@pytest.mark.parametrize("net", G.TV_NETS, ids=lambda n: f"d{n[0]}-{n[1]}")
def test_the_maximum_of_x_reaches_the_next_layer(net, frames):
    """The hand-off of max |x'| from one fused fp16-plane tail to the next (amax_x + 2 B (l + 1)), on the "tv" weight set, whose v
    projection is small: there a layer's x operand is scaled by the table entry alone (with the "t" set the v-maximum, which the kernel
    also takes into the bound, is the larger and hides a missing entry).  The element-wise test, under "latency_forms" = off, and the
    shipped run's gnn_tail form must be the one that ran."""
    d, lname = net
    tag = f"d{d}-{lname}-tv-B"
    eng = G.engine(d, lname, None, "B", variant="tv")
    t, n0, n1 = frames[d]
    outs, seen = G.forward(eng, t, n0, n1, forms=True)
    dense = G.library_dense(eng, len(G.LISTS[lname]), G.COUNTS, float(G.state(d, lname, None, "tv")["bin_score"]))
    G.check_against_oracle(tag, dense, outs, G.oracle(d, lname, None, "tv"), G.COUNTS, G.config(d, lname)["match_threshold"])
    check_forms(tag, seen, shipped_forms(d, None, "B", frames), d, lname, "B")


@pytest.mark.parametrize("net", G.LOPSIDED_NETS, ids=lambda n: f"d{n[0]}-{n[1]}")
def test_the_cross_flag_chooses_the_side_that_bounds_att(net, frames):
    """The lopsided pair (side 1's positions x 24: its v-maximum is more than 16 times side 0's) with the "tq" weights under
    "latency_forms" = off: kenc and every layer's output at the bar against the oracle's float64.  A layer that bounds att by the wrong
    side's v-maximum -- the fused tail at d = 128, gnn_mlp1 on the fp16 planes at d = 256 -- is off by four binades here.  scores_in
    and Z are not held: the reference's own fp32 forward is outside the bar on them at these magnitudes (test_sg_shapes_host.py)."""
    d, lname = net
    tag = f"d{d}-{lname}-lopsided-B"
    sd, cfg, p = G.state(d, lname, None, "tq"), G.config(d, lname), G.lopsided_pair(d)
    eng = G.engine(d, lname, None, "B", sd=sd)
    _, seen = G.forward(eng, p, forms=True)
    got = G.library_dense(eng, len(G.LISTS[lname]), ((G.K, G.K),), float(sd["bin_score"]))[0]
    fr = G.dense_fractions(got, G.oracle_run(sd, cfg, p, torch.float64))
    print(f"[sg-shapes] {tag}: fraction of the bar used: kenc {fr['kenc']:.3f}, gnn {fr['gnn']:.3f} (layer {fr['gnn_layer']}); not held: scores_in {fr['scores_in']:.3f}, Z {fr['Z']:.3f}")
    assert fr["kenc"] <= 1.0 and fr["gnn"] <= 1.0, f"{tag}: {fr}"
    want = shipped_forms(d, None, "B", frames)
    name = "gnn_tail" if d == 128 else "gnn_mlp1"
    meant = {(n, f) for n, f in want if n == name}
    assert meant and meant <= seen, f"{tag}: the shipped run's {name} form {sorted(meant)} did not run: {sorted(seen)}"


@pytest.mark.parametrize("opts", ["A", "B"])
def test_a_non_finite_valid_row_gets_no_partner(opts):
    """A NaN descriptor in one VALID row (row 5 of side 0): the match extraction must not use an argmax that was never set as an index
    (a row or column of Z that is all NaN keeps the sentinel of match_rowmax / match_colmax, which match_finalize used to index with).
    By the reference's own arithmetic the NaN does not stay in its row: it is a key of the first self-attention, so every side-0 row
    becomes NaN, the cross layer carries it to side 1, and the Sinkhorn column pass would spread a single NaN row of the scores
    anyway.  So this is a forward in which EVERY row and column takes the guarded path, not one: what is asserted is that the call
    returns without touching memory it does not own, that row 5 is unmatched with score 0, and that every output is well-formed --
    indices in [-1, n), matches0 / matches1 consistent, scores finite and not negative -- whichever rows a kernel form leaves finite."""
    d, lname, bad = 128, "sc", 5
    p = {k: v.clone() for k, v in G.pair_inputs(d).items()}
    p["descriptors0"][0, :, bad] = float("nan")
    eng = G.engine(d, lname, None, opts, debug=False)
    (m0, m1, ms0, ms1), _ = G.forward(eng, p)
    assert m0[0, bad] == -1 and ms0[0, bad] == 0 and not (m1[0] == bad).any()
    assert ((m0 >= -1) & (m0 < G.K)).all() and ((m1 >= -1) & (m1 < G.K)).all()
    i = np.nonzero(m0[0] > -1)[0]
    assert np.array_equal(m1[0][m0[0][i]], i)
    assert np.isfinite(ms0).all() and np.isfinite(ms1).all() and (ms0 >= 0).all() and (ms1 >= 0).all()
