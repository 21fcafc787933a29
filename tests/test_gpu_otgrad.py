"""The SuperGlue match loss and its gradient through the unrolled Sinkhorn on the GPU (imx_ot_match_loss_grad,
Engine.ot_match_loss_grad, image_matching_amd.sgtrain_grad) against the project's restatement in float64 (tests/otgrad_ref.py, itself
held to the reference's autograd by tests/test_otgrad_host.py) and against the samples, row sums and column sums the reference's own
autograd wrote (tests/golden/make_golden_otgrad.py).  The default bar, element-wise, at gout = n_all (the direct term is -1 per listing
and the gradient O(1)): |g - g64| <= max(1e-4 + 1e-4 |g64|, 2.5 |ref32 - g64|); where the reference's fp32 gradient is not at hand
(full maps, sums) the first term alone.  Row sums, column sums, d bin_score and the descriptor gradients behind the einsum are held to the
same bar on their own values.  Needs an MI355X; a few seconds per test."""
import numpy as np
import pytest
import torch

from tests import otgrad_ref as O
from tests import util
from tests.golden.make_golden_otgrad import CASES, RAGGED_FRAME, sample_positions

pytestmark = pytest.mark.gpu
D = 128


def new_engine():
    from image_matching_amd.engine import Engine
    return Engine(util.sp_config(D, 256), util.sg_config(D), "cuda")


@pytest.fixture(scope="module")
def eng():
    return new_engine()


def cuda(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def item(g, k):
    return {key[:-len(f"_{k}")]: v for key, v in g.items() if key.endswith(f"_{k}")}


def frame(pairs, N0=None, N1=None, L=None, fill=np.nan):
    """[(scores (m,n), matches (2,K))] -> scores (B,N0,N1) with `fill` on the padding, all_matches (B,2,L) with an index far outside past
    each count (never read), n_all, n0, n1"""
    N0 = N0 or max(s.shape[0] for s, _ in pairs)
    N1 = N1 or max(s.shape[1] for s, _ in pairs)
    L = L or max(max(mt.shape[1] for _, mt in pairs), 1)
    S = np.full((len(pairs), N0, N1), fill, np.float32)
    am = np.full((len(pairs), 2, L), 1 << 40, np.int64)
    for b, (s, mt) in enumerate(pairs):
        S[b, :s.shape[0], :s.shape[1]] = s
        am[b, :, :mt.shape[1]] = mt
    return (S, am, np.array([mt.shape[1] for _, mt in pairs], np.int32), np.array([s.shape[0] for s, _ in pairs], np.int32),
            np.array([s.shape[1] for s, _ in pairs], np.int32))


def call(eng, S, am, n_all, iters, n0=None, n1=None, gout="n_all", bin_score=1.0, want_grad=True):
    """-> dict of numpy arrays; gout 'n_all': each pair's own count (the bar's scale), None: NULL"""
    go = cuda(n_all.astype(np.float32)) if isinstance(gout, str) else None if gout is None else cuda(gout)
    res = eng.ot_match_loss_grad(cuda(S), bin_score, cuda(am, torch.int64), cuda(n_all, torch.int32), iters,
                                 n0=None if n0 is None else cuda(n0, torch.int32), n1=None if n1 is None else cuda(n1, torch.int32),
                                 gout=go, want_grad=want_grad)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def frac(got, g64, d32=None):
    got, g64 = np.asarray(got, np.float64), np.asarray(g64, np.float64)
    return float(np.max(np.abs(got - g64) / O.bar(g64, d32))) if got.size else 0.0


def against_restatement(res, S, am, n_all, iters, n0=None, n1=None, bin_score=1.0):
    """the kernels against the float64 restatement in full at gout = n_all: the worst fraction of the default bar over d scores, over
    d bin_score, and of 1e-4 + 1e-4 |ref| on the value"""
    loss, g, gbin, flag = O.batch_loss_grad(S, bin_score, am, n_all, iters, n0, n1, gout=n_all.astype(np.float64))
    assert np.array_equal(res["flag"], flag)
    f = frac(res["grad_scores"], g)
    fb = frac(res["grad_bin"], gbin)
    fin = np.isfinite(res["loss"])
    if not fin.all():                                                    # an fp32 exp that underflowed: float64 does not show it, the fp32 restatement does
        loss32 = O.batch_loss_grad(S, bin_score, am, n_all, iters, n0, n1, dtype=torch.float32)[0]
        assert np.array_equal(res["loss"][~fin], loss32[~fin].astype(np.float32))
    assert np.isfinite(loss[fin]).all()
    fl = float(np.max(np.abs(res["loss"][fin] - loss[fin]) / (1e-4 + 1e-4 * np.abs(loss[fin])))) if fin.any() else 0.0
    return f, fb, fl


def same_bits(a, b, keys=("loss", "grad_scores", "grad_bin", "flag")):
    return all(np.array_equal(a[k].view(np.int32), b[k].view(np.int32)) for k in keys if k in a and k in b)


# ---------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("name", list(CASES))
def test_reference_fixtures(eng, name):
    """samples, row sums, column sums and d bin_score against the reference's float64 autograd; the value within 1e-4 + 1e-4 |ref|"""
    g = util.golden(f"otgrad_{name}.npz")
    worst = [0.0, 0.0, 0.0, 0.0]
    for k in range(int(g["n_items"])):
        it = item(g, k)
        S, am, n_all, _, _ = frame([(it["scores"], it["matches"])])
        K, T = int(n_all[0]), int(it["iters"])
        res = call(eng, S, am, n_all, T, bin_score=float(it["bin"]))
        got = res["grad_scores"][0].astype(np.float64)
        pos = sample_positions(int(it["seed"]), got.size)
        worst[0] = max(worst[0], frac(got.reshape(-1)[pos], K * it["g"], K * it["d32"].astype(np.float64)))
        worst[1] = max(worst[1], frac(got.sum(1), K * it["rows"]), frac(got.sum(0), K * it["cols"]))
        worst[2] = max(worst[2], float(abs(res["grad_bin"][0] - K * it["gbin64"]) / O.bar(K * it["gbin64"], K * (it["gbin32"] - it["gbin64"]))))
        worst[3] = max(worst[3], float(abs(res["loss"][0] - it["loss64"]) / (1e-4 + 1e-4 * abs(it["loss64"]))))
    print(f"{name}: of the bar -- samples {worst[0]:.3g}, row and column sums {worst[1]:.3g}, d bin_score {worst[2]:.3g}, value {worst[3]:.3g}")
    assert max(worst) <= 1.0


@pytest.mark.parametrize("shape", [(7, 5), (33, 40)])
def test_iterations_0_to_3(eng, shape):
    """a dropped or reordered half-step moves the result by O(0.1) here"""
    s, mt = O.case_scores(21 + shape[0], *shape)
    worst = 0.0
    for T in (0, 1, 2, 3):
        S, am, n_all, _, _ = frame([(s, mt)])
        f = against_restatement(call(eng, S, am, n_all, T), S, am, n_all, T)
        print(f"{shape} T={T}: {f[0]:.3g} of the bar on d scores, {f[1]:.3g} on d bin_score, {f[2]:.3g} on the value")
        worst = max(worst, *f)
    assert worst <= 1.0


@pytest.mark.parametrize("shape", [(1, 1), (1, 40), (3, 2080), (15, 32), (64, 64), (65, 63), (1023, 1024), (1024, 1024)])
def test_tile_edge_shapes(eng, shape):
    """T = 3; (1023,1024) and (1024,1024): the dustbin row closes or opens a tile"""
    s, mt = O.case_scores(40 + shape[0] + shape[1], *shape)
    S, am, n_all, _, _ = frame([(s, mt)])
    f = against_restatement(call(eng, S, am, n_all, 3), S, am, n_all, 3)
    print(f"{shape}: {f[0]:.3g} of the bar on d scores, {f[1]:.3g} on d bin_score, {f[2]:.3g} on the value")
    assert max(f) <= 1.0


def ragged_pairs():
    g = util.golden("otgrad_ragged.npz")
    return [(item(g, k)["scores"], item(g, k)["matches"]) for k in range(3)], int(item(g, 0)["iters"])


def test_ragged_batch(eng):
    """B = 3 under one (N0, N1): NaN on the padding in, 0 out; each pair's bits equal its B = 1 call, padded or not"""
    pairs, T = ragged_pairs()
    S, am, n_all, n0, n1 = frame(pairs, *RAGGED_FRAME)
    assert np.isnan(S).any()
    res = call(eng, S, am, n_all, T, n0, n1)
    f = against_restatement(res, S, am, n_all, T, n0, n1)
    print(f"ragged batch: {f[0]:.3g} of the bar on d scores, {f[1]:.3g} on d bin_score, {f[2]:.3g} on the value")
    assert max(f) <= 1.0
    for b, (s, mt) in enumerate(pairs):
        m, n = s.shape
        assert not res["grad_scores"][b, m:].any() and not res["grad_scores"][b, :, n:].any(), "0 on the padding, not NaN"
        one = call(eng, S[b:b + 1], am[b:b + 1], n_all[b:b + 1], T, n0[b:b + 1], n1[b:b + 1])
        own = call(eng, *frame([(s, mt)])[:3], T)
        for r, sl in ((one, (0,)), (own, (0,))):
            assert r["loss"][0].view(np.int32) == res["loss"][b].view(np.int32) and r["grad_bin"][0].view(np.int32) == res["grad_bin"][b].view(np.int32)
        assert np.array_equal(one["grad_scores"][0].view(np.int32), res["grad_scores"][b].view(np.int32))
        assert np.array_equal(own["grad_scores"][0].view(np.int32), res["grad_scores"][b, :m, :n].view(np.int32))


# ---------------------------------------------------------------------------------------------- the list
def test_list_edge_cases(eng):
    s, mt = O.case_scores(61, 37, 29)
    m, n = s.shape
    dust = np.stack([np.arange(m), np.full(m, n)])                       # every row against the dustbin column
    dup = np.concatenate([mt, mt[:, 3:4], mt[:, 3:4]], 1)                # one entry three times
    bad = np.concatenate([mt[:, :5], np.array([[m + 1, -1, 0], [0, 0, n + 1]]), mt[:, 5:]], 1)
    empty = mt[:, :0]
    pairs = [(s, empty), (s, dust), (s, dup), (s, bad), (s, mt)]
    S, am, n_all, _, _ = frame(pairs)
    res = call(eng, S, am, n_all, 5)
    f = against_restatement(res, S, am, n_all, 5)
    print(f"list cases: {f[0]:.3g} of the bar on d scores, {f[1]:.3g} on d bin_score, {f[2]:.3g} on the value")
    assert max(f) <= 1.0
    assert res["loss"][0] == 0 and not res["grad_scores"][0].any() and res["grad_bin"][0] == 0, "n_all = 0: loss 0, zero gradients"
    assert res["flag"].tolist() == [0, 0, 0, O.FLAG_INDEX, 0]
    # the duplicated entry counts three times: its direct term at gout = n_all is -3, against -1 in the plain list
    x, y = mt[:, 3]
    assert x < m and y < n
    direct = res["grad_scores"][2][x, y] - res["grad_scores"][4][x, y]
    assert abs(direct + 2.0) < 0.05, direct
    # the flagged entries are inert: the same list without them, at the same cotangent per listing, gives the same bits
    clean = np.concatenate([mt[:, :5], mt[:, 5:]], 1)
    Sc, amc, nc, _, _ = frame([(s, clean)])
    ref = call(eng, Sc, amc, nc, 5, gout=np.array([nc[0]], np.float32))
    flagged = call(eng, Sc, am[3:4], n_all[3:4], 5, gout=np.array([n_all[3]], np.float32))
    assert np.array_equal(ref["grad_scores"].view(np.int32), flagged["grad_scores"].view(np.int32)) and flagged["flag"][0] == O.FLAG_INDEX
    # gout per pair; NULL = 1
    go = np.array([2.0, -0.5, 3.0, 1.0, 0.25], np.float32)
    scaled, unit, ones = call(eng, S, am, n_all, 5, gout=go), call(eng, S, am, n_all, 5, gout=None), call(eng, S, am, n_all, 5, gout=np.ones(5, np.float32))
    assert same_bits(unit, ones), "NULL means 1"
    l64, g64, b64, _ = O.batch_loss_grad(S, 1.0, am, n_all, 5, gout=go.astype(np.float64) * n_all)
    fg, fgb = frac(scaled["grad_scores"] * n_all[:, None, None], g64), frac(scaled["grad_bin"] * n_all, b64)
    print(f"per-pair gout {go.tolist()}: {fg:.3g} of the bar on d scores, {fgb:.3g} on d bin_score")
    assert max(fg, fgb) <= 1.0 and same_bits(scaled, unit, keys=("loss", "flag"))


def test_underflowing_listed_entries(eng):
    """a listed entry whose exp underflows: the value is +inf, the gradient finite and the restatement's (the derivative of -Z)"""
    s, mt = O.case_scores(62, 20, 24)
    s = s.copy()
    x, y = mt[:, 0]
    s[x, y] = -400.0
    S, am, n_all, _, _ = frame([(s, mt)])
    res = call(eng, S, am, n_all, 4)
    assert np.isposinf(res["loss"][0]) and np.isfinite(res["grad_scores"]).all() and np.isfinite(res["grad_bin"]).all()
    f = against_restatement(res, S, am, n_all, 4)
    print(f"underflow: {f[0]:.3g} of the bar on d scores, {f[1]:.3g} on d bin_score")
    assert max(f) <= 1.0


# ---------------------------------------------------------------------------------------------- determinism
def test_equal_bits_between_calls_histories_and_handles(eng):
    pairs, T = ragged_pairs()
    S, am, n_all, n0, n1 = frame(pairs, *RAGGED_FRAME)
    first = call(eng, S, am, n_all, T, n0, n1)
    assert same_bits(first, call(eng, S, am, n_all, T, n0, n1)), "the same call twice"
    big, small = O.case_scores(63, 130, 70), O.case_scores(64, 9, 11)
    call(eng, *frame([big])[:3], 7)                                      # grows every workspace
    call(eng, *frame([small])[:3], 2)
    assert same_bits(first, call(eng, S, am, n_all, T, n0, n1)), "after calls of other sizes"
    for pattern in ("nan", "huge"):
        other = new_engine()                                             # a fresh handle: every workspace it allocates is poisoned
        other.set_option("debug_poison", pattern)
        try:
            assert same_bits(first, call(other, S, am, n_all, T, n0, n1)), f"a second handle, workspaces poisoned with {pattern}"
            call(other, *frame([big])[:3], 7)                            # (grown, poisoned again)
            assert same_bits(first, call(other, S, am, n_all, T, n0, n1))
        finally:
            other.set_option("debug_poison", "off")
    value = call(eng, S, am, n_all, T, n0, n1, want_grad=False)
    assert set(value) == {"loss", "flag"} and same_bits(first, value), "the value-only mode gives the same value"


# ---------------------------------------------------------------------------------------------- the bridge to autograd
def test_autograd_bridge(eng):
    """scores = einsum(mdesc0, mdesc1) / sqrt(d) with leaf descriptors (d = 32, 40 x 36); .grad against the float64 chain through the
    restatement, at the default bar on the descriptor gradients and on bin_score.grad, at gout = n_all."""
    from image_matching_amd import sgtrain_grad
    d, m, n, T = 32, 40, 36, 6
    rng = np.random.default_rng(7)
    a0, a1 = rng.standard_normal((1, d, m)).astype(np.float32) * 2, rng.standard_normal((1, d, n)).astype(np.float32) * 2
    _, mt = O.case_scores(65, m, n)
    K = mt.shape[1]
    md0, md1 = cuda(a0).requires_grad_(True), cuda(a1).requires_grad_(True)
    bin_score = torch.nn.Parameter(torch.tensor(1.0, device="cuda"))
    with torch.enable_grad():                                            # (whatever an imported module left as the global mode)
        scores = (torch.einsum("bdn,bdm->bnm", md0, md1) / d ** .5).contiguous()
        loss = sgtrain_grad.match_loss(eng, scores, bin_score, cuda(mt[None], torch.int64), cuda(np.array([K]), torch.int32), T)
        assert loss.shape == (1,) and loss.requires_grad
        (loss * K).sum().backward()
    S64 = np.einsum("dn,dm->nm", a0[0].astype(np.float64), a1[0].astype(np.float64)) / d ** .5
    l64, g64, b64, _ = O.loss_grad(S64, 1.0, mt, T, gout=K)
    r0, r1 = a1[0].astype(np.float64) @ g64.T / d ** .5, a0[0].astype(np.float64) @ g64 / d ** .5
    f0, f1, fb = frac(md0.grad[0].cpu().numpy(), r0), frac(md1.grad[0].cpu().numpy(), r1), frac(float(bin_score.grad), b64)
    print(f"bridge: {f0:.3g} / {f1:.3g} of the bar on the descriptor gradients, {fb:.3g} on bin_score.grad, loss {float(loss[0]):.5f} against {l64:.5f}")
    assert bin_score.grad.shape == bin_score.shape and max(f0, f1, fb) <= 1.0 and abs(float(loss[0]) - l64) <= 1e-4 + 1e-4 * abs(l64)
    from image_matching_amd.engine import ImxError
    with pytest.raises(ImxError, match="contiguous fp32 cuda"):
        sgtrain_grad.match_loss(eng, scores.detach().transpose(1, 2), bin_score, cuda(mt[None], torch.int64), cuda(np.array([K]), torch.int32), T)


# ---------------------------------------------------------------------------------------------- the forward is untouched
def test_forward_unchanged_by_a_gradient_call():
    from image_matching_amd import _lib as L
    from image_matching_amd.engine import Engine
    g = util.golden("sg_small.npz")
    e = Engine(util.sp_config(D, 1024), util.sg_config(D), "cuda")
    e.load_state_dict(L.NET_SUPERGLUE, util.sg_sd(D))
    t = {k: torch.from_numpy(g[k]).cuda() for k in ("keypoints0", "keypoints1", "scores0", "scores1", "descriptors0", "descriptors1")}
    shp = (1, 1, 120, 160)

    def forward():
        out = e.superglue(t["keypoints0"], t["scores0"], t["descriptors0"], shp, t["keypoints1"], t["scores1"], t["descriptors1"], shp)
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in out]
    before = forward()
    N0, N1 = g["keypoints0"].shape[1], g["keypoints1"].shape[1]
    s, mt = O.case_scores(66, N0, N1)
    S, am, n_all, _, _ = frame([(s, mt)], L=N0 + N1)
    res = call(e, S, am, n_all, 30)
    assert np.isfinite(res["grad_scores"]).all()
    after = forward()
    assert all(np.array_equal(a.view(np.int32) if a.dtype == np.float32 else a, b.view(np.int32) if b.dtype == np.float32 else b) for a, b in zip(before, after))
    loss = e.match_loss(cuda(am, torch.int64), cuda(n_all, torch.int32))
    call(e, S, am, n_all, 30)                                            # a gradient call between the forward and its loss: the record stays
    again = e.match_loss(cuda(am, torch.int64), cuda(n_all, torch.int32))
    assert loss.shape == (1,) and torch.equal(loss.view(torch.int32), again.view(torch.int32))


# ---------------------------------------------------------------------------------------------- the CLI
def test_export_cli_prints_gradient_norms(tmp_path, capsys):
    """superglue_export_pairs.py --synthetic 2 --grads: the gradient line beside the loss, its value within the default bar of the forward's"""
    import re
    import superglue_export_pairs
    superglue_export_pairs.main(["--synthetic", "2", "--grads", "--out_dir", str(tmp_path), "--batch", "2", "--seed", "4"])
    text = capsys.readouterr().out
    val = re.search(r"validation over (\d+) pairs: loss ([-+.\w]+)", text)
    grd = re.search(r"gradients over (\d+) pairs: loss ([-+.\w]+) .*d scores\| ([-+.\w]+)  mean d loss / d bin_score ([-+.\w]+)", text)
    assert val and grd and val.group(1) == grd.group(1), text
    lv, lg, norm, gbin = float(val.group(2)), float(grd.group(2)), float(grd.group(3)), float(grd.group(4))
    print(text)
    if np.isfinite(lv):
        assert abs(lg - lv) <= 2e-4 + 1e-4 * abs(lv)                     # (both printed to four decimals)
    assert np.isfinite(norm) and norm > 0 and np.isfinite(gbin)
