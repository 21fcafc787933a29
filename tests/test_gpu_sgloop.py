"""The matches of SuperGlue's training forward from the loss's own Sinkhorn on the GPU (libimx_sgloop.so: imx_assignment_matches,
imx_ot_match_loss_grad_matches; Engine, image_matching_amd.sgtrain_grad, sgtrain_model.SuperGlueTrainable) and the training loop on top
of them (superglue/train_loop.py, superpoint_glue_train.py).  The references are tests/scoregrad_ref.transport / matches_of /
top_two_margins in float64 on tests/otgrad_ref.case_scores, and the fixtures the reference's own code wrote (tests/golden/otgrad_*.npz,
sgmodel_step.npz).

The comparison rule for matches: indices equal the float64 reference's, except at keypoints whose float64 top-two margin in Z is below
MARGIN (1e-3) or whose float64 matching score lies within 1e-4 of the threshold; those left out are at most MARGIN_CAP (5 %) of all.
The matching scores of the kept ones at the default bar max(1e-4 + 1e-4 |x64|, 2.5 |ref32 - x64|), ref32 the same restatement in
fp32.  Needs an MI355X; a few seconds per test."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import otgrad_ref as O
from tests import scoregrad_ref as R
from tests import util
from tests.golden.make_golden_otgrad import CASES as OT_CASES
from tests.golden.make_golden_sgmodel import ADAM_LR, ADAM_STEPS, MARGIN, MARGIN_CAP

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 128
THRESHOLD, NEAR = 0.2, 1e-4
# (seed, m, n, iterations): one element, one row, one column, around the 64-lane and 32-row tiles, several workgroups, odd sizes
SHAPES = ((1, 1, 1, 5), (2, 1, 7, 5), (3, 7, 1, 5), (4, 63, 65, 20), (5, 64, 64, 20), (6, 65, 63, 20), (7, 129, 200, 30), (8, 257, 130, 30),
          (9, 300, 513, 100))
RAGGED_COUNTS, RAGGED_FRAME, RAGGED_ITERS = ((40, 33), (23, 48), (0, 17)), (48, 48), 20
KEYS = ("matches0", "matches1", "matching_scores0", "matching_scores1")


@pytest.fixture(autouse=True)
def grad_enabled():
    """(a test module that imports one of the inference scripts switches autograd off for the whole process)"""
    with torch.enable_grad():
        yield


def new_engine():
    from image_matching_amd.engine import Engine
    return Engine(util.sp_config(D, 256), util.sg_config(D), "cuda")


@pytest.fixture(scope="module")
def eng():
    return new_engine()


def cuda(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def host(res):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def same_bits(a, b, keys=None):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in (keys or a))


# ---------------------------------------------------------------------------------------------- the float64 reference, computed once
@functools.lru_cache(maxsize=None)
def reference(seed, m, n, iters, bin_score=1.0, scores_key=None):
    """the float64 statement of one pair: potentials, matches, scores, margins, and the fp32 restatement's scores -> dict of numpy arrays
    (read-only).  scores_key names a fixture item instead of a seeded case."""
    s = _FIXTURE_SCORES[scores_key] if scores_key is not None else O.case_scores(seed, m, n)[0]
    out = {"scores": s}
    for dtype, tag in ((torch.float64, "64"), (torch.float32, "32")):
        S = torch.from_numpy(s).to(dtype)
        Z = R.transport(S, torch.tensor(bin_score, dtype=dtype), iters)
        m0, m1, ms0, ms1 = R.matches_of(Z, THRESHOLD)
        out.update({f"matches0_{tag}": m0.numpy(), f"matches1_{tag}": m1.numpy(), f"ms0_{tag}": ms0.double().numpy(), f"ms1_{tag}": ms1.double().numpy()})
        if dtype == torch.float64:
            g0, g1 = R.top_two_margins(Z)
            C, log_mu, log_nu, _ = O.coupling(s, bin_score, dtype)
            u, v = O.potentials(C, log_mu, log_nu, iters)
            out.update({"margin0": g0.numpy(), "margin1": g1.numpy(), "u": u[-1].numpy(), "v": v[-1].numpy()})
    for a in out.values():
        a.setflags(write=False)
    return out


_FIXTURE_SCORES = {}


def by_the_rule(got, ref, what):
    """the comparison rule of the module docstring on one pair (got: the four arrays cut to the counts) -> (left out, keypoints, the worst
    fraction of the bar over the kept scores)"""
    left, total, worst = 0, 0, 0.0
    for side in ("0", "1"):
        ms64 = ref[f"ms{side}_64"]
        keep = (ref[f"margin{side}"] >= MARGIN) & (np.abs(ms64 - THRESHOLD) > NEAR)
        left, total = left + int((~keep).sum()), total + keep.size
        g = got[f"matches{side}"]
        assert g.dtype == np.int64 and g.shape == ref[f"matches{side}_64"].shape, (what, side)
        assert np.array_equal(g[keep], ref[f"matches{side}_64"][keep]), (what, side, np.flatnonzero(g[keep] != ref[f"matches{side}_64"][keep]))
        ms = got[f"matching_scores{side}"].astype(np.float64)
        if keep.any():
            worst = max(worst, float(np.max(np.abs(ms[keep] - ms64[keep]) / R.bar(ms64[keep], ref[f"ms{side}_32"][keep] - ms64[keep]))))
    assert left <= MARGIN_CAP * total, (what, left, total)
    return left, total, worst


def cut(res, b, m, n):
    return {"matches0": res["matches0"][b, :m], "matches1": res["matches1"][b, :n], "matching_scores0": res["matching_scores0"][b, :m],
            "matching_scores1": res["matching_scores1"][b, :n]}


# ---------------------------------------------------------------------------------------------- 1. exact, the extraction alone
def numpy_matches(z):
    """superglue_train.py:276-286 in numpy with first-occurrence argmax; z any array whose ORDER is that of Z -> (m0, m1, mutual0, mutual1)"""
    i0, i1 = z.argmax(1), z.argmax(0)
    mut0, mut1 = i1[i0] == np.arange(z.shape[0]), i0[i1] == np.arange(z.shape[1])
    return i0, i1, mut0, mut1


def integer_scores(seed, m, n):
    """integers in [-64, 64] (many exact ties), with a duplicated row and a duplicated column planted where the shape allows"""
    rng = np.random.RandomState(seed)
    s = rng.randint(-64, 65, size=(m, n)).astype(np.float32)
    if m > 2:
        s[m - 1] = s[0]
        s[m // 2] = s[0]
    if n > 2:
        s[:, n - 1] = s[:, 1 % n]
        s[:, n // 2] = s[:, 1 % n]
    return s


@pytest.mark.parametrize("seed,m,n,_iters", SHAPES)
def test_exact_on_integer_scores(eng, seed, m, n, _iters):
    """NULL potentials, integer scores |s| <= 64: Z = s + log(m + n) in fp32 keeps the order and the ties of the integers (one constant
    added to all, rounding is monotone, distinct integers stay >= 1 - 2^-16 apart), so indices and mutual flags equal numpy's
    first-occurrence argmax EXACTLY; among the planted duplicates the lowest index wins on both sides; threshold 0 keeps every mutual
    pair, the largest float keeps none; stats against a numpy restatement.  The scores within 3e-5 relative of exp(s + log(m + n)):
    |Z| < 128 has half-ulp 2^-18 ~ 3.8e-6, twice (the sum, the normaliser), plus logf's and expf's few ulp."""
    s = integer_scores(seed, m, n)
    i0, i1, mut0, mut1 = numpy_matches(s)
    gt0 = np.random.RandomState(100 + seed).randint(-1, n, size=(1, m)).astype(np.int64)
    res = host(eng.assignment_matches(cuda(s[None]), threshold=0.0, gt0=cuda(gt0, torch.int64)))
    assert res["matches0"].dtype == np.int64 and res["matches1"].dtype == np.int64 and res["stats"].dtype == np.int32
    assert np.array_equal(res["matches0"][0], np.where(mut0, i0, -1)) and np.array_equal(res["matches1"][0], np.where(mut1, i1, -1))
    z = s.astype(np.float64) + np.log(float(m + n))
    want0, want1 = np.where(mut0, np.exp(z.max(1)), 0.0), np.where(mut1, np.exp(z.max(0)), 0.0)
    assert np.array_equal(res["matching_scores0"][0] > 0, mut0) and np.array_equal(res["matching_scores1"][0] > 0, mut1)
    assert np.allclose(res["matching_scores0"][0], want0, rtol=3e-5, atol=0) and np.allclose(res["matching_scores1"][0], want1, rtol=3e-5, atol=0)
    # ms1 is GATHERED from ms0: the same bits
    assert np.array_equal(res["matching_scores1"][0][mut1].view(np.int32), res["matching_scores0"][0][i1[mut1]].view(np.int32))
    m0 = res["matches0"][0]
    assert res["stats"][0].tolist() == [int((gt0[0] >= 0).sum()), int((m0 > -1).sum()), int(((m0 == gt0[0]) & (gt0[0] >= 0)).sum())]
    if m > 2 and n > 2:                                                  # the later copies of a duplicated row / column never win
        assert not np.isin(i1, (m // 2, m - 1)).any() and not np.isin(i0, (n // 2, n - 1)).any(), "the planting"
        assert not np.isin(res["matches1"][0], (m // 2, m - 1)).any() and not np.isin(res["matches0"][0], (n // 2, n - 1)).any()
    none = host(eng.assignment_matches(cuda(s[None]), threshold=float(np.finfo(np.float32).max)))
    assert set(none) == set(KEYS) and (none["matches0"] == -1).all() and (none["matches1"] == -1).all()
    assert same_bits(none, res, ("matching_scores0", "matching_scores1")), "the threshold does not touch the scores"


def test_argument_checks(eng):
    from image_matching_amd.engine import ImxError
    s = cuda(integer_scores(1, 5, 6)[None])
    for kwargs in ({"u": torch.zeros(1, 5, device="cuda")}, {"v": torch.zeros(1, 6, device="cuda")}, {"threshold": float("nan")},
                   {"gt0": torch.zeros(1, 6, dtype=torch.int64)}, {"n0": torch.zeros(2, dtype=torch.int32)}):
        with pytest.raises(ImxError):
            eng.assignment_matches(s, **kwargs)
    with pytest.raises(ImxError):
        eng.assignment_matches(s[0])


# ---------------------------------------------------------------------------------------------- 2. with potentials
@pytest.mark.parametrize("seed,m,n,iters", SHAPES)
def test_with_float64_potentials(eng, seed, m, n, iters):
    """the float64 u_T, v_T of the case, cast to fp32 and handed in: the comparison rule"""
    ref = reference(seed, m, n, iters)
    res = host(eng.assignment_matches(cuda(ref["scores"][None]), u=cuda(ref["u"][None]), v=cuda(ref["v"][None]), threshold=THRESHOLD))
    left, total, worst = by_the_rule(cut(res, 0, m, n), ref, (seed, m, n))
    print(f"seed {seed} {m}x{n} T={iters}: {left} of {total} keypoints left out, {int((ref['matches0_64'] >= 0).sum())} matches; scores use {worst:.3g} of the bar; "
          f"the restatement's own fp32 agrees with its float64 on {int((ref['matches0_32'] == ref['matches0_64']).sum())} of {m} rows")
    assert worst <= 1.0


# ---------------------------------------------------------------------------------------------- 3. the fused call
def fused(eng, S, am, n_all, iters, n0=None, n1=None, bin_score=1.0, gt0=None, **kw):
    i32 = lambda a: None if a is None else cuda(a, torch.int32)
    args = (cuda(S), bin_score, cuda(am, torch.int64), i32(n_all), iters)
    return (host(eng.ot_match_loss_grad_matches(*args, n0=i32(n0), n1=i32(n1), threshold=THRESHOLD, gt0=None if gt0 is None else cuda(gt0, torch.int64), **kw)),
            host(eng.ot_match_loss_grad(*args, n0=i32(n0), n1=i32(n1), **kw)))


def item(g, k):
    return {key[:-len(f"_{k}")]: v for key, v in g.items() if key.endswith(f"_{k}")}


@pytest.mark.parametrize("name", list(OT_CASES))
def test_fused_call_on_the_reference_fixtures(eng, name):
    """loss, grad_scores, grad_bin and flag equal Engine.ot_match_loss_grad's bit for bit; the matches by the comparison rule"""
    g = util.golden(f"otgrad_{name}.npz")
    for k in range(int(g["n_items"])):
        it = item(g, k)
        s, mt, T, alpha = it["scores"], it["matches"], int(it["iters"]), float(it["bin"])
        both, plain = fused(eng, s[None], mt[None], np.array([mt.shape[1]], np.int32), T, bin_score=alpha)
        assert set(both) == set(plain) | set(KEYS) and same_bits(both, plain, plain), (name, k)
        _FIXTURE_SCORES[(name, k)] = s
        ref = reference(0, s.shape[0], s.shape[1], T, alpha, (name, k))
        left, total, worst = by_the_rule(cut(both, 0, *s.shape), ref, (name, k))
        print(f"{name}[{k}] {s.shape[0]}x{s.shape[1]} T={T}: {left} of {total} left out, {int((ref['matches0_64'] >= 0).sum())} matches, scores use {worst:.3g} of the bar")
        assert worst <= 1.0
        value, plain_value = fused(eng, s[None], mt[None], np.array([mt.shape[1]], np.int32), T, bin_score=alpha, want_grad=False)
        assert "grad_scores" not in value and same_bits(value, plain_value, plain_value) and same_bits(value, both, KEYS), "the value-only mode"


def ragged():
    """B = 3 in a 48 x 48 frame with NaN padding: counts (40,33), (23,48) and an empty pair (0,17)"""
    (F0, F1), B = RAGGED_FRAME, len(RAGGED_COUNTS)
    S = np.full((B, F0, F1), np.nan, np.float32)
    am = np.full((B, 2, F0 + F1), 1 << 40, np.int64)
    n_all = np.zeros(B, np.int32)
    for b, (m, n) in enumerate(RAGGED_COUNTS):
        if m and n:
            s, mt = O.case_scores(20 + b, m, n)
            S[b, :m, :n], am[b, :, :mt.shape[1]], n_all[b] = s, mt, mt.shape[1]
    n0, n1 = (np.array([c[i] for c in RAGGED_COUNTS], np.int32) for i in (0, 1))
    gt0 = np.full((B, F0), -1, np.int64)
    for b, (m, n) in enumerate(RAGGED_COUNTS):
        if m and n:
            inner = (am[b, 0, :n_all[b]] < m) & (am[b, 1, :n_all[b]] < n)
            gt0[b, am[b, 0, :n_all[b]][inner]] = am[b, 1, :n_all[b]][inner]
    return S, am, n_all, n0, n1, gt0


def test_fused_call_on_a_ragged_batch(eng):
    """the same bits as the plain call on a ragged batch; matches by the rule per pair; -1 / 0 past the counts; the empty pair all -1 with
    zero counts; stats against numpy"""
    S, am, n_all, n0, n1, gt0 = ragged()
    assert np.isnan(S).any()
    both, plain = fused(eng, S, am, n_all, RAGGED_ITERS, n0, n1, gt0=gt0)
    assert same_bits(both, plain, plain)
    for b, (m, n) in enumerate(RAGGED_COUNTS):
        assert (both["matches0"][b, m:] == -1).all() and (both["matches1"][b, n:] == -1).all()
        assert not both["matching_scores0"][b, m:].any() and not both["matching_scores1"][b, n:].any()
        m0 = both["matches0"][b]
        if not (m and n):
            assert (m0 == -1).all() and (both["matches1"][b] == -1).all() and not both["matching_scores0"][b].any() and not both["matching_scores1"][b].any()
            assert both["stats"][b].tolist() == [0, 0, 0] and both["loss"][b] == 0
            continue
        ref = reference(20 + b, m, n, RAGGED_ITERS)
        left, total, worst = by_the_rule(cut(both, b, m, n), ref, b)
        print(f"ragged pair {b} {m}x{n}: {left} of {total} left out, {int((m0 >= 0).sum())} matches, scores use {worst:.3g} of the bar, stats {both['stats'][b].tolist()}")
        assert worst <= 1.0
        assert both["stats"][b].tolist() == [int((gt0[b, :m] >= 0).sum()), int((m0[:m] > -1).sum()), int(((m0[:m] == gt0[b, :m]) & (gt0[b, :m] >= 0)).sum())]
        assert np.isfinite(both["matching_scores0"][b]).all() and np.isfinite(both["matching_scores1"][b]).all(), "NaN padding leaked"


# ---------------------------------------------------------------------------------------------- 4. invariance
def test_equal_bits_alone_in_a_batch_in_another_frame_on_poisoned_and_second_handles(eng):
    S, am, n_all, n0, n1, gt0 = ragged()
    first, _ = fused(eng, S, am, n_all, RAGGED_ITERS, n0, n1, gt0=gt0)
    again, _ = fused(eng, S, am, n_all, RAGGED_ITERS, n0, n1, gt0=gt0)
    assert same_bits(first, again), "a repeated call"
    out_keys = KEYS + ("stats", "loss", "grad_bin")
    for b, (m, n) in enumerate(RAGGED_COUNTS):
        one, _ = fused(eng, S[b:b + 1], am[b:b + 1], n_all[b:b + 1], RAGGED_ITERS, n0[b:b + 1], n1[b:b + 1], gt0=gt0[b:b + 1])
        assert all(np.array_equal(bits(one[k][0]), bits(first[k][b])) for k in out_keys + ("grad_scores",)), f"pair {b} alone"
        if m and n:                                                      # its own frame (m, n) and a larger one (70, 50), padding of another kind
            own, _ = fused(eng, S[b:b + 1, :m, :n], am[b:b + 1], n_all[b:b + 1], RAGGED_ITERS, gt0=gt0[b:b + 1, :m])
            big = np.full((1, 70, 50), 1e30, np.float32)
            big[0, :m, :n] = S[b, :m, :n]
            gt_big = np.full((1, 70), 5, np.int64)
            gt_big[0, :m] = gt0[b, :m]
            wide, _ = fused(eng, big, am[b:b + 1], n_all[b:b + 1], RAGGED_ITERS, n0[b:b + 1], n1[b:b + 1], gt0=gt_big)
            for other in (own, wide):
                assert all(np.array_equal(bits(other[k][0]), bits(first[k][b])) for k in ("stats", "loss", "grad_bin")), f"pair {b}, another frame"
                assert all(np.array_equal(bits(v), bits(cut(first, b, m, n)[k])) for k, v in cut(other, 0, m, n).items()), f"pair {b}, another frame"
            assert (wide["matches0"][0, m:] == -1).all() and (wide["matches1"][0, n:] == -1).all()
    # the extraction alone from the SAME potentials gives the fused call's matches: iters = 0 means zero potentials
    zero, _ = fused(eng, S, am, n_all, 0, n0, n1, gt0=gt0)
    alone = host(eng.assignment_matches(cuda(S), threshold=THRESHOLD, n0=cuda(n0, torch.int32), n1=cuda(n1, torch.int32), gt0=cuda(gt0, torch.int64)))
    assert same_bits(alone, zero, alone), "iters = 0 equals the extraction with NULL potentials"
    for pattern in ("nan", "huge"):
        other = new_engine()                                             # a fresh handle: every workspace it allocates is poisoned
        other.set_option("debug_poison", pattern)
        try:
            got, _ = fused(other, S, am, n_all, RAGGED_ITERS, n0, n1, gt0=gt0)
            assert same_bits(first, got), f"a second handle, workspaces poisoned with {pattern}"
            big_s, big_mt = O.case_scores(63, 130, 70)
            fused(other, big_s[None], big_mt[None], np.array([big_mt.shape[1]], np.int32), RAGGED_ITERS + 3)      # (grown, poisoned again)
            got, _ = fused(other, S, am, n_all, RAGGED_ITERS, n0, n1, gt0=gt0)
            assert same_bits(first, got), f"after a larger call, {pattern}"
            assert same_bits(alone, host(other.assignment_matches(cuda(S), threshold=THRESHOLD, n0=cuda(n0, torch.int32), n1=cuda(n1, torch.int32),
                                                                  gt0=cuda(gt0, torch.int64))))
        finally:
            other.set_option("debug_poison", "off")


# ---------------------------------------------------------------------------------------------- 5. the model on sgmodel_step.npz
@pytest.fixture(scope="module")
def golden():
    return util.golden("sgmodel_step.npz")


def trainable(eng, seed):
    from image_matching_amd.sgtrain_model import SuperGlueTrainable
    return R.load_parameters(SuperGlueTrainable(R.MODEL_CONFIG, eng).train(), seed)


def sample(seed):
    return {k: torch.from_numpy(v).cuda() for k, v in R.model_case(seed).items()}


def step(eng, seed, want_matches):
    model = trainable(eng, seed)
    out = model(sample(seed), want_matches=want_matches)
    out["loss"].backward()
    return out, {n: p.grad.cpu().numpy() for n, p in model.named_parameters()}, model


def test_model_matches_from_the_loss(eng, golden):
    """forward(sample, want_matches="loss"): the reference's keys, none requiring grad; matches equal the reference's outside MARGIN,
    scores at the bar; the loss and all 42 gradients (41 parameters and the loss) have the bits of want_matches=False; want_matches=True
    still gives what the PyTorch restatement gives"""
    from image_matching_amd import sgtrain_model
    g, seed = golden, int(golden["seed"])
    plain, grads_plain, _ = step(eng, seed, False)
    out, grads, model = step(eng, seed, "loss")
    assert set(out) == {"loss", "skip_train"} | set(KEYS) and out["skip_train"] is False
    assert out["loss"].requires_grad and not any(out[k].requires_grad for k in KEYS)
    assert out["matches0"].dtype == torch.int64 and tuple(out["matches0"].shape) == (R.MODEL_SAMPLE["N0"],) and tuple(out["matches1"].shape) == (R.MODEL_SAMPLE["N1"],)
    assert len(grads) == 41 and set(grads) == set(grads_plain)
    assert out["loss"].detach().cpu().numpy().view(np.int32) == plain["loss"].detach().cpu().numpy().view(np.int32)
    for n in grads:
        assert np.array_equal(grads[n].view(np.int32), grads_plain[n].view(np.int32)), n
    keep0, keep1 = g["margin0"] >= MARGIN, g["margin1"] >= MARGIN
    left_out = int((~keep0).sum() + (~keep1).sum())
    assert left_out <= MARGIN_CAP * (len(keep0) + len(keep1))
    worst = 0.0
    for side, keep in (("0", keep0), ("1", keep1)):
        got = out[f"matches{side}"].cpu().numpy()
        assert got.shape == g[f"matches{side}"].shape and np.array_equal(got[keep], g[f"matches{side}"][keep]), side
        ms, ref = out[f"matching_scores{side}"].cpu().numpy().astype(np.float64), g[f"mscores{side}_g"]
        worst = max(worst, float(np.max(np.abs(ms[keep] - ref[keep]) / R.bar(ref[keep], g[f"mscores{side}_d32"][keep]))))
    print(f"model, want_matches='loss': {left_out} of {len(keep0) + len(keep1)} keypoints left out, {int((g['matches0'] >= 0).sum())} matches; scores use {worst:.3g} of the bar")
    assert worst <= 1.0
    # want_matches=True: the second Sinkhorn in PyTorch, as before -- what transport() and mutual_matches() give on the scores
    old, grads_old, _ = step(eng, seed, True)
    assert set(old) == set(out) and all(np.array_equal(grads_old[n].view(np.int32), grads_plain[n].view(np.int32)) for n in grads)
    k0, k1 = keep0, keep1
    assert np.array_equal(old["matches0"].cpu().numpy()[k0], g["matches0"][k0]) and np.array_equal(old["matches1"].cpu().numpy()[k1], g["matches1"][k1])
    assert sgtrain_model.transport is not None and old["matching_scores0"].dtype == torch.float32
    with pytest.raises(Exception):
        model(sample(seed), want_matches="both")


def test_forward_pairs_matches_with_stats(eng, golden):
    """forward_pairs_matches on the fixture's pair twice in one batch with gt0: both rows equal, stats consistent with the matches"""
    seed = int(golden["seed"])
    model, p = trainable(eng, seed), R.as_pair(R.model_case(seed), torch.float32)
    two = lambda t: torch.cat([t, t], 0).cuda().contiguous()
    am = torch.stack([p["all_matches"]] * 2).cuda()
    N0, N1 = R.MODEL_SAMPLE["N0"], R.MODEL_SAMPLE["N1"]
    gt0 = torch.full((2, N0), -1, dtype=torch.int64)
    xs, ys = p["all_matches"]
    inner = (xs < N0) & (ys < N1)
    gt0[:, xs[inner]] = ys[inner]
    n_all = torch.full((2,), am.shape[2], dtype=torch.int32).cuda()
    args = (two(p["kpts0"]), two(p["scores0"]), two(p["desc0"]), two(p["kpts1"]), two(p["scores1"]), two(p["desc1"]), am, n_all, p["shape0"], p["shape1"])
    loss, found = model.forward_pairs_matches(*args, gt0=gt0.cuda())
    assert tuple(loss.shape) == (2,) and set(found) == set(KEYS) | {"stats"} and not any(v.requires_grad for v in found.values())
    m0, st = found["matches0"].cpu().numpy(), found["stats"].cpu().numpy()
    assert np.array_equal(m0[0], m0[1]) and loss[0].item() == loss[1].item()
    g = gt0.numpy()
    assert st[0].tolist() == st[1].tolist() == [int((g[0] >= 0).sum()), int((m0[0] > -1).sum()), int(((m0[0] == g[0]) & (g[0] >= 0)).sum())]
    print(f"stats [ground truth, predicted, correct] = {st[0].tolist()}")
    loss2, found2 = model.forward_pairs_matches(*args)
    assert set(found2) == set(KEYS)


# ---------------------------------------------------------------------------------------------- 6. the trainer
@pytest.mark.parametrize("kind", ["flat", "torch"])
def test_four_train_steps_on_the_fixture(eng, golden, kind):
    """4 consecutive train_step()s on the fixture's sample at its adam_lr: each loss within 1e-4 + 1e-4 |ref| of the reference's float64
    sequence (the bar of tests/test_gpu_sgmodel.py), with FlatAdam and with torch.optim.Adam"""
    from image_matching_amd.superglue.train_loop import SuperGlueTrainer
    g, seed = golden, int(golden["seed"])
    assert ADAM_STEPS == 4 and ADAM_LR == float(g["adam_lr"])
    t = SuperGlueTrainer(R.MODEL_CONFIG, None, eng, optimizer=kind, lr=ADAM_LR, keep_losses=True)
    R.load_parameters(t.net, seed)
    data = sample(seed)
    for _ in range(ADAM_STEPS):
        t.train_step(dict(data))
    losses, ref = [v.item() for v in t.step_losses], g["adam_losses"]
    used = np.abs(np.array(losses) - ref) / (1e-4 + 1e-4 * np.abs(ref))
    print(f"{kind}: losses {losses}, the reference's {ref.tolist()}; of 1e-4 + 1e-4 |ref|: {used.round(4).tolist()}")
    assert t.steps == 4 and used.max() <= 1.0 and np.all(np.diff(losses) < 0)


LOOP_CONFIG = {"descriptor_dim": D, "keypoint_encoder": [32, 64], "GNN_layers": ["self", "cross"], "sinkhorn_iterations": 20, "match_threshold": 0.2}


def loop_trainer(result_dir, **kw):
    """a trainer over 4 synthetic 120 x 160 images at 64 keypoints, batch 2, its own dataset"""
    from image_matching_amd.superglue.train_loop import SuperGlueTrainer
    from superglue_export_pairs import SyntheticPairs
    ds = SyntheticPairs(4, {"weights": None, "descriptor_dim": D, "nms_radius": 4, "keypoint_threshold": 0.005, "max_keypoints": 64}, [160, 120],
                        torch.device("cuda:0"))
    ds.seed = 2
    torch.manual_seed(0)                                                 # (the parameters' initial values)
    return SuperGlueTrainer(LOOP_CONFIG, ds, ds._engine(), optimizer="flat", lr=1e-3, batch_size=2, shuffle=True, seed=3, result_dir=str(result_dir),
                            log_interval=2, keep_losses=True, **kw)


def same_checkpoint(a, b):
    assert list(a) == list(b) == ["epoch", "net", "optimizer", "rng"] and a["epoch"] == b["epoch"]
    assert list(a["net"]) == list(b["net"]) and all(torch.equal(a["net"][k], b["net"][k]) for k in a["net"])
    assert torch.equal(a["rng"], b["rng"]) and sorted(a["optimizer"]["state"]) == sorted(b["optimizer"]["state"])
    for i, s in a["optimizer"]["state"].items():
        assert all(torch.equal(torch.as_tensor(s[k]), torch.as_tensor(b["optimizer"]["state"][i][k])) for k in ("step", "exp_avg", "exp_avg_sq")), i


def test_train_two_epochs_checkpoints_and_resume(tmp_path):
    """train(2) on 4 synthetic images: two checkpoints in the reference's layout whose 'net' loads into the inference SuperGlue; the logged
    mean loss is the mean of the per-step losses and the epoch loss their sum over the number of batches; a match picture is written; a
    run resumed from the epoch-1 checkpoint writes the epoch-2 checkpoint of the uninterrupted run, bit for bit"""
    from image_matching_amd.superglue.models.superglue_test import SuperGlue
    a = loop_trainer(tmp_path / "a")
    assert a.train(2) == 2 and a.steps == 4
    files = sorted((tmp_path / "a" / "checkpoints").iterdir())
    assert [f.name for f in files] == ["SuperGlue_epoch_1.pth", "SuperGlue_epoch_2.pth"]
    ckpts = [torch.load(str(f), map_location="cpu") for f in files]
    for e, c in enumerate(ckpts, 1):
        assert list(c) == ["epoch", "net", "optimizer", "rng"] and c["epoch"] == e
        SuperGlue({**LOOP_CONFIG, "weights": ""}).load_state_dict(c["net"])
    assert not all(torch.equal(ckpts[0]["net"][k], ckpts[1]["net"][k]) for k in ckpts[0]["net"]), "the second epoch moved the parameters"
    losses = [v.item() for v in a.step_losses]
    logged = {(tag, step): v for tag, step, v in a.history}
    print(f"step losses {losses}; logged {a.history}")
    assert np.isfinite(losses).all()
    for epoch in (1, 2):
        want = np.mean(losses[2 * epoch - 2:2 * epoch])
        assert abs(logged[("Mean_Loss", 2 * epoch)] - want) <= 1e-6 * abs(want), "fp32 on the device against float64 here"
        assert abs(logged[("epoch_loss", epoch)] - want) <= 1e-6 * abs(want)
        assert 0.0 <= logged[("precision", 2 * epoch)] <= 1.0 and 0.0 <= logged[("recall", 2 * epoch)] <= 1.0
    assert (tmp_path / "a" / "match" / "1_matches.png").exists()
    b = loop_trainer(tmp_path / "b")
    assert b.resume(files[0]) == 1
    assert b.train(2) == 2 and b.steps == 2
    same_checkpoint(torch.load(str(tmp_path / "b" / "checkpoints" / "SuperGlue_epoch_2.pth"), map_location="cpu"), ckpts[1])
    assert [v.item() for v in b.step_losses] == losses[2:]


def test_the_script_on_synthetic_images(tmp_path):
    """python superpoint_glue_train.py --synthetic 2 --iters 2 as a child process: exit code 0 and a checkpoint in the reference's layout"""
    out = tmp_path / "run"
    cmd = [sys.executable, os.path.join(ROOT, "superpoint_glue_train.py"), "--synthetic", "2", "--iters", "2", "--epoch", "3", "--Result_dir", str(out),
           "--resize", "160", "120", "--max_keypoints", "64", "--keypoint_encoder", "32", "64", "--sinkhorn_iterations", "20"]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    print(res.stdout[-1500:], res.stderr[-1500:])
    assert res.returncode == 0
    ckpt = torch.load(str(out / "checkpoints" / "SuperGlue_epoch_1.pth"), map_location="cpu")
    assert list(ckpt)[:2] == ["epoch", "net"] and ckpt["epoch"] == 1
    assert (out / "logdir").is_dir()
