"""Gradients of the two SuperPoint training losses on the GPU (imx_detector_loss_grad, imx_desc_loss_sparse_grad,
Engine.sp_train_loss_grads, image_matching_amd.sptrain_grad) against the project's restatement in float64 (tests/spgrad_ref.py, itself
held to the reference's autograd by tests/test_spgrad_host.py) and against the samples and per-cell norms the reference's own autograd
wrote (tests/golden/make_golden_spgrad.py).  The default bar, element-wise: |g - g64| <= max(1e-4 + 1e-4 |g64|, 2.5 |ref32 - g64|);
where the reference's fp32 gradient is not at hand (full maps) the first term alone.  Needs an MI355X; a few seconds per test."""
import copy

import numpy as np
import pytest
import torch

from tests import spgrad_ref as G
from tests import sptrain_ref as R
from tests import util
from tests.golden.make_golden_spgrad import DET_CASES, METHODS, desc_key, det_key, sample_positions
from tests.golden.make_golden_sptrain import DIMS, LAMDA_D, MARGIN, SETTINGS, desc_maps

pytestmark = pytest.mark.gpu
NAMES = ("120x160_s1", "120x160_s2", "136x200_s2", "136x200_s3")
D = 128


@pytest.fixture(scope="module")
def fx():
    return {n: (util.golden(f"sptrain_{n}.npz"), util.golden(f"spgrad_{n}.npz")) for n in NAMES}


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


def frac(got, g64, d32=None):
    """the worst fraction of the default bar used"""
    got, g64 = np.asarray(got, np.float64), np.asarray(g64, np.float64)
    return float(np.max(np.abs(got - g64) / G.bar(g64, d32)))


def same_bits(a, b):
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(a, b))


def desc_case(src, d, si):
    H, W = (int(v) for v in src["size"])
    da, db = desc_maps(int(src["seed"]), d, H // 8, W // 8)
    return da, db, src[f"choice_{si}"].astype(np.int32), src[f"nonmatch_{si}"].astype(np.int32)


def det_inputs(src, sl):
    labels = np.stack([src["labels"], src["warped_labels"]]).astype(np.float32)
    mask = np.stack([np.ones_like(src["warped_valid_mask"]), src["warped_valid_mask"]]).astype(np.float32)
    return src["semi"][sl], labels[sl], mask[sl]


def against_samples(g, seed, key, name, norm_name, got):
    """a full gradient map against the reference's samples (default bar, with the reference's own fp32 error) and per-cell norms"""
    pos = sample_positions(seed, key, got.size)
    f = frac(got.reshape(-1)[pos], g[name], g[name + "_d32"])
    norms = G.cell_l1(got)
    # a per-cell L1 norm sums |g| over the channels: each of them within its bar.  For the detector gradient (65 channels, elements of a
    # few 1e-3 at these sizes) this bar is wider than the norms themselves: there the norms only show a cell that went missing or wild, and
    # the formulas are held by the logit-gap case and by the 1e-5 bar of tests/test_spgrad_host.py
    nbar = 1e-4 * got.shape[-3] + 1e-4 * g[norm_name].astype(np.float64)
    return max(f, float(np.max(np.abs(norms - g[norm_name]) / nbar)))


# ---------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("name", NAMES)
def test_detector_grad_on_the_fixtures(eng, fx, name):
    src, g = fx[name]
    worst = [0.0, 0.0]
    for case, sl in zip(DET_CASES, (slice(0, 1), slice(1, 2), slice(0, 2))):
        semi, labels, mask = det_inputs(src, sl)
        out, grad = eng.detector_loss_grad(cuda(semi), cuda(labels), cuda(mask))
        assert same_bits([out], [eng.detector_loss(cuda(semi), cuda(labels), cuda(mask))]), "the value is imx_detector_loss's, bit for bit"
        g64 = G.detector_grad(semi, labels, mask)[1]
        got = grad.cpu().numpy()
        worst[0] = max(worst[0], frac(got, g64))
        worst[1] = max(worst[1], against_samples(g, int(g["seed"]), det_key(case), f"gdet_{case}", f"ndet_{case}", got))
    print(f"{name}: detector gradient at most {worst[0]:.3g} of the bar from the float64 restatement, {worst[1]:.3g} from the reference's samples and norms")
    assert worst[0] <= 1.0 and worst[1] <= 1.0


@pytest.mark.parametrize("name", NAMES)
def test_desc_grad_on_the_fixtures(eng, fx, name):
    src, g = fx[name]
    seed = int(g["seed"])
    hom = torch.from_numpy(src["homography"][None])
    worst = [0.0, 0.0]
    for si in range(len(SETTINGS)):
        for d in DIMS:
            da, db, choice, non = desc_case(src, d, si)
            for method in METHODS:
                args = (cuda(da[None]), cuda(db[None]), hom, cuda(choice[None], torch.int32), cuda(non[None], torch.int32), LAMDA_D, MARGIN, method)
                out = eng.desc_loss_sparse_grad(*args, want_pairs=True)
                fwd = eng.desc_loss_sparse(*args, want_pairs=True)
                tag = f"{name} setting {si} d={d} {method}"
                assert same_bits([out[k] for k in ("out", "mean", "pairs", "flag")], [fwd[k] for k in ("out", "mean", "pairs", "flag")]), tag
                assert int(out["flag"]) == 0
                _, ga, gb = G.desc_grad(da, db, src["pair_a"], src["pair_b"], choice, non.astype(np.int64), LAMDA_D, MARGIN, method)
                for side, (s, ref) in enumerate(zip("ab", (ga, gb))):
                    got = out["grad_" + s][0].cpu().numpy()
                    f0 = frac(got, ref)
                    f1 = against_samples(g, seed, desc_key(si, d, method, side), f"g{s}_{si}_{d}_{method}", f"n{s}_{si}_{d}_{method}", got)
                    assert f0 <= 1.0 and f1 <= 1.0, f"{tag} side {s}: {f0} / {f1} of the bar"
                    worst = [max(worst[0], f0), max(worst[1], f1)]
    print(f"{name}: descriptor gradient at most {worst[0]:.3g} of the bar from the float64 restatement, {worst[1]:.3g} from the reference's samples and "
          f"norms, 24 combinations")


def test_collisions(eng, fx):
    """the (512, 8) setting: choice repeats cells and 4 096 non-match rows land on at most 425 cells -- asserted, so that the parity
    of this setting cannot pass on a collision-free case -- and the gradient at the most crowded cells meets the restatement"""
    for name in NAMES:
        src, _ = fx[name]
        assert SETTINGS[2] == (512, 8)
        ia = src["pair_a"][src["choice_2"]]
        cnt_a, cnt_b = np.bincount(ia), np.bincount(src["nonmatch_2"].astype(np.int64).reshape(-1))
        assert cnt_a.max() >= 2 and cnt_b.max() >= 8, (name, cnt_a.max(), cnt_b.max())
        da, db, choice, non = desc_case(src, 64, 2)
        for method in METHODS:
            out = eng.desc_loss_sparse_grad(cuda(da[None]), cuda(db[None]), torch.from_numpy(src["homography"][None]), cuda(choice[None], torch.int32),
                                            cuda(non[None], torch.int32), LAMDA_D, MARGIN, method)
            _, ga, gb = G.desc_grad(da, db, src["pair_a"], src["pair_b"], choice, non.astype(np.int64), LAMDA_D, MARGIN, method)
            a_cell, b_cell = int(cnt_a.argmax()), int(cnt_b.argmax())
            got_a = out["grad_a"][0].reshape(64, -1)[:, a_cell].cpu().numpy()
            got_b = out["grad_b"][0].reshape(64, -1)[:, b_cell].cpu().numpy()
            assert np.abs(ga.reshape(64, -1)[:, a_cell]).sum() > 0 and np.abs(gb.reshape(64, -1)[:, b_cell]).sum() > 0
            assert frac(got_a, ga.reshape(64, -1)[:, a_cell]) <= 1.0 and frac(got_b, gb.reshape(64, -1)[:, b_cell]) <= 1.0


# ---------------------------------------------------------------------------------------------- determinism
def grad_calls(fx):
    calls = {}
    for tag, names, d, si in (("small", NAMES[:2], 128, 2), ("odd", NAMES[2:], 256, 0)):
        srcs = [fx[n][0] for n in names]
        hom = torch.from_numpy(np.stack([s["homography"] for s in srcs]))
        masks = cuda(np.stack([s["warped_valid_mask"] for s in srcs]).astype(np.float32))
        semi = cuda(np.concatenate([s["semi"][1:] for s in srcs]))
        labels = cuda(np.stack([s["warped_labels"] for s in srcs]).astype(np.float32))
        cases = [desc_case(s, d, si) for s in srcs]
        da, db, ch, nm = (cuda(np.stack([c[k] for c in cases]), torch.int32 if k > 1 else torch.float32) for k in range(4))
        calls[f"detector_{tag}"] = lambda e, semi=semi, labels=labels, masks=masks: e.detector_loss_grad(semi, labels, masks)
        for method in METHODS:
            calls[f"desc_{tag}_{method}"] = lambda e, da=da, db=db, hom=hom, ch=ch, nm=nm, method=method: tuple(
                e.desc_loss_sparse_grad(da, db, hom, ch, nm, LAMDA_D, MARGIN, method)[k] for k in ("out", "mean", "grad_a", "grad_b"))
    return calls


def test_gradients_do_not_depend_on_history(eng, fx):
    calls = grad_calls(fx)
    want = {k: tuple(t.clone() for t in f(eng)) for k, f in calls.items()}
    for k, f in calls.items():
        assert same_bits(f(eng), want[k]), f"{k}: twice"
    for order in (sorted(calls), sorted(calls, reverse=True)):
        for k in order:
            assert same_bits(calls[k](eng), want[k]), f"{k}: after a call of another size"
    for poison in ("nan", "huge", "zero"):
        eng.set_option("debug_poison", poison)
        for k, f in calls.items():
            assert same_bits(f(eng), want[k]), f"{k}: after debug_poison = {poison}"
    eng.set_option("debug_poison", "off")
    fresh = new_engine()
    fresh.set_option("debug_poison", "nan")
    for k in sorted(calls, reverse=True):
        assert same_bits(calls[k](fresh), want[k]), f"{k}: on a second handle"


# ---------------------------------------------------------------------------------------------- batch assembly
def test_batch_assembly(eng, fx):
    sa, sb = fx[NAMES[0]][0], fx[NAMES[1]][0]
    for si, d, method in ((2, 64, "2d"), (0, 128, "1d")):
        cases = [desc_case(sa, d, si), desc_case(sb, d, si), desc_case(sa, d, si)]
        homs = np.stack([sa["homography"], sb["homography"], sa["homography"]])
        stack = lambda idx, k: cuda(np.stack([cases[i][k] for i in idx]), torch.int32 if k > 1 else torch.float32)
        run = lambda idx: eng.desc_loss_sparse_grad(stack(idx, 0), stack(idx, 1), torch.from_numpy(homs[list(idx)]), stack(idx, 2), stack(idx, 3),
                                                    LAMDA_D, MARGIN, method)
        two, singles = run((0, 1)), [run((0,)), run((1,))]
        for b in (0, 1):                                                 # the factor 1 / B is a power of two: exact
            for s in ("grad_a", "grad_b"):
                assert same_bits([two[s][b]], [0.5 * singles[b][s][0]]), f"B = 2, image {b}, {s}"
        three = run((0, 1, 2))
        for b, src in enumerate((sa, sb, sa)):
            da, db, ch, nm = cases[b]
            _, ga, gb = G.desc_grad(da, db, src["pair_a"], src["pair_b"], ch, nm.astype(np.int64), LAMDA_D, MARGIN, method, gout=1 / 3)
            assert frac(three["grad_a"][b].cpu().numpy(), ga) <= 1.0 and frac(three["grad_b"][b].cpu().numpy(), gb) <= 1.0
        assert same_bits([three["grad_a"][0], three["grad_b"][0]], [three["grad_a"][2], three["grad_b"][2]])


# ---------------------------------------------------------------------------------------------- edges, against the restatement
def unit_maps(rng, B, d, Hc, Wc):
    x = rng.standard_normal((B, d, Hc, Wc))
    return (x / np.sqrt((x * x).sum(1, keepdims=True))).astype(np.float32)


def run_cells(eng, da, db, mats, ch, nm, method, lamda_d=LAMDA_D, gout=None):
    return eng.desc_loss_sparse_grad(cuda(da), cuda(db), cuda(mats), cuda(ch, torch.int32), cuda(nm, torch.int32), lamda_d, MARGIN, method, gout=gout,
                                     cell_space=True)


@pytest.mark.parametrize("d,Hc,Wc,M,Rn", ((4, 2, 3, 5, 3), (20, 2, 3, 1, 4), (512, 2, 3, 7, 1), (8, 1, 1, 3, 2), (20, 9, 13, 40, 6)))
def test_desc_grad_edges(eng, d, Hc, Wc, M, Rn):
    """d in {4, 20, 512}; maps of 1 x 1 and 2 x 3 cells under the identity (size - 1 = 0 in the 2d taps of the first); R = 1; M = 1"""
    rng = np.random.default_rng([d, Hc, Wc, M, Rn])
    N = Hc * Wc
    eye = np.eye(3, dtype=np.float32)
    da, db = unit_maps(rng, 1, d, Hc, Wc), unit_maps(rng, 1, d, Hc, Wc)
    db[0] = (0.6 * da[0] + 0.8 * db[0]).astype(np.float32)             # correlated maps: hinges of both signs
    ch = rng.integers(0, N, (1, M)).astype(np.int32)
    nm = rng.integers(0, N, (1, M, Rn)).astype(np.int32)
    pa, pb = R.desc_pairs(eye, Hc, Wc)
    assert len(pa) == N
    for method in METHODS:
        out = run_cells(eng, da, db, eye[None], ch, nm, method)
        loss, ga, gb = G.desc_grad(da[0], db[0], pa, pb, ch[0], nm[0].astype(np.int64), LAMDA_D, MARGIN, method)
        assert int(out["flag"]) == 0 and abs(float(out["mean"][0]) - loss) <= 1e-4 + 1e-4 * abs(loss)
        fa, fb = frac(out["grad_a"][0].cpu().numpy(), ga), frac(out["grad_b"][0].cpu().numpy(), gb)
        print(f"d={d} {Hc}x{Wc} M={M} R={Rn} {method}: {fa:.3g} / {fb:.3g} of the bar")
        assert fa <= 1.0 and fb <= 1.0 and (np.abs(ga).sum() > 0 or loss == 0)


def test_desc_grad_flags_and_gout(eng):
    Hc, Wc, d, M, Rn = 9, 13, 64, 100, 8
    N = Hc * Wc
    rng = np.random.default_rng(12)
    eye = np.eye(3, dtype=np.float32)
    away = eye.copy()
    away[0, 2] = 1000.0
    da, db = unit_maps(rng, 2, d, Hc, Wc), unit_maps(rng, 2, d, Hc, Wc)
    ch = rng.integers(0, N, (2, M)).astype(np.int32)
    nm = rng.integers(0, N, (2, M, Rn)).astype(np.int32)
    pa, pb = R.desc_pairs(eye, Hc, Wc)
    # an image without a valid pair beside a valid one: zeros, bit 2 of the flag, NaN values, the neighbour as if alone (times 1 / B)
    out = run_cells(eng, da, db, np.stack([eye, away]), ch, nm, "2d")
    alone = run_cells(eng, da[:1], db[:1], eye[None], ch[:1], nm[:1], "2d")
    assert int(out["flag"]) == 4 and np.isnan(out["out"][1, :3].cpu().numpy()).all() and float(out["out"][1, 4]) == 0
    assert not out["grad_a"][1].any() and not out["grad_b"][1].any()
    assert same_bits([out["grad_a"][0], out["grad_b"][0], out["out"][0]], [0.5 * alone["grad_a"][0], 0.5 * alone["grad_b"][0], alone["out"][0]])
    assert int(alone["flag"]) == 0
    # a flagged non-match index contributes nothing: the same bits as with a harmless (inactive) index in its place
    cold = int(np.argmin(da[0].reshape(d, -1)[:, pa[ch[0, 5]]] @ db[0].reshape(d, -1)))       # a b cell far below the margin for match 5
    good, bad = nm[:1].copy(), nm[:1].copy()
    good[0, 5, 2], bad[0, 5, 2] = cold, N
    assert float(da[0].reshape(d, -1)[:, pa[ch[0, 5]]] @ db[0].reshape(d, -1)[:, cold]) < MARGIN - 0.05
    o_good, o_bad = run_cells(eng, da[:1], db[:1], eye[None], ch[:1], good, "1d"), run_cells(eng, da[:1], db[:1], eye[None], ch[:1], bad, "1d")
    assert int(o_bad["flag"]) == 2 and int(o_good["flag"]) == 0
    assert same_bits([o_bad[k] for k in ("grad_a", "grad_b", "out")], [o_good[k] for k in ("grad_a", "grad_b", "out")])
    # a flagged choice index: the match and its non-match row drop out, M stays in the mean (restated with M - 1 matches, lamda_d (M - 1) / M)
    half = eye.copy()
    half[0, 2] = 1.5
    pa2, pb2 = R.desc_pairs(half, Hc, Wc)
    ch2 = (ch[:1] % len(pa2)).astype(np.int32)
    ch2[0, 3] = len(pa2)
    o = run_cells(eng, da[:1], db[:1], half[None], ch2, nm[:1], "2d")
    keep = np.arange(M) != 3
    _, ga, gb = G.desc_grad(da[0], db[0], pa2, pb2, ch2[0][keep], nm[0][keep].astype(np.int64), LAMDA_D * (M - 1) / M, MARGIN, "2d")
    assert int(o["flag"]) == 1 and frac(o["grad_a"][0].cpu().numpy(), ga) <= 1.0 and frac(o["grad_b"][0].cpu().numpy(), gb) <= 1.0
    # the upstream cotangent, given on the device
    gout = torch.tensor(0.37, device="cuda")
    o = run_cells(eng, da[:1], db[:1], eye[None], ch[:1], nm[:1], "2d", gout=gout)
    _, ga, gb = G.desc_grad(da[0], db[0], pa, pb, ch[0], nm[0].astype(np.int64), LAMDA_D, MARGIN, "2d", gout=float(np.float32(0.37)))
    assert frac(o["grad_a"][0].cpu().numpy(), ga) <= 1.0 and frac(o["grad_b"][0].cpu().numpy(), gb) <= 1.0
    assert same_bits([o["out"], o["mean"]], [alone["out"], alone["mean"]]), "gout does not touch the values"


def test_detector_grad_edges(eng, fx):
    src, _ = fx[NAMES[0]]
    semi, labels, mask = det_inputs(src, slice(0, 2))
    # gout on the device
    out, grad = eng.detector_loss_grad(cuda(semi), cuda(labels), cuda(mask), gout=torch.tensor(0.37, device="cuda"))
    g64 = G.detector_grad(semi, labels, mask, gout=float(np.float32(0.37)))[1]
    assert frac(grad.cpu().numpy(), g64) <= 1.0 and same_bits([out], [eng.detector_loss(cuda(semi), cuda(labels), cuda(mask))])
    # an all-zero mask: D = 1e-10, a finite zero gradient
    out, grad = eng.detector_loss_grad(cuda(semi), cuda(labels), cuda(np.zeros_like(mask)))
    assert float(out[0]) == 0.0 and float(out[1]) == 0.0 and not grad.any()
    # logit gaps 0, 40, 120, 200: finite, clamped terms give zero, the float64 restatement of the conditioned form
    x = np.full((1, 65, 1, 3), -200.0, np.float32)
    x[0, 0], x[0, 1], x[0, 2] = 0.0, -40.0, -120.0
    x[0, :, 0, 0] = 0.0
    lab = np.zeros((1, 8, 24), np.float32)
    lab[0, 0, 0] = lab[0, 0, 8 + 1] = lab[0, 0, 16 + 2] = 1
    ones = np.ones_like(lab)
    out, grad = eng.detector_loss_grad(cuda(x), cuda(lab), cuda(ones))
    g64 = G.detector_grad(x, lab, ones)[1]
    got = grad.cpu().numpy()
    print(f"logit gaps: {frac(got, g64):.3g} of the bar")
    assert np.isfinite(got).all() and frac(got, g64) <= 1.0 and abs(got[0, 2, 0, 2]) < 1e-30


# ---------------------------------------------------------------------------------------------- the autograd bridge
def test_autograd_bridge(eng, fx):
    """a two-layer convolution head emits semi and desc for a 120 x 160 pair; total_loss(...).backward() against the same head in
    float64 under tests/spgrad_ref.py's torch losses on the same device.  lamda_d = 1 (as test_sp_train_losses): the parameter
    gradients are sums over every cell, and with the fp32 head's own rounding they are held at 1e-4 + 1e-4 |ref|"""
    from image_matching_amd import sptrain_grad
    src, _ = fx[NAMES[0]]
    H, W = (int(v) for v in src["size"])
    Hc, Wc = H // 8, W // 8
    d, si, lambda_loss = 64, 0, 0.5
    torch.manual_seed(5)
    head = torch.nn.Sequential(torch.nn.Conv2d(1, 24, 8, stride=8), torch.nn.Tanh(), torch.nn.Conv2d(24, 65 + d, 1)).cuda()
    x = torch.cat(util.pair(int(src["seed"]), H, W)).cuda()              # (2,1,H,W): the image and its partner

    def emit(net, inp):
        y = net(inp)
        semi, desc = y[:, :65], y[:, 65:]
        desc = desc / desc.norm(dim=1, keepdim=True)
        return semi[:1].contiguous(), semi[1:].contiguous(), desc[:1].contiguous(), desc[1:].contiguous()
    semi_t, labels_t, mask_t = (cuda(v) for v in det_inputs(src, slice(0, 2)))
    sample = {"labels_2D": labels_t[:1], "valid_mask": mask_t[:1], "warped_labels": labels_t[1:], "warped_valid_mask": mask_t[1:],
              "homographies": torch.from_numpy(src["homography"][None]), "choice": cuda(src[f"choice_{si}"][None], torch.int32),
              "nonmatch_b": cuda(src[f"nonmatch_{si}"][None], torch.int32)}
    with torch.enable_grad():                                            # (whatever an imported module left as the global mode)
        semi, semi_w, desc, desc_w = emit(head, x)
        loss = sptrain_grad.total_loss(eng, semi, semi_w, desc, desc_w, sample, lambda_loss, lamda_d=1.0, margin=MARGIN, method="2d")
        assert loss.dim() == 0 and loss.is_cuda
        loss.backward()
        got = [p.grad.double().cpu().numpy() for p in head.parameters()]
        head64 = copy.deepcopy(head).double()
        head64.zero_grad()
        semi, semi_w, desc, desc_w = emit(head64, x.double())
        lab, msk = labels_t.cpu().numpy(), mask_t.cpu().numpy()
        ref = (G.detector_loss_t(semi, lab[:1], msk[:1]) + G.detector_loss_t(semi_w, lab[1:], msk[1:])
               + lambda_loss * G.desc_loss_t(desc[0], desc_w[0], src["pair_a"], src["pair_b"], src[f"choice_{si}"], src[f"nonmatch_{si}"].astype(np.int64),
                                             1.0, MARGIN, "2d"))
        ref.backward()
    want = [p.grad.cpu().numpy() for p in head64.parameters()]
    assert abs(float(loss) - float(ref)) <= 1e-4 + 1e-4 * abs(float(ref))
    worst = max(frac(a, b) for a, b in zip(got, want))
    print(f"autograd bridge: parameter gradients at most {worst:.3g} of 1e-4 + 1e-4 |ref|")
    assert worst <= 1.0 and all(np.abs(w).max() > 0 for w in want)
    with pytest.raises(Exception, match="contiguous fp32 cuda"):
        sptrain_grad.detector_loss.apply(eng, semi.detach(), labels_t[:1], mask_t[:1])       # float64: refused


def test_sp_train_loss_grads(eng, fx):
    names = NAMES[:2]
    srcs = [fx[n][0] for n in names]
    H, W = (int(v) for v in srcs[0]["size"])
    images = torch.cat([util.pair(int(s["seed"]), H, W)[0] for s in srcs]).cuda()
    hom = torch.from_numpy(np.stack([s["homography"] for s in srcs]))
    inv = torch.from_numpy(np.stack([s["inv_homography"] for s in srcs]))
    pts = cuda(np.stack([s["pts"] for s in srcs]))
    counts = torch.tensor([150, 90], dtype=torch.int32).cuda()
    ch = cuda(np.stack([s["choice_0"] for s in srcs]), torch.int32)
    nm = cuda(np.stack([s["nonmatch_0"] for s in srcs]), torch.int32)
    kw = dict(erosion_radius=3, lamda_d=1.0, method="2d", lambda_loss=0.5)
    out = eng.sp_train_loss_grads(images, pts, counts, hom, inv, ch, nm, **kw)
    fwd = eng.sp_train_losses(images, pts, counts, hom, inv, ch, nm, **kw)
    keys = ("loss", "loss_det", "loss_det_warp", "loss_desc", "positive_dist", "negative_dist", "semi", "semi_warp", "coarse_desc", "coarse_desc_warp")
    assert same_bits([out[k].contiguous() for k in keys], [fwd[k].contiguous() for k in keys]), "the losses sp_train_losses returns, bit for bit"
    assert same_bits([out["desc"]["out"]], [fwd["desc"]["out"]])
    # the staged calls
    _, g_semi = eng.detector_loss_grad(out["semi"], out["labels_2D"], out["valid_mask"])
    _, g_semi_w = eng.detector_loss_grad(out["semi_warp"], out["warped_labels"], out["warped_valid_mask"])
    dl = eng.desc_loss_sparse_grad(out["coarse_desc"], out["coarse_desc_warp"], hom, ch, nm, 1.0, MARGIN, "2d", gout=0.5)
    assert same_bits([out["grad_semi"], out["grad_semi_warp"], out["grad_desc"], out["grad_desc_warp"]], [g_semi, g_semi_w, dl["grad_a"], dl["grad_b"]])
    assert all(bool(torch.isfinite(out[k]).all()) and bool(out[k].any()) for k in ("grad_semi", "grad_semi_warp", "grad_desc", "grad_desc_warp"))
