"""SuperGlue on network shapes other than the shipped one: the tables (GNN layer lists, keypoint encoders, option sets) and the
helpers shared by tests/test_sg_shapes_host.py (CPU) and tests/test_gpu_sg_shapes.py (MI355X).  Importable without a GPU.

The library takes the network's shape from the configuration -- 0 to 64 GNN layers with a free 'self' / 'cross' flag each, a keypoint
encoder of 1 to 8 entries -- and plans a forward as a chain in which every launch leans on a neighbour through a layer-indexed table
(csrc/imx_superglue.cpp: the fused tail of layer l computes layer l + 1's q|k|v or final_proj, leaves its maxima in slot l + 1, reads
the other side's maxima exactly when layer l is 'cross').  The lists below put every one of those states next to a neighbour of the
other kind, first and last included."""
import functools

import numpy as np
import torch

from tests import util

S, C = "self", "cross"
SHIPPED = [S, C] * 9
LISTS = {
    "none": [], "s": [S], "c": [C], "sc": [S, C], "cs": [C, S], "ss": [S, S], "cc": [C, C], "sss": [S] * 3, "ccc": [C] * 3,
    "ssccs": [S, S, C, C, S], "cs9": [C, S] * 9, "s18": [S] * 18, "c18": [C] * 18, "sc17": SHIPPED[:17],
    "alt19": ([S, C] * 10)[:19], "alt64": [S, C] * 32,
    "sc18": SHIPPED,        # the shipped list: the forms' yardstick and a link of the prefix chains, not a case of its own
}
ALL = [k for k in LISTS if k != "sc18"]
FEW = ["none", "c", "ssccs", "c18"]
# the leading widths equal the calibrated ones (synth.apply_bn_stats asserts on another width); later BatchNorms keep mean 0 / var 1
ENCODERS = {"k1": [32], "k8": [32, 64, 128, 256, 128, 64, 32, 16]}
OPTION_SETS = {
    "A": (),                                                     # defaults: up to 4096 rows take the latency forms
    "B": (("latency_forms", "off"),),
    "C": (("latency_forms", "off"), ("gnn_tail", "bf16x3")),
    "D": (("latency_forms", "off"), ("mfma", "f32")),
    "E": (("latency_forms", "unfused"),),
}
# (d, list, encoder or None, option set) of the element-wise parity test, list-major so that the cached oracle result is reused
CASES = ([(128, l, None, o) for l in ALL for o in "AB"] + [(128, l, None, o) for l in FEW for o in "CDE"]
         + [(256, l, None, o) for l in FEW for o in "ABD"] + [(64, l, None, o) for l in FEW for o in "AB"]
         + [(128, "sc", e, o) for e in ENCODERS for o in "AB"])
CASES.sort(key=lambda c: (c[0], c[2] or "", list(LISTS).index(c[1])))
NETS = sorted({c[:3] for c in CASES}, key=lambda c: (c[0], c[2] or "", list(LISTS).index(c[1])))

# tests/golden/sg_layers.npz (make_golden.py --sg-layers): the reference's own forward on these nets, sg_small's inputs, d = 128
GOLDEN_NETS = (("none", None), ("c", None), ("ss", None), ("ssccs", None), ("c18", None), ("sc", "k8"))
GOLDEN_STRIDE_K, GOLDEN_STRIDE_C, GOLDEN_STRIDE_S = 16, 16, 8     # every 16th keypoint and 16th channel of a layer's output, every 8th row / column of scores_in and Z

# Two weight sets that make a table state observable which the "t" set's statistics hide (both are the "t" set with some projections of
# every layer scaled, and both are judged by the reference alone in test_sg_shapes_host.py):
#   "tv"  the v projection x 1/64: max |v| (about 0.15) lies far below max |x| (about 7), so a layer's x operand is scaled by the
#         max |x'| its predecessor left in the table, not by the v-maximum that otherwise bounds it too -- a slot that was not written
#         (or written elsewhere) overflows the fp16 planes;
#   "tq"  the q and k projections x 1/32: attention logits stay small on the lopsided pair below, whose |x| reaches 200.
VARIANT_GAINS = {"tv": ((".attn.proj.2.",), 1.0 / 64), "tq": ((".attn.proj.0.", ".attn.proj.1."), 1.0 / 32)}
TV_NETS = ((128, "ssccs"), (128, "cs9"))
# The lopsided pair: side 1's keypoint positions x 24 about the image centre (positions are data; the descriptors stay unit-norm).  Its
# keypoint encoder's output, which dominates x, and with it max |v| are about 24 times side 0's: whether a layer bounds att by its own
# side's v-maximum or by the other's -- the 'cross' flag -- changes the scale by four or five binades.  The magnitudes take the
# reference's own fp32 scores_in and Z outside the bar (6 and 1.2 to 6 of it), so kenc and every layer's output are held, not those.
LOPSIDED_SCALE, LOPSIDED_NETS = 24.0, ((128, "cs"), (128, "sc"), (256, "cs"), (256, "sc"))

H, W, K, SEED, SEED_Y = 120, 160, 256, 77, 70       # both sides of seed 77 (and of 70) keep 256 keypoints at d = 64, 128 and 256
COUNTS = ((256, 256), (200, 131), (256, 97))        # B = 3 pairs in one 256 frame: the 8 B l strides of the tables matter
KEYS = ("keypoints0", "keypoints1", "scores0", "scores1", "descriptors0", "descriptors1")
SHAPE = (1, 1, H, W)


def case_id(c):
    return f"d{c[0]}-{c[1]}" + (f"-{c[2]}" if c[2] else "") + (f"-{c[3]}" if len(c) > 3 else "")


def config(d, lname, ename=None, **kw):
    extra = {"keypoint_encoder": ENCODERS[ename]} if ename else {}
    return util.sg_config(d, GNN_layers=list(LISTS[lname]), **extra, **kw)


@functools.lru_cache(maxsize=None)
def state(d, lname, ename=None, variant="t"):
    """The "t" weight set (trained-model-like score statistics: the reference's own fp32 forward stays inside the bar of its float64
    self, so a result can be held element-wise) or the default one.  The "t" set's calibrated statistics exist for d = 128 and 256
    only; at d = 64 the same seeded values and the "t" gains (synth.SGT_GAINS[64]) carry the default set's calibrated BatchNorm
    statistics and bin_score.  That choice is judged like the "t" set was, by the reference alone: test_sg_shapes_host.py holds the
    oracle's fp32 forward on it to half the bar."""
    from image_matching_amd import synth
    kenc, nl = ENCODERS[ename] if ename else None, len(LISTS[lname])
    if variant in VARIANT_GAINS:      # the "t" set with some projections of every layer scaled down (see VARIANT_GAINS)
        sub, g = VARIANT_GAINS[variant]
        return {k: (v * g if any(x in k for x in sub) else v) for k, v in state(d, lname, ename, "t").items()}
    if variant == "t" and d == 64:
        kenc = kenc or synth.SG_CONFIGS[d][0]
        sd = synth.synth_state_dict(synth.superglue_shapes(d, kenc, nl), synth.SG_SEED, gains=synth.SGT_GAINS[d])
        synth.apply_bn_stats(sd, {k: v for k, v in synth.calibrated_stats(f"sg{d}").items() if k in sd})
        sd["bin_score"] = np.float32(synth._stats()[f"sg{d}/bin_score"]).reshape(())
        return util.to_torch(sd)
    return util.sg_sd(d, kenc, nl, variant=variant)


@functools.lru_cache(maxsize=None)
def _superpoint(seed, d):
    from oracle import superpoint_ref
    sd = util.sp_sd(d)
    out = [superpoint_ref.superpoint_forward(x, sd, util.sp_config(d, K)) for x in util.pair(seed, H, W)]
    assert all(o["keypoints"][0].shape[0] == K for o in out), (seed, d)      # N0p % 128 == 0: what the fp16-plane linear chain needs
    return out


def pair_inputs(d, seed0=SEED, seed1=SEED):
    """The oracle's SuperPoint on side 0 of pair `seed0` and side 1 of pair `seed1`, as SuperGlue's inputs (B = 1, 256 keypoints)."""
    o0, o1 = _superpoint(seed0, d)[0], _superpoint(seed1, d)[1]
    return {"keypoints0": o0["keypoints"][0][None], "keypoints1": o1["keypoints"][0][None], "scores0": o0["scores"][0][None],
            "scores1": o1["scores"][0][None], "descriptors0": o0["descriptors"][0][None], "descriptors1": o1["descriptors"][0][None]}


def lopsided_pair(d):
    p = dict(pair_inputs(d))
    c = torch.tensor([W / 2.0, H / 2.0])
    p["keypoints1"] = c + (p["keypoints1"] - c) * LOPSIDED_SCALE
    return p


def _cut(t, key, n):
    return t[:, :, :n] if key.startswith("desc") else t[:, :n]


@functools.lru_cache(maxsize=None)
def pairs(d):
    """The three pairs of the frame, each cut to its counts: the seed's pair, the same with both keypoint orders reversed, and the same
    with the sides exchanged."""
    a = pair_inputs(d)
    flip = {k: v.flip(-1 if k.startswith("desc") else 1) for k, v in a.items()}
    swap = {k: a[k[:-1] + ("1" if k.endswith("0") else "0")] for k in KEYS}
    return tuple({k: _cut(p[k], k, n[int(k[-1])]).contiguous() for k in KEYS} for p, n in zip((a, flip, swap), COUNTS))


def frame(d):
    """(inputs (3, 256, ..), n0, n1) on the CPU: the three pairs in one frame, NaN past the counts."""
    out = {}
    for k in KEYS:
        shape = (len(COUNTS), d, K) if k.startswith("desc") else (len(COUNTS), K, 2) if k.startswith("key") else (len(COUNTS), K)
        t = torch.full(shape, float("nan"))
        for b, p in enumerate(pairs(d)):
            n = COUNTS[b][int(k[-1])]
            if k.startswith("desc"):
                t[b, :, :n] = p[k][0]
            else:
                t[b, :n] = p[k][0]
        out[k] = t
    return out, torch.tensor([c[0] for c in COUNTS], dtype=torch.int32), torch.tensor([c[1] for c in COUNTS], dtype=torch.int32)


# ---------------------------------------------------------------------------------------------- the oracle, fp32 and float64
QUANTITIES = ("kenc", "gnn", "scores_in", "Z")


def oracle_run(sd, cfg, data, dtype):
    """One pair through oracle/superglue_ref.py (dtype-agnostic) in `dtype`: {kenc: (n0 + n1, d), gnn: [per layer (n0 + n1, d)],
    scores_in (n0, n1), Z (n0 + 1, n1 + 1), matches0, matches1, matching_scores0, matching_scores1} as numpy arrays, rows = keypoints."""
    from oracle import superglue_ref
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    data = {k: v.to(dtype) for k, v in data.items()}
    r = superglue_ref.superglue_forward({**data, "image_shape0": SHAPE, "image_shape1": SHAPE}, sd, cfg, return_dense=True)
    dn = r["dense"]
    rows = lambda a, b: np.concatenate([a[0].T.numpy(), b[0].T.numpy()])
    out = {"kenc": rows(dn["kenc0"], dn["kenc1"]), "gnn": [rows(*dn["gnn_taps"][l]) for l in range(len(cfg["GNN_layers"]))],
           "scores_in": dn["scores_in"][0].numpy(), "Z": dn["Z"][0].numpy()}
    for k in ("matches0", "matches1", "matching_scores0", "matching_scores1"):
        out[k] = r[k][0].numpy()
    return out


@functools.lru_cache(maxsize=3)
def oracle(d, lname, ename=None, variant="t"):
    """[(fp32 result, float64 result) for the three pairs of the frame], once per net."""
    sd, cfg = state(d, lname, ename, variant), config(d, lname, ename)
    return [(oracle_run(sd, cfg, p, torch.float32), oracle_run(sd, cfg, p, torch.float64)) for p in pairs(d)]


def fraction(a, b64):
    """Worst |a - b| / (1e-4 + 1e-4 |b|): the fraction of the bar used against the float64 value."""
    return util.tolerance_used(a, b64) if np.size(b64) else 0.0


def dense_fractions(got, ref64):
    """{quantity: fraction of the bar} for one pair's dense results laid out like oracle_run's ('gnn': the worst layer, and which)."""
    out = {"kenc": fraction(got["kenc"], ref64["kenc"]), "scores_in": fraction(got["scores_in"], ref64["scores_in"]), "Z": fraction(got["Z"], ref64["Z"])}
    per = [fraction(g, r) for g, r in zip(got["gnn"], ref64["gnn"])]
    assert len(got["gnn"]) == len(ref64["gnn"])
    out["gnn"] = max(per) if per else 0.0
    out["gnn_layer"] = int(np.argmax(per)) if per else -1
    return out


def index_excuses(Z64, thr, mine, ref, scores_mine, scores_ref, axis, tag):
    """Rows (axis 0) or columns (axis 1) of one pair whose match index or matching score may differ from the float64 oracle's: only
    those whose float64 top-two margin of Z -- of the line itself or of the line its argmax points to -- is below 1e-3, or whose
    candidate score lies within 1e-4 of the threshold.  Every use is printed.  Returns (number excused, list of unexcused lines); the
    matching scores of all other lines are held at the bar by the caller (the returned mask marks them)."""
    Zi = Z64[:-1, :-1] if axis == 0 else Z64[:-1, :-1].T
    n, m = Zi.shape

    def gaps(A):
        if A.shape[1] < 2:
            return np.full(A.shape[0], np.inf)
        top = np.sort(A, axis=1)[:, -2:]
        return top[:, 1] - top[:, 0]
    own, other = gaps(Zi), gaps(Zi.T)
    arg = Zi.argmax(1)
    cand = np.exp(Zi[np.arange(n), arg])
    excusable = (own < 1e-3) | (other[arg] < 1e-3) | (np.abs(cand - thr) < 1e-4)
    lim = util.ATOL + util.RTOL * np.abs(scores_ref)
    differs = (mine != ref) | (np.abs(scores_mine.astype(np.float64) - scores_ref) > lim)
    bad = [int(i) for i in np.nonzero(differs & ~excusable)[0]]
    used = np.nonzero(differs & excusable)[0]
    for i in used:
        print(f"[sg-shapes excuse] {tag}: {'row' if axis == 0 else 'column'} {int(i)}: index {int(mine[i])} (float64 oracle {int(ref[i])}), score {float(scores_mine[i]):.6f} "
              f"({float(scores_ref[i]):.6f}); margins {own[i]:.2e} / {other[arg[i]]:.2e}, candidate score {cand[i]:.6f} vs threshold {thr}")
    return len(used), bad


# ---------------------------------------------------------------------------------------------- the library side (GPU tests only)
def engine(d, lname, ename=None, opts="A", variant="t", debug=True, sd=None):
    """A fresh handle for the net with the option set applied by set_option, weights loaded."""
    from image_matching_amd import _lib as L
    from image_matching_amd.engine import Engine
    eng = Engine(util.sp_config(d, K), config(d, lname, ename), "cuda")
    for key, val in OPTION_SETS[opts]:
        eng.set_option(key, val)
    eng.load_state_dict(L.NET_SUPERGLUE, sd if sd is not None else state(d, lname, ename, variant))
    eng.set_debug(debug)
    return eng


def forward(eng, t, n0=None, n1=None, forms=False):
    """One imx_superglue_forward; returns ([matches0, matches1, matching_scores0, matching_scores1] on the host, the set of (launch name,
    kernel form) pairs the timing report names when `forms`)."""
    tc = {k: v.cuda() for k, v in t.items()}
    if forms:
        eng.timing_reset()
        eng.set_timing(True)
    out = eng.superglue(tc["keypoints0"], tc["scores0"], tc["descriptors0"], SHAPE, tc["keypoints1"], tc["scores1"], tc["descriptors1"], SHAPE,
                        None if n0 is None else n0.cuda(), None if n1 is None else n1.cuda())
    torch.cuda.synchronize()
    seen = None
    if forms:
        seen = {(r[0], r[3]) for r in eng.timing_report(forms=True)}
        eng.set_timing(False)
    return [o.cpu().numpy() for o in out], seen


def library_dense(eng, n_layers, counts, alpha):
    """The library's taps of the last forward, per pair and cut to the counts, laid out like oracle_run's results."""
    B = len(counts)
    kenc, taps = eng.fetch("kenc"), [eng.fetch(f"gnn{l}") for l in range(n_layers)]
    Sall, U, V = eng.fetch("scores_in"), eng.fetch("u"), eng.fetch("v")
    _, N0p, N1p = Sall.shape
    out = []
    for b, (n0, n1) in enumerate(counts):
        rows = lambda a: np.concatenate([a[b * N0p:b * N0p + n0], a[B * N0p + b * N1p:B * N0p + b * N1p + n1]])
        out.append({"kenc": rows(kenc), "gnn": [rows(t) for t in taps], "scores_in": Sall[b, :n0, :n1],
                    "Z": util.transport_Z(Sall[b], U[b], V[b], n0, n1, alpha)})
    return out


def check_against_oracle(tag, dense, outs, ref, counts, thr, anchored=False):
    """The library's dense results and outputs of one forward against the oracle's per-pair results `ref` = [(fp32, float64)]: kenc,
    every layer's output, scores_in, Z and the matching scores element-wise at 1e-4 + 1e-4 |x64| on the valid rows (anchored = True:
    only the indices and the padding; the caller anchors the dense quantities), -1 / 0 past the counts, match indices equal to the
    float64 oracle's except on excusable lines (index_excuses), at most 1 % of the case's keypoints.  Prints and returns the worst
    fraction of the bar per quantity."""
    m0, m1, ms0, ms1 = outs
    worst, excused, bad, total = {q: 0.0 for q in QUANTITIES + ("mscores",)}, 0, [], 0
    for b, (n0, n1) in enumerate(counts):
        r64 = ref[b][1]
        assert (m0[b, n0:] == -1).all() and (m1[b, n1:] == -1).all() and (ms0[b, n0:] == 0).all() and (ms1[b, n1:] == 0).all(), f"{tag} pair {b}: outputs past the counts"
        if not anchored:
            fr = dense_fractions(dense[b], r64)
            for q in QUANTITIES:
                worst[q] = max(worst[q], fr[q])
            print(f"[sg-shapes] {tag} pair {b} ({n0} x {n1}): fraction of 1e-4 + 1e-4|x64| used: kenc {fr['kenc']:.3f}, gnn {fr['gnn']:.3f} (layer {fr['gnn_layer']}), "
                  f"scores_in {fr['scores_in']:.3f}, Z {fr['Z']:.3f}")
        for axis, mine, sc, n in ((0, m0[b, :n0], ms0[b, :n0], n0), (1, m1[b, :n1], ms1[b, :n1], n1)):
            rs = r64[f"matching_scores{axis}"]
            e, bd = index_excuses(r64["Z"], thr, mine, r64[f"matches{axis}"], sc, rs, axis, f"{tag} pair {b}")
            excused += e
            bad += [(b, axis, i) for i in bd]
            ok = (mine == r64[f"matches{axis}"]) & (np.abs(sc.astype(np.float64) - rs) <= util.ATOL + util.RTOL * np.abs(rs))
            if ok.any():
                worst["mscores"] = max(worst["mscores"], fraction(sc[ok], rs[ok]))
        total += n0 + n1
    shown = {q: v for q, v in worst.items() if not anchored or q == "mscores"}
    print(f"[sg-shapes] {tag}: worst fractions {', '.join(f'{q} {v:.3f}' for q, v in shown.items())}; {excused} of {total} keypoints excused")
    assert not bad, f"{tag}: match indices / matching scores differ from the float64 oracle's on lines with no excuse (pair, axis, line): {bad[:8]}"
    assert excused <= 0.01 * total, f"{tag}: {excused} of {total} keypoints needed an excuse (at most 1 %)"
    if not anchored:
        over = {q: v for q, v in worst.items() if v > 1.0}
        assert not over, f"{tag}: outside 1e-4 + 1e-4|x64| of the float64 oracle: {over}"
    return worst
