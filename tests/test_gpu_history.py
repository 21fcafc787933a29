"""History independence: what a handle returns must not depend on what it computed before.  Its workspaces are hipMalloc'd
uninitialised, reused across calls and shapes, and re-allocated when they grow; several kernels skip regions nobody wrote in the
current call (padded tiles of the swizzled tensors, the short last slice's maxima table, Sinkhorn slab rows past the count, key tiles
past the count, candidate buffers past an image's yield).  On a fresh handle those regions are usually zero, so a read that should
have been masked is invisible.  Every test here compares a used or poisoned handle ("debug_poison": include/imx.h) with THE SAME CALL
ON A FRESH HANDLE, bit for bit, on every output and on the valid region of the taps.  Nothing here provokes a fault: the hook writes
values into float workspaces only (imx_host.h: poisonable()).  Needs an MI355X.
Wall time on an MI355X: 22 s alone (tests/test_gpu_padding.py: 14 s); the whole GPU suite with both 540 s, about 505 s without them."""
import numpy as np
import pytest
import torch

from tests import util
from tests.test_gpu_padding import CASES, make_inputs, poison_padding, run_with_counts, sg_weights

pytestmark = pytest.mark.gpu
POISONS = ("nan", "huge", "zero")          # NaN first: the pattern that shows a read soonest


def _engine(d=128, K=64, sp=True, sg=False, opts=(), sg_sd=None, sp_sd=None, **sp_kw):
    from image_matching_amd import _lib as L
    from image_matching_amd.engine import Engine
    eng = Engine(util.sp_config(d, K, **sp_kw), util.sg_config(d), "cuda")
    if sp:
        eng.load_state_dict(L.NET_SUPERPOINT, sp_sd if sp_sd is not None else util.sp_sd(d))
    if sg:
        eng.load_state_dict(L.NET_SUPERGLUE, sg_sd if sg_sd is not None else sg_weights(d))
    for k, v in opts:
        eng.set_option(k, v)
    return eng


_IMAGES = {}


def _images(seed, H, W, B):
    if (seed, H, W, B) not in _IMAGES:
        base = [util.pair(seed + i, H, W)[i & 1] for i in range(min(B, 8))]
        _IMAGES[seed, H, W, B] = torch.cat([base[i % 8] * (1.0 + (i % 5)) for i in range(B)])
    return _IMAGES[seed, H, W, B].cuda()


def _same(got, want, tag):
    assert got.keys() == want.keys(), (tag, sorted(got), sorted(want))
    for k, w in want.items():
        g = got[k]
        if isinstance(w, torch.Tensor):
            assert g.shape == w.shape and g.dtype == w.dtype, f"{tag}: {k}: {tuple(g.shape)} {g.dtype} vs {tuple(w.shape)} {w.dtype}"
            bad = int((g.view(torch.int32) != w.view(torch.int32)).sum()) if w.dtype == torch.float32 else int((g != w).sum())
            assert bad == 0, (f"{tag}: {k} differs from the fresh handle's in {bad} of {w.numel()} elements"
                              + (f" (non-finite: {int((~torch.isfinite(g)).sum())})" if w.dtype == torch.float32 else ""))
        else:
            assert g == w, f"{tag}: {k}: {g} vs {w}"


# ---------------------------------------------------------------------------------------------- calls: fn(eng) -> {name: tensor}
def call_dense(H, W, B, seed=700):
    def fn(eng):
        semi, desc = eng.superpoint_dense(_images(seed, H, W, B))
        torch.cuda.synchronize()
        return {"semi": semi.cpu(), "desc": desc.cpu()}
    return fn


def call_superpoint(H, W, B, seed=700):
    def fn(eng):
        kpts, scores, desc, n = eng.superpoint(_images(seed, H, W, B))
        torch.cuda.synchronize()
        return {"keypoints": kpts.cpu(), "scores": scores.cpu(), "descriptors": desc.cpu(), "counts": list(n)}
    return fn


def call_match_pairs(H, W, seeds):
    def fn(eng):
        base = [util.pair(s, H, W) for s in seeds]
        out = eng.match_pairs(torch.cat([p[0] for p in base]).cuda(), torch.cat([p[1] for p in base]).cuda(), want_desc=True)
        rec = eng.pack_records(list(range(len(seeds))), out, pad_to=len(seeds) + 3)
        torch.cuda.synchronize()
        res = {k: v.cpu() for k, v in out.items()}
        res["records"] = rec.cpu()
        return res
    return fn


def call_superglue(case):
    d, N0, N1, n0, n1, opts, _ = CASES[case]
    want_amax = opts.get("mfma") != "f32" and opts.get("attention") != "bf16x3"
    t = poison_padding(make_inputs(d, len(n0), N0, N1, seed=4242), n0, n1, "nan")

    def fn(eng):
        eng.set_debug(True)
        res = run_with_counts(eng, t, n0, n1, want_amax)
        flat = dict(zip(("matches0", "matches1", "matching_scores0", "matching_scores1"), res.pop("tail")))
        if want_amax:
            flat["amax"] = res.pop("amax")
        for b, r in res.items():
            flat.update({f"pair{b}/{k}": v for k, v in r.items()})
        return flat
    return fn


def call_registration(eng):
    """knn_ratio_match, estimate_affine_partial, ingest and warp_affine_u8 in one go (their workspaces: knn.*, ransac.scratch)."""
    g = torch.Generator().manual_seed(9)
    t = make_inputs(128, 2, 200, 150, seed=11)
    m, d1, d2 = eng.knn_ratio_match(t["descriptors0"].cuda(), t["descriptors0"][:, :, :150].cuda(), 0.9,
                                    torch.tensor([137, 200], dtype=torch.int32, device="cuda"), torch.tensor([150, 45], dtype=torch.int32, device="cuda"))
    K = 9000                                            # beyond the LDS slots of the RANSAC kernel: its coordinates live in ransac.scratch
    k0 = torch.rand(2, K, 2, generator=g) * 500
    k1 = k0 * 1.02 + 5.0 + torch.randn(2, K, 2, generator=g)
    m0 = torch.arange(K).repeat(2, 1)
    m0[:, ::3] = -1
    M, inl, ninl = eng.estimate_affine_partial(k0.cuda(), k1.cuda(), m0.cuda(), counts0=torch.tensor([K, 4000], dtype=torch.int32, device="cuda"))
    u8 = (torch.rand(2, 90, 130, generator=g) * 255).to(torch.uint8)
    ing = eng.ingest(u8.cuda(), (72, 104))
    wp = eng.warp_affine_u8(u8[0].cuda(), [[1.0, 0.05, 3.0], [-0.05, 1.0, -2.0]], (80, 120))
    torch.cuda.synchronize()
    return {"knn_matches": m.cpu(), "knn_d1": d1.cpu(), "knn_d2": d2.cpu(), "M": M.cpu(), "inliers": inl.cpu(), "n_inliers": ninl.cpu(),
            "ingest": ing.cpu(), "warp": wp.cpu()}


# id -> (engine keyword arguments, call)
POISON_CALLS = {
    "dense_123x165_b40_pair_form": (dict(), call_dense(123, 165, 40)),
    "dense_72x104_b260_two_slices": (dict(opts=(("latency_forms", "off"),)), call_dense(72, 104, 260, seed=900)),
    "dense_120x160_b2_tile_form": (dict(), call_dense(120, 160, 2)),
    "dense_123x165_b5_wino32": (dict(opts=(("conv", "wino32"),)), call_dense(123, 165, 5)),
    "dense_123x165_b5_direct": (dict(opts=(("conv", "direct"),)), call_dense(123, 165, 5)),
    "keypoints_bits_k_below_yield": (dict(K=30, opts=(("keypoints", "bits"),)), call_superpoint(123, 165, 3)),
    "keypoints_bits_k_above_yield": (dict(K=5000, opts=(("keypoints", "bits"),)), call_superpoint(123, 165, 3)),
    "keypoints_dense_k_below_yield": (dict(K=30, opts=(("keypoints", "dense"),)), call_superpoint(123, 165, 3)),
    "keypoints_dense_k_above_yield": (dict(K=5000, opts=(("keypoints", "dense"),)), call_superpoint(123, 165, 3)),
    "keypoints_all": (dict(K=-1), call_superpoint(72, 104, 3)),
    "match_pairs_counts_differ": (dict(K=2500, sg=True, opts=(("latency_forms", "off"),)), call_match_pairs(200, 264, (40, 41, 42))),
    "superglue_throughput": (dict(sp=False, sg=True), call_superglue("throughput_d128_b17_auto")),
    "superglue_latency": (dict(sp=False, sg=True), call_superglue("latency_d128_b3")),
    "superglue_keysplit_d256": (dict(d=256, sp=False, sg=True), call_superglue("keysplit_d256_b1")),
    "superglue_linear_h2_d256": (dict(d=256, sp=False, sg=True, opts=(("latency_forms", "off"),)), call_superglue("linear_h2_d256_off")),
    "superglue_fused_merge": (dict(sp=False, sg=True, opts=(("latency_forms", "off"), ("sinkhorn_group", "2"), ("sinkhorn_merge", "fused"))),
                              call_superglue("sinkhorn_group_2_fused_merge_off")),
    "registration_and_ingest": (dict(sp=False), call_registration),
}


@pytest.mark.parametrize("name", sorted(POISON_CALLS))
def test_poisoned_workspaces_between_calls_change_nothing(name):
    """Warm the handle with the call, fill its float workspaces with NaN / 3.4e38 / zero bytes, repeat the call: every output (and, for
    SuperGlue, the valid region of every tap and the maxima table) equals the same call on a fresh handle.  A third handle runs the call
    with the hook armed from the start, so every workspace is ALLOCATED poisoned."""
    kw, fn = POISON_CALLS[name]
    want = fn(_engine(**kw))
    eng = _engine(**kw)
    _same(fn(eng), want, f"{name}: a second fresh handle")
    for p in POISONS:
        eng.set_option("debug_poison", p)
        assert eng.get_option("debug_poison") == p
        _same(fn(eng), want, f"{name}: after debug_poison = {p}")
    eng.set_option("debug_poison", "off")
    assert eng.get_option("debug_poison") == "off"
    cold = _engine(**kw)
    cold.set_option("debug_poison", "nan")
    _same(fn(cold), want, f"{name}: workspaces allocated under debug_poison = nan")


def test_shape_history_superpoint():
    """large -> small -> large and small -> large on one handle (image size and batch; the second forces ws() to grow), dense and keypoint
    calls interleaved: each result equals a fresh handle's."""
    calls = {"big": call_dense(123, 165, 40), "small": call_dense(72, 104, 3, seed=900), "kp_small": call_superpoint(64, 72, 2, seed=900),
             "kp_big": call_superpoint(123, 165, 7)}
    want = {k: fn(_engine(K=50)) for k, fn in calls.items()}
    for order in (("big", "small", "kp_small", "big", "kp_big", "small"), ("small", "big"), ("kp_small", "kp_big", "small", "kp_small")):
        eng = _engine(K=50)
        for i, k in enumerate(order):
            _same(calls[k](eng), want[k], f"superpoint history {order}: step {i} ({k})")


def test_shape_history_superglue_and_match_pairs():
    """SuperGlue large -> small -> large and small -> large (K and B change; d is fixed per handle), and match_pairs between
    superpoint_dense and superpoint calls on the same handle."""
    big, small = call_superglue("throughput_d128_b17_auto"), call_superglue("latency_d128_b3")
    want = {"big": big(_engine(sp=False, sg=True)), "small": small(_engine(sp=False, sg=True))}
    for order in (("big", "small", "big"), ("small", "big", "small")):
        eng = _engine(sp=False, sg=True)
        for i, k in enumerate(order):
            _same({"big": big, "small": small}[k](eng), want[k], f"superglue history {order}: step {i} ({k})")
    kw = dict(K=300, sg=True, opts=(("latency_forms", "off"),))
    calls = {"mp_big": call_match_pairs(200, 264, (40, 41, 42)), "mp_small": call_match_pairs(120, 160, (43,)), "dense": call_dense(123, 165, 5),
             "kp": call_superpoint(72, 104, 2, seed=900)}
    want = {k: fn(_engine(**kw)) for k, fn in calls.items()}
    for order in (("mp_big", "dense", "mp_small", "kp", "mp_big"), ("mp_small", "kp", "mp_big", "dense", "mp_small")):
        eng = _engine(**kw)
        for i, k in enumerate(order):
            _same(calls[k](eng), want[k], f"match_pairs history {order}: step {i} ({k})")


OPTION_FLIPS = (("mfma", "f32", "x3"), ("conv", "direct", "wino"), ("conv", "wino32", "wino"), ("attention", "bf16x3", "auto"), ("gnn_tail", "unfused", "auto"),
                ("gnn_tail", "bf16x3", "auto"), ("linear", "bf16x3", "auto"), ("latency_forms", "on", "off"), ("latency_forms", "auto", "off"),
                ("sinkhorn_group", "1", "auto"), ("sinkhorn_group", "4", "auto"), ("sinkhorn_merge", "fused", "auto"), ("sinkhorn_prefetch", "on", "auto"),
                ("keypoints", "dense", "auto"), ("conv_swizzle", "off", "on"), ("qkv_amax", "kernel", "epilogue"), ("attention_qblocks", "2", "auto"))


def test_option_history():
    """Every option flipped away and back with a call in between: the last result equals the first (images in, 3 pairs whose counts
    differ, the throughput forms as the baseline)."""
    fn = call_match_pairs(200, 264, (40, 41, 42))
    eng = _engine(K=2500, sg=True, opts=(("latency_forms", "off"),))
    want = fn(eng)
    for key, away, back in OPTION_FLIPS:
        eng.set_option(key, away)
        fn(eng)
        eng.set_option(key, back)
        _same(fn(eng), want, f"option history: {key} = {away} and back to {back}")


def test_weight_reload_leaves_nothing_behind():
    """The heavy weight sets (guards trip, other packed planes), a call, then the default sets on the same handle: the result equals a
    fresh handle with the default sets, and the guards report what the fresh handle reports."""
    from image_matching_amd import _lib as L, synth
    fn = call_match_pairs(200, 264, (40, 41, 42))
    kw = dict(K=2500, sg=True, opts=(("latency_forms", "off"),))
    fresh = _engine(**kw)
    want, guard = fn(fresh), fresh.get_option("arith_guard")
    eng = _engine(**kw, sp_sd=util.to_torch(synth.make_superpoint_state_dict(128, heavy=True)),
                  sg_sd=util.to_torch(synth.make_superglue_state_dict(128, heavy=True)))
    assert eng.get_option("arith_guard") != guard, "the heavy sets must move a guard, or the reload has nothing to leave behind"
    fn(eng)
    eng.load_state_dict(L.NET_SUPERPOINT, util.sp_sd(128))
    eng.load_state_dict(L.NET_SUPERGLUE, sg_weights(128))
    assert eng.get_option("arith_guard") == guard
    _same(fn(eng), want, "default weights after the heavy sets on the same handle")


def test_lazy_nms_tap_follows_the_last_forward():
    """The "nms" tap under "keypoints" = bits is computed when it is fetched, from the last detect's score map: it must equal the dense
    form's map -- also after a second, LARGER forward re-allocated every workspace (then it is the SECOND call's map)."""
    maps = {}
    for mode in ("dense", "bits"):
        eng = _engine(K=50, opts=(("keypoints", mode),))
        eng.set_debug(True)
        call_superpoint(72, 104, 2, seed=900)(eng)
        maps[mode, "small"] = eng.fetch("nms").copy()
        call_superpoint(123, 165, 7)(eng)
        maps[mode, "big"] = eng.fetch("nms").copy()
    for size in ("small", "big"):
        assert maps["dense", size].shape == maps["bits", size].shape and (maps["dense", size] > 0).any()
        assert np.array_equal(maps["dense", size], maps["bits", size]), f"nms tap ({size} call): the lazily computed map differs from the dense form's"
