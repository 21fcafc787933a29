"""SuperPoint's eight 3x3 inference layers at every tile variant the image shape can select, layer by layer (DESIGN.md section 4:
the coverage table).  tests/superpoint_tiles.py restates the host rules that pick the variants and holds the shape lists;
tests/test_superpoint_tiles_host.py proves on the CPU that the lists reach every variant.  Here, on the device:

  (a) the taps a1 = pool(x1), a2 = pool(x2), a3 = pool(x3), x4, semi and the normalised dense descriptors against the reference's own
      stages evaluated in float64 (oracle/superpoint_ref.py: _double_conv, max_pool2d, heads_bn), element-wise at the project's
      1e-4 + 1e-4|ref| -- "conv" = "wino_h", "wino32" and "direct" on two images of every small shape, "wino_h" on the large batches;
  (b) on the large batches, the pair forms ("conv" = "wino", tile-swizzled and with "conv_swizzle" = "off") bit for bit against the
      tile-per-workgroup form ("wino_h") on every tap and output, every copy of an image against its first copy, and images of a
      260-image batch against the same image alone;
  (c) the forms of the timing report against what the restated rules predict for the device's CU count: a case cannot silently
      test another kernel.

A batch holds 16 distinct images in an order that is periodic neither in 2 nor in 16 (superpoint_tiles.image_order), so the two tiles
of a pair, and neighbouring items of a persistent workgroup, belong to different images.  Every test prints the fraction of the bar
each tap uses before it asserts.  Needs an MI355X."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import superpoint_tiles as T
from tests import util

pytestmark = pytest.mark.gpu
D = 128
TAPS = ("a1", "a2", "a3", "x4", "semi", "desc_raw")
MODES = ("wino_h", "wino", "wino/blocked")       # "conv" / "conv_swizzle" = "off"
LARGE_HW = {c[:2] for c in T.LARGE}
_ids = lambda c: "x".join(map(str, c[:2])) + (f"_b{c[2]}" if len(c) == 3 else "")


@functools.lru_cache(maxsize=None)
def _weights():
    sd = util.sp_sd(D)
    return sd, {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def _engine():
    from image_matching_amd import _lib as L
    from image_matching_amd.engine import Engine
    eng = Engine(util.sp_config(D, 64), util.sg_config(D), "cuda")
    eng.load_state_dict(L.NET_SUPERPOINT, _weights()[0])
    eng.set_debug(True)
    return eng


def _cu():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@functools.lru_cache(maxsize=None)
def _images(H, W):
    """The 16 distinct images of a shape: both sides of eight synthetic pairs."""
    return torch.cat([util.pair(1200 + k // 2, H, W)[k & 1] for k in range(16)])


@functools.lru_cache(maxsize=None)
def _f64(H, W, ks):
    """The float64 stages of images `ks` of the shape, NCHW, computed once and shared: {tap: array (len(ks), C, h, w)}."""
    from oracle import superpoint_ref as R
    sd64 = _weights()[1]
    with torch.no_grad():
        x = _images(H, W)[list(ks)].double()
        a1 = F.max_pool2d(R._double_conv(x, sd64, "inc.conv.conv"), 2)
        a2 = F.max_pool2d(R._double_conv(a1, sd64, "down1.mpconv.1.conv"), 2)
        a3 = F.max_pool2d(R._double_conv(a2, sd64, "down2.mpconv.1.conv"), 2)
        x4 = R._double_conv(a3, sd64, "down3.mpconv.1.conv")
        semi, desc = R.heads_bn(x4, sd64)
    return {"a1": a1.numpy(), "a2": a2.numpy(), "a3": a3.numpy(), "x4": x4.numpy(), "semi": semi.numpy(), "desc_raw": desc.numpy()}


def _nchw_taps(taps):
    """The library's NHWC taps as the reference lays them out, the raw descriptors divided by their channel norm (superpoint_test.py:125-126)."""
    out = {k: np.transpose(v, (0, 3, 1, 2)) for k, v in taps.items()}
    out["desc_raw"] = out["desc_raw"] / np.linalg.norm(out["desc_raw"], axis=1, keepdims=True)
    return out


def _hold_to_float64(mine, ref, what):
    used = {k: util.tolerance_used(mine[k], ref[k]) for k in TAPS}
    print(f"[tiles] {what}: fraction of 1e-4 + 1e-4|f64| used: " + "  ".join(f"{k.replace('desc_raw', 'desc')} {used[k]:.3f}" for k in TAPS))
    for k in TAPS:
        assert np.isfinite(mine[k]).all(), f"{what}: {k} holds non-finite values"
        util.assert_close(mine[k], ref[k], f"{what}: {k} against the float64 stage")
    return used


def _detect(eng, x, conv, swizzle="on"):
    """One detecting call under the given options with timing on: (keypoints, scores, descriptors, counts), the report's (name, form)
    rows of the eight layers, and the six taps as the library lays them out (NHWC)."""
    eng.set_option("conv_swizzle", swizzle)
    eng.set_option("conv", conv)
    assert eng.get_option("conv") == conv
    eng.timing_reset()
    eng.set_timing(True)
    try:
        out = eng.superpoint(x)
        torch.cuda.synchronize()
        rows = [(r[0], r[3]) for r in eng.timing_report(forms=True) if r[0] in T.NAMES]
    finally:
        eng.set_timing(False)
    return out, rows, {k: eng.fetch(k) for k in TAPS}


def _restore(eng):
    eng.set_option("conv", "wino")
    eng.set_option("conv_swizzle", "on")
    eng.set_option("latency_forms", "auto")


# ------------------------------------------------------------------------------------------------- two images: the tile forms, (a) and (c)
@pytest.mark.parametrize("shape", T.SMALL, ids=_ids)
def test_every_tap_of_the_tile_per_workgroup_fp32_and_direct_forms_against_float64(shape):
    """"conv" = "wino_h" (conv3x3_wino24h / conv1ab_wino24h), "wino32" (conv3x3_wino24 / conv1ab_wino24) and "direct" (conv3x3_direct)
    on two images of every small shape: whole and partial tiles on either axis and on both, levels smaller than a tile and of a single
    pixel, for the direct kernel a level narrower than, exactly and one column beyond its 32-column tile.  A wrong halo column at level
    1 shows at a1, not six layers later."""
    H, W = shape
    eng = _engine()
    order = T.image_order(T.SMALL_B)
    ks = tuple(range(16)) if (H, W) in LARGE_HW else tuple(order)      # (a shape shared with a large batch shares its float64 stages)
    ref = {k: v[[ks.index(i) for i in order]] for k, v in _f64(H, W, ks).items()}
    x = _images(H, W)[order].cuda()
    try:
        for conv in ("wino_h", "wino32", "direct"):
            _, rows, taps = _detect(eng, x, conv)
            assert rows == T.report_rows(T.variants(H, W, T.SMALL_B, _cu(), conv)), (conv, rows)
            _hold_to_float64(_nchw_taps(taps), ref, f"{H}x{W} b{T.SMALL_B} {conv}")
    finally:
        _restore(eng)


# ------------------------------------------------------------------------------------------------- large batches: the pair forms
@functools.lru_cache(maxsize=None)
def _large(case):
    """The three settings on one large batch, reduced to what the tests below assert (the taps of a 4.2-Mpixel batch are 450 MB per
    setting: compared here and dropped)."""
    H, W, B = case
    eng = _engine()
    order = T.image_order(B)
    slots = {k: [i for i, o in enumerate(order) if o == k] for k in range(16)}
    x = _images(H, W)[order].cuda()
    res = {"rows": {}, "differs": {}, "copies": [], "alone": []}
    try:
        if B > T.SLICE:         # (the 1x1 heads of a single image would otherwise take their latency form: another summation order)
            eng.set_option("latency_forms", "off")
        first = None
        for mode in MODES:
            conv, swizzle = mode.split("/")[0], "off" if mode.endswith("/blocked") else "on"
            (kp, sc, de, n), rows, cur = _detect(eng, x, conv, swizzle)
            res["rows"][mode] = rows
            semi, desc = eng.superpoint_dense(x)
            cur.update({"dense semi": semi.cpu().numpy(), "dense desc": desc.cpu().numpy(), "keypoints": kp.cpu().numpy(),
                        "scores": sc.cpu().numpy(), "descriptors": de.cpu().numpy(), "counts": np.asarray(n)})
            if first is None:
                first = cur
                res["first_slot"] = _nchw_taps({k: cur[k][[slots[i][0] for i in range(16)]] for k in TAPS})
                res["keypoints"] = int(np.asarray(n).sum())
                for k, v in cur.items():
                    for i in range(16):
                        bad = [b for b in slots[i][1:] if not np.array_equal(v[b], v[slots[i][0]])]
                        if bad:
                            res["copies"].append(f"{k}: slots {bad[:4]} differ from slot {slots[i][0]} (image {i})")
            else:
                res["differs"][mode] = [f"{k}: first differing slots {[b for b in range(B) if not np.array_equal(cur[k][b], first[k][b])][:4]}"
                                        for k in cur if not np.array_equal(cur[k], first[k])]
            if mode == "wino" and B > T.SLICE:
                for b in (0, 255, 256, 259):
                    s1, d1 = eng.superpoint_dense(x[b:b + 1])
                    if not (torch.equal(s1[0], semi[b]) and torch.equal(d1[0], desc[b])):
                        res["alone"].append(b)
    finally:
        _restore(eng)
    return res


@pytest.mark.parametrize("case", T.LARGE, ids=_ids)
def test_the_pair_forms_run_where_the_restated_rules_say(case):
    """(c) The timing report's forms of all eight layers, per slice, under the three settings."""
    H, W, B = case
    cu = _cu()
    is_pair = lambda vs: [v.form in (T.PAIR, T.PAIR1) for v in vs]
    if is_pair(T.variants(H, W, B, cu)) != is_pair(T.variants(H, W, B, T.CU)):
        pytest.skip(f"with {cu} CUs instead of {T.CU} this case loses (or gains) a pair-form layer: it would not run what it is listed for")
    rows = _large(case)["rows"]
    assert rows["wino"] == T.report_rows(T.variants(H, W, B, cu, "wino", True)), rows["wino"]
    assert rows["wino/blocked"] == T.report_rows(T.variants(H, W, B, cu, "wino", False)), rows["wino/blocked"]
    assert rows["wino_h"] == T.report_rows(T.variants(H, W, B, cu, "wino_h")), rows["wino_h"]
    assert ("conv4a", T.PAIR) in rows["wino"] and ("conv4b", T.PAIR) in rows["wino"] and ("conv1ab_pool", T.PAIR1) in rows["wino"]
    assert all(f in (T.TILE, T.TILE1) for _, f in rows["wino_h"])


@pytest.mark.parametrize("case", T.LARGE, ids=_ids)
def test_the_pair_forms_swizzled_and_blocked_equal_the_tile_form_bit_for_bit_on_every_tap(case):
    """(b) a1, a2, a3, x4, semi, the raw descriptors, superpoint_dense's semi and desc, keypoints, scores, descriptors and counts of
    "conv" = "wino" and of "wino" with "conv_swizzle" = "off" equal those of "wino_h" for every image; every copy of an image equals
    its first copy; images 0, 255, 256 and 259 of the 260-image batch equal the same image alone."""
    res = _large(case)
    assert res["keypoints"] > 0, "the case must produce keypoints"
    assert not res["differs"]["wino"], f"pair form vs tile-per-workgroup form: {res['differs']['wino']}"
    assert not res["differs"]["wino/blocked"], f"pair form on blocked tensors vs tile-per-workgroup form: {res['differs']['wino/blocked']}"
    assert not res["copies"], res["copies"][:6]
    assert not res["alone"], f"images {res['alone']} of the batch differ from the same image alone"


@pytest.mark.parametrize("case", T.LARGE, ids=_ids)
def test_the_first_slot_of_each_image_of_a_large_batch_against_float64(case):
    """(a) on the large batches: "wino_h" on the first slot of each of the 16 images -- with (b), the pair forms too."""
    H, W, B = case
    _hold_to_float64(_large(case)["first_slot"], _f64(H, W, tuple(range(16))), f"{H}x{W} b{B} wino_h, first slot of 16 images")
