"""The shape lists of tests/superpoint_tiles.py reach every code path of SuperPoint's 3x3 layers that they claim to reach (no GPU:
the host rules restated in superpoint_tiles.variants, evaluated at the MI355X's 256 CUs), and every shape of the lists is needed."""
import json
import os

import pytest

from tests import superpoint_tiles as T
from tests import util

# the dense SuperPoint configurations of the form census (tools/form_census.py: CONFIGS) with the default weights: H, W, images,
# "conv", "conv_swizzle" ("mfma" = "f32" rules the fp16 chain out: the forms of "wino32")
CENSUS = {"sp/123x165_b40": (123, 165, 40, "wino", True), "sp/123x165_b40/conv_swizzle_off": (123, 165, 40, "wino", False),
          "sp/123x165_b40/conv_wino_h": (123, 165, 40, "wino_h", True), "sp/123x165_b40/conv_wino32": (123, 165, 40, "wino32", True),
          "sp/123x165_b40/conv_direct": (123, 165, 40, "direct", True), "sp/123x165_b40/mfma_f32": (123, 165, 40, "wino32", True),
          "sp/72x104_b260_two_slices_off": (72, 104, 260, "wino", True), "sp/120x160_b2_tile_form": (120, 160, 2, "wino", True)}


def _reached(large=T.LARGE, small=T.SMALL):
    cells = set()
    for c in large:
        cells |= T.large_cells(*c)
    for c in small:
        cells |= T.small_cells(*c)
    return cells


def test_the_shape_lists_reach_every_cell_of_the_coverage_table():
    missing = T.required_cells() - _reached()
    assert not missing, sorted(map(str, missing))


@pytest.mark.parametrize("case", T.LARGE + T.SMALL, ids=lambda c: "x".join(map(str, c[:2])) + (f"_b{c[2]}" if len(c) == 3 else ""))
def test_every_shape_of_the_lists_is_needed(case):
    rest = _reached([c for c in T.LARGE if c != case], [c for c in T.SMALL if c != case])
    assert T.required_cells() - rest, f"{case} reaches nothing the other shapes do not reach: drop it or say what it is for"


@pytest.mark.parametrize("name", list(CENSUS))
def test_the_restated_rules_reproduce_the_recorded_form_census(name):
    """tests/golden/form_census.json holds the timing report's rows of these forwards as a device produced them: the restatement must
    predict the rows of the eight layers, in order, at the recorded CU count."""
    with open(os.path.join(util.GOLDEN, "form_census.json")) as fh:
        rec = json.load(fh)
    H, W, B, conv, swizzle = CENSUS[name]
    rows = [(r[0], r[1]) for r in rec["configs"][name]["rows"] if r[0] in T.NAMES]
    assert T.report_rows(T.variants(H, W, B, rec["cu_count"], conv, swizzle)) == rows


def test_the_restated_rules_on_shapes_whose_forms_the_suite_already_asserts():
    """Anchors of the restatement at 256 CUs, each taken from a test that asserts the same forms on the device
    (tests/test_gpu_superpoint.py; tests/golden/form_census.json, recorded at 256 CUs)."""
    forms = lambda *a, **k: {(v.slice, v.name): v.form for v in T.variants(*a, **k)}
    f = forms(72, 104, 48, 256)       # the stress batch of 48: pair forms on the first levels
    assert f[0, "conv1ab_pool"] == T.PAIR1 and f[0, "conv2a"] == f[0, "conv2b_pool"] == f[0, "conv3a"] == T.PAIR
    f = forms(72, 104, 8, 256)
    assert f[0, "conv1ab_pool"] == T.TILE1 and f[0, "conv4b"] == T.TILE
    f = forms(72, 104, 260, 256)      # census "sp/72x104_b260_two_slices_off": every layer a pair in the first slice, a tile form in the second
    assert all(f[0, n] == (T.PAIR1 if n == "conv1ab_pool" else T.PAIR) and f[1, n] == (T.TILE1 if n == "conv1ab_pool" else T.TILE) for n in T.NAMES)
    f = forms(120, 160, 2, 256)       # census "sp/120x160_b2_tile_form"
    assert all(f[0, n] == (T.TILE1 if n == "conv1ab_pool" else T.TILE) for n in T.NAMES)
    assert set(forms(123, 165, 40, 256, conv="wino32").values()) == {T.F321, T.F32}
    assert set(forms(123, 165, 40, 256, conv="direct").values()) == {T.DIRECT}
    v = {x.name: x for x in T.variants(123, 165, 40, 256)}      # census "sp/123x165_b40": the pair form, swizzled
    assert v["conv2a"].form == T.PAIR and v["convPaDa"].form == T.PAIR and v["conv2a"].out == 2 and v["conv2b_pool"].inz and not v["conv2a"].fastw


def test_the_largest_batch_stays_at_4_2_megapixels_and_the_image_order_is_not_periodic():
    assert max(H * W * B for H, W, B in T.LARGE) <= 128 * 256 * 128
    order = T.image_order(260)
    assert sorted(set(order)) == list(range(16))
    # the two tiles of a pair (neighbouring images where an image is one tile) and the slots 2 and 16 apart hold different images
    assert all(order[i] != order[i + s] for s in (1, 2, 16) for i in range(260 - s))
