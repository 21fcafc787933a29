"""The code paths of SuperPoint's eight 3x3 inference layers, restated once, and the image shapes that pin each of them
(tests/test_gpu_superpoint_tiles.py runs the shapes, tests/test_superpoint_tiles_host.py proves what they reach).

The IMAGE SHAPE selects these paths, not the caller.  variants() restates the host rules that do it (paths relative to
image-matching_amd/csrc):

  * imx_superpoint.cpp:14-17 (kSpLayers: level, pool, the three swizzle candidates), :22 (slices of 256 images), :90-126
    (plan_superpoint: chain, pairs, the form per layer and slice, the layout between two pair-form layers);
  * conv3x3_wino24p.hip:618-624 (conv3x3_wino24p_preferred: ceil(tiles / 2) * Cout / 64 >= CU count), :581-596 (its items and
    persistent grid), :628 (fastw), :600 (INZ = the input is tile-swizzled);
  * conv1ab_wino24p.hip:390-396 (conv1ab_wino24p_preferred: at least two tile pairs per CU), :400-407 (its grid);
  * conv3x3_wino24h.hip:185 and conv3x3_wino24.hip:224 (the same fastw rule, evaluated in the kernel), :361-369 / :381-391 (items,
    two workgroups per CU); conv1ab_wino24h.hip:261-267;
  * conv3x3.hip:24, :244-245 (the direct kernel: 8 x 32-pixel tiles, one workgroup per tile, every store masked).

The *_supported predicates (conv3x3_wino24.hip:420, conv3x3_wino24h.hip:380, conv3x3_wino24p.hip:610, conv1ab_wino24h.hip:255) are
channel counts the network always meets, weights the synthetic state dict meets (tests/test_gpu_superpoint.py asserts the fp16 forms
ran) and a 2 GB limit per image far above these shapes: restated as true.

FASTW: `W % 16 == 0 and (not out_blocked or H % 8 == 0)` on the layer's OWN input size -- the unmasked store path of the three
Winograd kernels (a template parameter of the pair kernel, a kernel-uniform branch of the other two).  The fused first layer and the
direct kernel mask every store; for them `fastw` says whether every tile is whole, i.e. whether a mask ever clips."""
from collections import namedtuple

OH, OW = 8, 16                  # wino24_h2.h:14
DIRECT_TH, DIRECT_TW = 8, 32    # conv3x3.hip:24
NT, NG, SLICE = 64, 2, 256      # wino24_h2.h:44, :27; imx_superpoint.cpp:22

# name, level, pool, swizzle candidate (imx_superpoint.cpp:14-17), Cout (64-64-64-128-128-128-128-(256 + 256))
LAYERS = (("conv1ab_pool", 0, True, False, 64), ("conv2a", 1, False, True, 64), ("conv2b_pool", 1, True, False, 64),
          ("conv3a", 2, False, True, 128), ("conv3b_pool", 2, True, False, 128), ("conv4a", 3, False, True, 128),
          ("conv4b", 3, False, False, 128), ("convPaDa", 3, False, False, 512))
NAMES = tuple(l[0] for l in LAYERS)
PAIR, TILE, F32, DIRECT = "conv3x3_wino24p:f16x2", "conv3x3_wino24h:f16x2", "conv3x3_wino24:f32", "conv3x3_direct:f32"
PAIR1, TILE1, F321 = "conv1ab_wino24p:f16x2", "conv1ab_wino24h:f16x2", "conv1ab_wino24:f32"

# slice: 0 = the (full) slices of 256 images or the only one, 1 = the short last slice of a batch of more than 256; images: in that
# slice; out: 0 NHWC, 1 channel-blocked, 2 tile-swizzled; items: per workgroup of the persistent grid (the largest); dead: the
# last pair's second tile does not exist
Variant = namedtuple("Variant", "name slice images H W form pool fastw inz out tiles_x tiles_y items dead")


def _ceil(a, b):
    return (a + b - 1) // b


def variants(H, W, B, cu, conv="wino", swizzle=True):
    """One Variant per (slice kind, layer) of a SuperPoint forward on B images of H x W with the default weights: eight for a batch of
    at most 256 images (or any batch outside the fp16 chain, which is not sliced), sixteen beyond."""
    assert conv in ("wino", "wino_h", "wino32", "direct")
    chain = conv in ("wino", "wino_h")                                   # imx_superpoint.cpp:92-103, :167
    nslice = _ceil(B, SLICE) if chain else 1                             # :109
    kinds = [B] if nslice == 1 else [SLICE, B - SLICE * (nslice - 1)]    # :111-115
    out = []
    for si, nb in enumerate(kinds):
        forms = []
        for name, level, pool, swz, cout in LAYERS:
            hh, ww = H >> level, W >> level
            tiles = _ceil(ww, OW) * _ceil(hh, OH) * nb
            if conv == "direct":
                forms.append(DIRECT)
            elif not chain:
                forms.append(F321 if name == "conv1ab_pool" else F32)
            elif name == "conv1ab_pool":
                forms.append(PAIR1 if conv == "wino" and _ceil(tiles, NG) >= 2 * cu else TILE1)     # conv1ab_wino24p.hip:395
            else:
                forms.append(PAIR if conv == "wino" and _ceil(tiles, NG) * (cout // NT) >= cu else TILE)   # conv3x3_wino24p.hip:623
        layout_in = 0
        for li, (name, level, pool, swz, cout) in enumerate(LAYERS):
            hh, ww = H >> level, W >> level
            z = swz and swizzle and forms[li] == PAIR and forms[li + 1] == PAIR                     # imx_superpoint.cpp:121-122
            layout = 2 if z else 1 if conv != "direct" and li + 1 < len(LAYERS) else 0
            ncob = cout // NT
            if forms[li] == DIRECT:
                tx, ty = _ceil(ww, DIRECT_TW), _ceil(hh, DIRECT_TH)
                fastw, items, dead = ww % DIRECT_TW == 0 and hh % DIRECT_TH == 0, 1, False
            else:
                tx, ty = _ceil(ww, OW), _ceil(hh, OH)
                ntiles = tx * ty * nb
                fastw = ww % OW == 0 and (hh % OH == 0 if li == 0 else not layout or hh % OH == 0)
                if forms[li] == PAIR:
                    nitems = _ceil(ntiles, NG) * ncob
                    grid = nitems if nitems <= cu else cu - cu % ncob                               # conv3x3_wino24p.hip:592
                elif forms[li] == PAIR1:
                    nitems = _ceil(ntiles, NG)
                    grid = min(nitems, cu)                                                          # conv1ab_wino24p.hip:407
                else:
                    nitems = ntiles * (1 if li == 0 else ncob)
                    grid = min(nitems, 2 * cu)
                items, dead = _ceil(nitems, grid), forms[li] in (PAIR, PAIR1) and ntiles % 2 == 1
            out.append(Variant(name, si, nb, hh, ww, forms[li], pool, fastw, layout_in == 2, layout, tx, ty, items, dead))
            layout_in = layout
    return out


def report_rows(vs):
    """The (name, form) rows of the timing report that the eight layers of such a forward leave: launch order, one row per name and
    form (imx_api.cpp: imx_timing_report)."""
    rows = []
    for name in NAMES:
        for v in vs:
            if v.name == name and (name, v.form) not in rows:
                rows.append((name, v.form))
    return rows


# ------------------------------------------------------------------------------------------------------------------- the shapes
# Large batches: the pair forms ("conv" = "wino"); every one is held bit for bit to "conv" = "wino_h" and to "conv_swizzle" = "off".
LARGE = ((64, 128, 255), (128, 256, 128), (72, 128, 256), (64, 136, 256), (65, 129, 255), (64, 128, 260))
# Two images: "wino_h", "wino32" and "direct" layer by layer against float64.
SMALL = ((64, 128), (72, 128), (64, 136), (65, 129), (128, 256), (256, 256), (8, 8), (16, 24), (64, 16), (64, 256), (64, 264))
SMALL_B = 2
CU = 256                        # the MI355X; the proof below is stated for it
LEVEL3 = ("conv4a", "conv4b", "convPaDa")
PRODUCERS, CONSUMERS = ("conv2a", "conv3a", "conv4a"), ("conv2b_pool", "conv3b_pool", "conv4b")


def large_cells(H, W, B, cu=CU):
    """The cells of the coverage table that a large-batch case reaches with "conv" = "wino", swizzled and blocked."""
    cells = set()
    on, off = variants(H, W, B, cu, "wino", True), variants(H, W, B, cu, "wino", False)
    for v in on:
        if v.form == PAIR and v.name in PRODUCERS and v.out == 2:
            cells.add(("pair", v.name, "swizzled out", "FASTW", int(v.fastw)))
        if v.form == PAIR and v.name in CONSUMERS and v.inz:
            cells.add(("pair", v.name, "INZ", "FASTW", int(v.fastw)))
        if v.form == PAIR and v.name == "convPaDa":
            cells.add(("pair", v.name, "FASTW", int(v.fastw)) + (("H % 8 == 0", v.H % 8 == 0) if v.fastw else ()))
        if v.form == PAIR and v.tiles_x == v.tiles_y == 1:
            cells.add(("pair", "one tile per image"))
        if v.form == PAIR and v.dead:
            cells.add(("pair", "dead tile in the last pair"))
        if v.form == PAIR and v.name in LEVEL3 and v.items > 1:
            cells.add(("pair", "level 3, more than one item per workgroup"))
        if v.form == PAIR1:
            cells.add(("pair", v.name, "whole tiles", int(v.fastw)))
    for v in off:
        if v.form == PAIR and v.name in PRODUCERS + CONSUMERS:
            assert v.out == 1 and not v.inz
            cells.add(("pair", v.name, "blocked in and out", "FASTW", int(v.fastw)))
    # what the rows of the shape table claim beyond single cells: the conjunctions that make each case its own
    first = [v for v in on if v.slice == 0]
    if all(v.form in (PAIR, PAIR1) and v.fastw for v in on) and any(v.dead and v.name in LEVEL3 for v in on):
        cells.add(("case", "every layer a pair with FASTW = 1, and a dead tile at level 3"))
    if first[0].form == PAIR1 and not first[0].fastw and all(v.fastw for v in first[1:]):
        cells.add(("case", "partial tiles in the first layer, whole tiles after its pool (the round-3 class)"))
    if all(v.form == PAIR and not v.fastw and v.W % OW == 0 for v in first[1:7]) and first[7].fastw:
        cells.add(("case", "H partial and W whole at every level"))
    if all(v.form == PAIR and v.W % OW and v.H % OH == 0 for v in first[1:]):
        cells.add(("case", "W partial and H whole at every level"))
    if all(v.fastw for v in on) and all(v.tiles_x > 1 and v.tiles_y > 1 and v.items > 1 for v in on if v.name in ("conv4a", "conv4b")):
        cells.add(("case", "whole tiles, several tile rows and columns per image at level 3, two items per workgroup on conv4a and conv4b"))
    if len(on) == 16 and on[5].out == 2 and on[13].out == 1 and on[13].form == TILE:
        cells.add(("case", "two slices: a4a swizzled in the first, blocked in the second"))
    return cells


def small_cells(H, W, cu=CU):
    """The cells a two-image case reaches with "conv" = "wino_h", "wino32" and "direct"."""
    cells = set()
    for conv in ("wino_h", "wino32", "direct"):
        vs = variants(H, W, SMALL_B, cu, conv)
        for v in vs:
            cells.add((conv, v.name, "FASTW", int(v.fastw)))
            if conv == "direct" and v.name in LEVEL3:
                cells.add((conv, "level 3", "narrower than" if v.W < DIRECT_TW else f"{v.W} wide" if v.W <= DIRECT_TW + 1 else "wider than", "the 32-column tile"))
            if conv == "direct":
                if v.name in LEVEL3 and v.fastw and v.tiles_x == v.tiles_y == 1:
                    cells.add((conv, "level 3 is exactly one whole 8 x 32 tile"))
                continue
            if v.H == v.W == 1:
                cells.add((conv, "a level of a single pixel"))
            if v.name in LEVEL3 and v.H < OH and v.W < OW and v.H * v.W > 1:
                cells.add((conv, "level 3 smaller than one tile on both axes, more than a pixel"))
            if v.name in LEVEL3 and v.W < 4 and v.H == OH:
                cells.add((conv, "level 3 narrower than one 2 x 4 output block, H a whole tile"))
            if v.items > 1:
                cells.add((conv, "more than one item per workgroup of the tile form"))
            if v.name == "conv1ab_pool" and v.tiles_x * v.tiles_y * SMALL_B == 2 * cu:
                cells.add((conv, "exactly two items per CU: the boundary of the grid's cap"))
            if v.name == "convPaDa" and v.fastw and v.H % OH:
                cells.add((conv, "convPaDa FASTW = 1 with H % 8 != 0"))
        if conv != "direct":
            if all(v.fastw for v in vs) and vs[-1].tiles_x == vs[-1].tiles_y == 1:
                cells.add((conv, "whole tiles at every layer, level 3 exactly one tile"))
            if not vs[0].fastw and all(v.fastw for v in vs[1:]):
                cells.add((conv, "partial tiles in the first layer, whole tiles after its pool (the round-3 class)"))
    # the tile-per-workgroup form is held to float64 on the very shapes at which the pair form is held to it bit for bit
    if any((H, W) == c[:2] for c in LARGE):
        cells.add(("twin of a large-batch case", H, W))
    return cells


def required_cells():
    """Every cell of the coverage table, at 256 CUs."""
    need = set()
    for name in PRODUCERS:
        need |= {("pair", name, "swizzled out", "FASTW", f) for f in (0, 1)} | {("pair", name, "blocked in and out", "FASTW", f) for f in (0, 1)}
    for name in CONSUMERS:
        need |= {("pair", name, "INZ", "FASTW", f) for f in (0, 1)} | {("pair", name, "blocked in and out", "FASTW", f) for f in (0, 1)}
    need |= {("pair", "convPaDa", "FASTW", 0), ("pair", "convPaDa", "FASTW", 1, "H % 8 == 0", True), ("pair", "convPaDa", "FASTW", 1, "H % 8 == 0", False),
             ("pair", "one tile per image"), ("pair", "dead tile in the last pair"), ("pair", "level 3, more than one item per workgroup"),
             ("pair", "conv1ab_pool", "whole tiles", 0), ("pair", "conv1ab_pool", "whole tiles", 1)}
    for conv in ("wino_h", "wino32", "direct"):
        need |= {(conv, name, "FASTW", f) for name in NAMES for f in (0, 1)}
    need |= {("direct", "level 3", w, "the 32-column tile") for w in ("narrower than", "32 wide", "33 wide")}
    need |= {("twin of a large-batch case", H, W) for H, W, _ in LARGE}
    # beyond the single cells: what makes each case of the lists its own (the conjunctions of its row, the small shapes' edges)
    need |= {("case", c) for c in ("every layer a pair with FASTW = 1, and a dead tile at level 3",
                                   "whole tiles, several tile rows and columns per image at level 3, two items per workgroup on conv4a and conv4b",
                                   "H partial and W whole at every level", "W partial and H whole at every level",
                                   "partial tiles in the first layer, whole tiles after its pool (the round-3 class)",
                                   "two slices: a4a swizzled in the first, blocked in the second")}
    for conv in ("wino_h", "wino32"):
        need |= {(conv, c) for c in ("whole tiles at every layer, level 3 exactly one tile", "convPaDa FASTW = 1 with H % 8 != 0",
                                     "partial tiles in the first layer, whole tiles after its pool (the round-3 class)",
                                     "exactly two items per CU: the boundary of the grid's cap", "more than one item per workgroup of the tile form",
                                     "a level of a single pixel", "level 3 smaller than one tile on both axes, more than a pixel",
                                     "level 3 narrower than one 2 x 4 output block, H a whole tile")}
    need.add(("direct", "level 3 is exactly one whole 8 x 32 tile"))
    return need


def image_order(B):
    """Which of the 16 distinct images sits in batch slot i: not periodic in 2 or 16, so the two tiles of a pair and neighbouring
    items belong to different images."""
    return [(7 * i + i // 16) % 16 for i in range(B)]
