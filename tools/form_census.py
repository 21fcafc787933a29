#!/usr/bin/env python
"""Census of the kernel forms: for each configuration below, one forward with timing on; the ordered (name, form, launches) rows of
timing_report(forms=True), a CRC32 of every output tensor's bytes, and the device's CU count (several forms are chosen by it).
The configurations are the smallest shapes of the suite at which each form decision of sg_forward / sp_detect flips.

    python tools/form_census.py --out tests/golden/form_census.json

tests/test_gpu_form_census.py holds every configuration to the committed file: a change of the host code that is meant to leave the
launches alone (a refactor of the planners) must reproduce it byte for byte."""
import argparse
import json
import os
import sys
import zlib

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from image_matching_amd import synth  # noqa: E402
from tests import util  # noqa: E402
from tests.test_gpu_padding import CASES, H as SG_H, W as SG_W, make_inputs, sg_weights  # noqa: E402

B17 = "throughput_d128_b17_auto"
DENSE = (123, 165, 40, 700)             # H, W, images, image seed: the pair form, swizzled

# id -> (kind, weight set, options, arguments)
CONFIGS = {f"sg/{k}": ("superglue", "default", c[5], k) for k, c in CASES.items()}
CONFIGS.update({
    f"sg/{B17}/qkv_amax_kernel": ("superglue", "default", {"qkv_amax": "kernel"}, B17),
    f"sg/{B17}/heavy": ("superglue", "heavy", {}, B17),
    "sp/123x165_b40": ("dense", "default", {}, DENSE),
    "sp/123x165_b40/conv_swizzle_off": ("dense", "default", {"conv_swizzle": "off"}, DENSE),
    "sp/123x165_b40/conv_wino_h": ("dense", "default", {"conv": "wino_h"}, DENSE),
    "sp/123x165_b40/conv_wino32": ("dense", "default", {"conv": "wino32"}, DENSE),
    "sp/123x165_b40/conv_direct": ("dense", "default", {"conv": "direct"}, DENSE),
    "sp/123x165_b40/mfma_f32": ("dense", "default", {"mfma": "f32"}, DENSE),
    "sp/72x104_b260_two_slices_off": ("dense", "default", {"latency_forms": "off"}, (72, 104, 260, 900)),
    "sp/120x160_b2_tile_form": ("dense", "default", {}, (120, 160, 2, 700)),
    "sp/123x165_b5/heavy": ("dense", "heavy", {}, (123, 165, 5, 700)),
    "sp/homography_adapt_small": ("homoadapt", "default", {}, "homoadapt_small"),
    "mp/200x264_s40-42_k2500_off": ("match_pairs", "default", {"latency_forms": "off"}, (200, 264, (40, 41, 42))),
})

_ENGINES = {}


def cu_count():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _engine(kind, weights, d):
    """One engine per (networks loaded, weight set, width): the configurations set their options on it and restore them."""
    from image_matching_amd import _lib as L
    from image_matching_amd.engine import Engine
    key = ("sp" if kind in ("dense", "homoadapt") else kind, weights, d)
    if key not in _ENGINES:
        heavy = weights == "heavy"
        eng = Engine(util.sp_config(d, 2500 if kind == "match_pairs" else 64), util.sg_config(d), "cuda")
        if kind != "superglue":
            eng.load_state_dict(L.NET_SUPERPOINT, util.to_torch(synth.make_superpoint_state_dict(d, heavy=True)) if heavy else util.sp_sd(d))
        if kind in ("superglue", "match_pairs"):
            eng.load_state_dict(L.NET_SUPERGLUE, util.to_torch(synth.make_superglue_state_dict(d, heavy=True)) if heavy else sg_weights(d))
        _ENGINES[key] = eng
    return _ENGINES[key]


def _images(seed, H, W, B):
    base = [util.pair(seed + i, H, W)[i & 1] for i in range(min(B, 8))]
    return torch.cat([base[i % 8] * (1.0 + (i % 5)) for i in range(B)]).cuda()


def _call(eng, kind, arg):
    """The configuration's forward: {output name: tensor}."""
    if kind == "superglue":
        d, N0, N1, n0, n1 = CASES[arg][:5]
        t = {k: v.cuda() for k, v in make_inputs(d, len(n0), N0, N1, seed=1000 + d + N0 + 7 * len(n0)).items()}
        for side, n in (("0", n0), ("1", n1)):       # zero padding past the counts
            for b, nb in enumerate(n):
                t["keypoints" + side][b, nb:] = 0
                t["scores" + side][b, nb:] = 0
                t["descriptors" + side][b, :, nb:] = 0
        c0, c1 = (torch.tensor(n, dtype=torch.int32, device="cuda") for n in (n0, n1))
        out = eng.superglue(t["keypoints0"], t["scores0"], t["descriptors0"], (1, 1, SG_H, SG_W),
                            t["keypoints1"], t["scores1"], t["descriptors1"], (1, 1, SG_H, SG_W), c0, c1)
        return dict(zip(("matches0", "matches1", "matching_scores0", "matching_scores1"), out))
    if kind == "dense":
        H, W, B, seed = arg
        return dict(zip(("semi", "desc"), eng.superpoint_dense(_images(seed, H, W, B))))
    if kind == "homoadapt":
        from tests.test_homoadapt_host import fixture, image
        g = fixture(arg)
        return dict(zip(("heatmap", "count"), eng.homography_adapt(image(g), torch.from_numpy(g["inv_homographies"]),
                                                                   torch.from_numpy(g["homographies"]), want_count=True)))
    H, W, seeds = arg
    base = [util.pair(s, H, W) for s in seeds]
    return eng.match_pairs(torch.cat([p[0] for p in base]).cuda(), torch.cat([p[1] for p in base]).cuda(), want_desc=True)


def run(name):
    """{"rows": [[name, form, launches], ...] in launch order, "crc32": {output: CRC32 of its bytes}} of one configuration."""
    kind, weights, opts, arg = CONFIGS[name]
    eng = _engine(kind, weights, CASES[arg][0] if kind == "superglue" else 128)
    before = {k: eng.get_option(k) for k in opts}
    try:
        for k, v in opts.items():
            eng.set_option(k, v)
        eng.timing_reset()
        eng.set_timing(True)
        out = _call(eng, kind, arg)
        torch.cuda.synchronize()
        rows = [[r[0], r[3], r[1]] for r in eng.timing_report(forms=True)]
    finally:
        eng.set_timing(False)
        for k, v in before.items():
            eng.set_option(k, v)
    return {"rows": rows, "crc32": {k: zlib.crc32(v.cpu().contiguous().numpy().tobytes()) for k, v in sorted(out.items())}}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    res = {"cu_count": cu_count(), "configs": {}}
    for name in CONFIGS:
        res["configs"][name] = run(name)
        print(name, "ok", flush=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
