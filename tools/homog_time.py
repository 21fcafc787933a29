#!/usr/bin/env python
"""Times the RANSAC homography fit of libimx_homog.so and what a validation epoch adds to SuperGlue's training, on the GPU.  HIP events
on the stream, a warm-up, then the median of `--batches` (at least 20) calls, the variants alternating inside one process; every row
runs in a child process of its own under a time limit.

  fit B,N,H         Engine.estimate_homography on B pairs of N matched points each (a planted warp, 0.5 px noise, every seventh match an
                    outlier), H hypotheses, 3 refinement steps: the whole call (`fit`, and `fit_repeat` for the spread), the kernel's own
                    time from the library's events, and Engine.homography_corner_error on the result (`corner_error`)
  val B,N,T         one validation pass over 4 B synthetic 240 x 320 images in batches of B (SuperGlueTrainer.validate: dataset batches,
                    the eval forward, the fit, the corner error, one read-back) against one training epoch over as many images at the
                    same batch size, N keypoints at most, the script's default network (d = 128, 18 layers, T iterations): wall clock
                    between synchronisations, the median of the repeats, and the share validation / epoch

A record, not a gate.  Needs a GPU.  Prints one JSON line (kept as profiles/homog_time.json)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.mhagrad_time import events_ms   # noqa: E402  (the same measurement)
from tools.sppool_time import engine, kernel_rows   # noqa: E402

ROWS = (("fit", 1, 1024, 512), ("fit", 64, 1024, 512), ("val", 4, 256, 30))
LIMIT_S = 240


def fit_row(B, N, hyp, batches):
    import numpy as np
    import torch
    from tests import homography_ref as R
    eng = engine()
    case = R.planted_case(1, 1, N, N, (N,), noise=0.5, unmatched_every=N + 1)         # every slot matched: N matched points
    k0, k1, m = (torch.from_numpy(np.repeat(case[k], B, 0)).cuda().contiguous() for k in ("kpts0", "kpts1", "matches0"))
    gt = torch.from_numpy(np.repeat(case["H_gt"], B, 0)).cuda()
    fit = lambda: eng.estimate_homography(k0, k1, m, hypotheses=hyp)
    Hm, _, ninl, _ = fit()
    row = events_ms({"fit": fit, "corner_error": lambda: eng.homography_corner_error(Hm, gt, (480, 640)), "fit_repeat": fit}, batches)
    row["fit_repeat_spread_ms"] = round(abs(row["fit"]["median_ms"] - row["fit_repeat"]["median_ms"]), 4)
    row["kernels_ms"], _ = kernel_rows(eng, "homog_", fit, batches)
    row["matched_points"], row["inliers"] = int((m[0] >= 0).sum()), int(ninl[0])
    return eng, row


def val_row(B, N, T, batches):
    import numpy as np
    import torch
    from image_matching_amd.superglue.train_loop import SuperGlueTrainer
    from superglue_export_pairs import SyntheticPairs
    images, repeats = 4 * B, max(3, batches // 4)
    sp = {"weights": None, "descriptor_dim": 128, "nms_radius": 4, "keypoint_threshold": 0.005, "max_keypoints": N}
    ds = SyntheticPairs(images, sp, [320, 240], torch.device("cuda:0"))
    val = SyntheticPairs(images, sp, [320, 240], torch.device("cuda:0"), first=images, superpoint=ds.superpoint)
    eng = ds._engine()
    row = {"images": images, "batches": images // B, "repeats": repeats}
    with tempfile.TemporaryDirectory() as tmp:
        t = SuperGlueTrainer({"descriptor_dim": 128, "keypoint_encoder": [32, 64, 128], "sinkhorn_iterations": T, "match_threshold": 0.2}, ds, eng,
                             optimizer="flat", lr=1e-4, batch_size=B, seed=0, result_dir=tmp, log_interval=5, val_dataset=val,
                             val_interval=1 << 30)                       # (train() itself never validates here)
        t.train(1)                                                       # warm-up: allocations, workspaces
        t.validate(0)
        epoch_s, val_s = [], []
        for r in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t.train(2 + r)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            t.validate(2 + r)
            torch.cuda.synchronize()
            epoch_s.append(t1 - t0)
            val_s.append(time.perf_counter() - t1)
    row["epoch_ms"], row["validation_ms"] = round(float(np.median(epoch_s)) * 1e3, 3), round(float(np.median(val_s)) * 1e3, 3)
    row["validation_over_epoch"] = round(row["validation_ms"] / row["epoch_ms"], 4)
    row["last_validation"] = {k: (v if np.isfinite(v) else str(v)) for k, v in t.last_validation.items()}
    return eng, row


def child(kind, B, N, T, batches):
    import torch
    torch.set_grad_enabled(True)
    eng, row = {"fit": fit_row, "val": val_row}[kind](B, N, T, batches)
    key = "hypotheses" if kind == "fit" else "T"
    print(json.dumps({"row": kind, "B": B, "N": N, key: T, "build": eng.lib.imx_version().decode(), "device": torch.cuda.get_device_name(0), **row}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--child", default=None, metavar="KIND,B,N,T", help="time one row in this process")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    a = ap.parse_args()
    batches = max(a.batches, 20)
    if a.child:
        kind, *shape = a.child.split(",")
        return child(kind, *(int(v) for v in shape), batches)
    rows, note = [], None
    for shape in ROWS:
        what = ",".join(map(str, shape))
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, "--batches", str(batches)],
                               capture_output=True, text=True, timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            note = f"{what}: no result within {LIMIT_S} s; the run ends here"
            break
        if p.returncode != 0:
            note = f"{what}: exit status {p.returncode}; the run ends here: {p.stderr[-400:]}"
            break
        rows.append(json.loads(p.stdout.strip().splitlines()[-1]))
        print(f"{what}: done", file=sys.stderr, flush=True)
    out = json.dumps({"tool": "homog_time",
                      "timing": "fit: HIP events on the stream, median of the batches after a warm-up, the variants alternating; the kernel's own "
                                "time from the library's events.  val: wall clock between synchronisations of one validation pass and of one "
                                "training epoch over as many images, the median of the repeats.  One child process per row",
                      "rows": rows, "note": note})
    print(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(out + "\n")
    return 0 if note is None else 1


if __name__ == "__main__":
    sys.exit(main())
