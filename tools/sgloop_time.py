#!/usr/bin/env python
"""Times what libimx_sgloop.so and SuperGlue's training loop add, on the GPU.  HIP events on the stream, a warm-up, then the median of
`--batches` (at least 20) calls, the variants alternating inside one process; every row runs in a child process of its own under a time
limit.

  ot B,N,T          on a (B, N, N) score matrix at T Sinkhorn iterations: the fused call Engine.ot_match_loss_grad_matches (`fused`), the
                    match loss alone, Engine.ot_match_loss_grad (`plain`: fused - plain is the increment), and the parent commit's way to
                    the same outputs, ot_match_loss_grad + sgtrain_model.transport + mutual_matches, a second Sinkhorn in PyTorch
                    (`parent`); the three extraction kernels' own times from the library's events beside the streaming bound of their bytes
                    (8 B N N, the matrix read twice) at 6.29 TB/s
  step 1,N,T        one whole SuperGlueTrainable step (forward, backward, optimiser) at d = 256, 18 layers, T iterations, N keypoints on
                    a side, a model each: want_matches False / "loss" / True with optim.FlatAdam, and "loss" with torch.optim.Adam
  train B,N,T       iterations per second of SuperGlueTrainer.train() on synthetic 240 x 320 images at batch B, N keypoints at most, the
                    script's default network (d = 128, 18 layers, T iterations): dataset batches, the step, one checkpoint per
                    epoch (wall clock between synchronisations, two repeats)

A record, not a gate.  Needs a GPU.  Prints one JSON line (kept as profiles/sgloop_time.json)."""
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

ROWS = (("ot", 1, 1024, 30), ("ot", 1, 1024, 100), ("ot", 8, 1024, 30), ("ot", 8, 1024, 100), ("step", 1, 1024, 100), ("train", 1, 256, 30),
        ("train", 4, 256, 30))
LIMIT_S = 240
STREAM_BYTES_PER_S = 6.29e12


def ot_row(B, N, T, batches):
    import numpy as np
    import torch
    from image_matching_amd import sgtrain_model
    from tests import otgrad_ref as O
    eng = engine()
    s, mt = O.case_scores(1, N, N)
    scores = torch.from_numpy(np.repeat(s[None], B, 0)).cuda().contiguous()
    am = torch.from_numpy(np.repeat(mt[None], B, 0)).cuda().contiguous()
    n_all = torch.full((B,), mt.shape[1], dtype=torch.int32, device="cuda")
    alpha = torch.ones(1, device="cuda")
    fused = lambda: eng.ot_match_loss_grad_matches(scores, alpha, am, n_all, T, threshold=0.2)
    plain = lambda: eng.ot_match_loss_grad(scores, alpha, am, n_all, T)

    def parent():
        res = eng.ot_match_loss_grad(scores, alpha, am, n_all, T)
        with torch.no_grad():
            return res, sgtrain_model.mutual_matches(sgtrain_model.transport(scores, alpha, T), 0.2)

    row = events_ms({"fused": fused, "plain": plain, "parent": parent, "fused_repeat": fused}, batches)
    row["increment_ms"] = round(row["fused"]["median_ms"] - row["plain"]["median_ms"], 4)
    row["parent_over_fused"] = round(row["parent"]["median_ms"] / row["fused"]["median_ms"], 3)
    row["fused_repeat_spread_ms"] = round(abs(row["fused"]["median_ms"] - row["fused_repeat"]["median_ms"]), 4)
    row["kernels_ms"], _ = kernel_rows(eng, "sgl_", fused, batches)
    row["kernels_sum_ms"] = round(sum(row["kernels_ms"].values()), 4)
    row["stream_bound_ms"] = round(8.0 * B * N * N / STREAM_BYTES_PER_S * 1e3, 6)
    return eng, row


def step_row(B, N, T, batches):
    import torch
    from image_matching_amd.optim import FlatAdam
    from image_matching_amd.sgtrain_model import SuperGlueTrainable
    from tests import scoregrad_ref as R
    eng = engine()
    config = {"descriptor_dim": 256, "keypoint_encoder": [32, 64, 128, 256], "GNN_layers": ["self", "cross"] * 9, "sinkhorn_iterations": T,
              "match_threshold": 0.2}
    data = {k: torch.from_numpy(v).cuda() for k, v in R.model_case(3, N0=N, N1=N, H=480, W=640, planted=N // 2, d=256).items()}
    variants = {"flat_false": (False, "flat"), "flat_loss": ("loss", "flat"), "flat_true": (True, "flat"), "torch_loss": ("loss", "torch")}
    models, opts = {}, {}
    for name, (_, kind) in variants.items():
        torch.manual_seed(0)
        models[name] = SuperGlueTrainable(config, eng).train()
        opts[name] = FlatAdam(models[name].parameters(), eng, lr=1e-4) if kind == "flat" else torch.optim.Adam(models[name].parameters(), lr=1e-4)

    def step(name):
        want, kind = variants[name]

        def run():
            if kind == "torch":
                opts[name].zero_grad()
            models[name](data, want_matches=want)["loss"].backward()
            opts[name].step()
        return run

    fns = {name: step(name) for name in variants}
    fns["flat_loss_repeat"] = step("flat_loss")
    row = events_ms(fns, batches)
    base = row["flat_false"]["median_ms"]
    row["loss_over_false"] = round(row["flat_loss"]["median_ms"] / base, 4)
    row["true_over_false"] = round(row["flat_true"]["median_ms"] / base, 4)
    row["flat_over_torch"] = round(row["flat_loss"]["median_ms"] / row["torch_loss"]["median_ms"], 4)
    row["flat_loss_repeat_spread_ms"] = round(abs(row["flat_loss"]["median_ms"] - row["flat_loss_repeat"]["median_ms"]), 4)
    row["parameters"] = sum(p.numel() for p in models["flat_false"].parameters())
    return eng, row


def train_row(B, N, T, batches):
    import torch
    from image_matching_amd.superglue.train_loop import SuperGlueTrainer
    from superglue_export_pairs import SyntheticPairs
    images = 4 * B
    epochs = max(1, batches // 4)
    row = {"images": images, "batches_per_epoch": images // B, "epochs_timed": epochs}
    eng = None
    for rep in range(2):
        ds = SyntheticPairs(images, {"weights": None, "descriptor_dim": 128, "nms_radius": 4, "keypoint_threshold": 0.005, "max_keypoints": N},
                            [320, 240], torch.device("cuda:0"))
        eng = ds._engine()
        with tempfile.TemporaryDirectory() as tmp:
            t = SuperGlueTrainer({"descriptor_dim": 128, "keypoint_encoder": [32, 64, 128], "sinkhorn_iterations": T, "match_threshold": 0.2}, ds, eng,
                                 optimizer="flat", lr=1e-4, batch_size=B, seed=rep, result_dir=tmp, log_interval=5)
            t.train(1)                                                   # warm-up: allocations, workspaces
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t.train(1 + epochs)
            torch.cuda.synchronize()
            row.setdefault("it_per_s", []).append(round(epochs * (images // B) / (time.perf_counter() - t0), 3))
    return eng, row


def child(kind, B, N, T, batches):
    import torch
    torch.set_grad_enabled(True)
    eng, row = {"ot": ot_row, "step": step_row, "train": train_row}[kind](B, N, T, batches)
    print(json.dumps({"row": kind, "B": B, "N": N, "T": T, "build": eng.lib.imx_version().decode(), "device": torch.cuda.get_device_name(0), **row}))


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
    out = json.dumps({"tool": "sgloop_time",
                      "timing": "HIP events on the stream, median of the batches after a warm-up, the variants alternating; one child process per row.  "
                                "ot: the fused loss-and-matches call against the match loss alone (the increment) and against the parent's way "
                                "(a second Sinkhorn in PyTorch), the extraction kernels beside the streaming bound of their bytes; step: one whole "
                                "training step at d = 256, 18 layers, with want_matches False / 'loss' / True and FlatAdam, and 'loss' with "
                                "torch.optim.Adam; train: iterations per second of train() (wall clock between synchronisations, two repeats)",
                      "rows": rows, "note": note})
    print(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(out + "\n")
    return 0 if note is None else 1


if __name__ == "__main__":
    sys.exit(main())
