#!/usr/bin/env python
"""Times what libimx_sploop.so and the training loop add, on the GPU.  HIP events on the stream, a warm-up, then the median of `--batches`
(at least 20) calls, the variants alternating inside one process; every row runs in a child process of its own under a time limit.

  step B,H,W        one SuperPointTrainable step (forward, a synthetic loss, backward, optimiser) with optim.FlatAdam (`flat`), with
                    torch.optim.Adam as it defaults (`adam`) and with torch.optim.Adam(fused=True) (`adam_fused`), a model each; the
                    optimiser call alone on the same models with gradients in place (`*_opt`); imx_adam_flat's own time from the
                    library's events beside the streaming bound of its bytes (32 per element with zero_grad) at 6.29 TB/s
  labels B,H,W      Engine.warp_labels_bi (levels 255) for B images of 300 points beside the same splat as PyTorch ops (`torch_ops`)
  train B,H,W       iterations per second of Train_model_heatmap_loop's train() on the shipped configuration at this shape (dataset
                    batches, both forwards, losses, backward, FlatAdam, validation and checkpoints off), beside the same loop with the
                    optimiser the parent commit had: torch.optim.Adam on a model without arenas, zero_grad() every step (`adam`)

A record, not a gate.  Needs a GPU.  Prints one JSON line (kept as profiles/sploop_time.json)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.mhagrad_time import events_ms   # noqa: E402  (the same measurement)
from tools.sppool_time import engine, kernel_rows   # noqa: E402

ROWS = (("step", 16, 240, 320), ("step", 8, 480, 640), ("labels", 8, 480, 640), ("train", 8, 480, 640))
LIMIT_S = 240
STREAM_BYTES_PER_S = 6.29e12


def step_row(B, H, W, batches):
    import torch
    from image_matching_amd.optim import FlatAdam
    from image_matching_amd.sptrain_model import SuperPointTrainable
    eng = engine()
    x = torch.rand(B, 1, H, W, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    target = 0.1 * torch.randn(B, 128, H // 8, W // 8, device="cuda")
    models, opts = {}, {}
    for name in ("flat", "adam", "adam_fused"):
        torch.manual_seed(0)
        models[name] = SuperPointTrainable(eng, 128).train()
    opts["flat"] = FlatAdam(models["flat"].parameters(), eng, lr=1e-4)
    opts["adam"] = torch.optim.Adam(models["adam"].parameters(), lr=1e-4)
    opts["adam_fused"] = torch.optim.Adam(models["adam_fused"].parameters(), lr=1e-4, fused=True)

    def step(name):
        def run():
            if name != "flat":
                opts[name].zero_grad()
            out = models[name](x)
            loss = (out['semi'] ** 2).mean() + ((out['desc'] - target) ** 2).mean()
            loss.backward()
            opts[name].step()
        return run

    def opt_alone(name):
        def run():
            opts[name].step(zero_grad=False) if name == "flat" else opts[name].step()
        return run

    fns = {name: step(name) for name in models}
    fns["flat_repeat"] = step("flat")
    row = events_ms(fns, batches)
    for name in models:                      # gradients in place for the optimiser-alone rows
        out = models[name](x)
        ((out['semi'] ** 2).mean() + ((out['desc'] - target) ** 2).mean()).backward()
    row.update(events_ms({name + "_opt": opt_alone(name) for name in models}, batches))
    kern, forms = kernel_rows(eng, "adam_flat", opt_alone("flat"), batches)
    n = opts["flat"].numel
    row["adam_flat_kernel_ms"] = kern.get("adam_flat")
    row["adam_flat_form"] = forms
    row["arena_floats"] = n
    row["stream_bound_ms"] = round(n * 32 / STREAM_BYTES_PER_S * 1e3, 6)
    row["flat_over_adam"] = round(row["flat"]["median_ms"] / row["adam"]["median_ms"], 4)
    row["flat_over_adam_fused"] = round(row["flat"]["median_ms"] / row["adam_fused"]["median_ms"], 4)
    row["flat_repeat_spread_ms"] = round(abs(row["flat"]["median_ms"] - row["flat_repeat"]["median_ms"]), 4)
    return eng, row


def torch_splat(pts, counts, mats, H, W):
    """get_labels_bi with the 8-bit round trip as PyTorch ops on the device: B images at once, the last write of index_put_ wins or not
    as the runtime pleases (a time reference, not a parity one)"""
    import torch
    B, K, _ = pts.shape
    p = torch.cat([pts.trunc(), torch.ones(B, K, 1, device=pts.device)], 2) @ mats.transpose(1, 2)
    w = p[..., :2] / p[..., 2:]
    q = w.trunc()
    r = w - q
    ex, ey = 1 - r[..., 0], 1 - r[..., 1]
    cx = torch.stack([q[..., 0], q[..., 0], q[..., 0] + 1, q[..., 0] + 1], 1)
    cy = torch.stack([q[..., 1], q[..., 1] + 1, q[..., 1], q[..., 1] + 1], 1)
    wt = torch.stack([ex * ey, ex * r[..., 1], r[..., 0] * ey, r[..., 0] * r[..., 1]], 1)
    keep = (cx >= 0) & (cx <= W - 1) & (cy >= 0) & (cy <= H - 1) & (torch.arange(K, device=pts.device)[None, None] < counts[:, None, None])
    flat = (torch.arange(B, device=pts.device)[:, None, None] * H + cy.clamp(0, H - 1).long()) * W + cx.clamp(0, W - 1).long()
    out = torch.zeros(B * H * W + 1, device=pts.device)
    out.index_put_((torch.where(keep, flat, torch.full_like(flat, B * H * W)).reshape(-1),), wt.reshape(-1))
    return torch.floor(out[:-1].view(B, H, W) * 255).clamp(0, 255) / 255


def labels_row(B, H, W, batches):
    import numpy as np
    import torch
    from image_matching_amd.homoadapt import sample_homographies
    from tests import sptrain_ref as R
    eng = engine()
    rng = np.random.default_rng(0)
    K = 300
    pts = torch.from_numpy(np.stack([rng.uniform(0, W - 1, (B, K)), rng.uniform(0, H - 1, (B, K))], 2).astype(np.float32)).cuda()
    counts = torch.full((B,), K, dtype=torch.int32, device="cuda")
    mats = torch.from_numpy(np.stack([R.scale_pixels(sample_homographies(2, [0, b], **R.WARPED_PAIR_PARAMS)[0][1], H, W)[0] for b in range(B)])).cuda()
    ours = lambda: eng.warp_labels_bi(pts, counts, mats, H, W, levels=255, pixel_space=True)
    row = events_ms({"ours": ours, "torch_ops": lambda: torch_splat(pts, counts, mats, H, W), "ours_repeat": ours}, batches)
    row["torch_over_ours"] = round(row["torch_ops"]["median_ms"] / row["ours"]["median_ms"], 3)
    row["kernels_ms"], _ = kernel_rows(eng, "warp_labels_bi", ours, batches)
    row["points_per_image"] = K
    return eng, row


def train_row(B, H, W, batches):
    import numpy as np
    import torch
    import yaml
    from image_matching_amd import synth
    from image_matching_amd.datasets.ALLSS_train import ALLSSTrain
    from image_matching_amd.sptrain_model import SuperPointTrainable
    from image_matching_amd.superpoint.Train_model_heatmap_loop import BatchLoader, Train_model_heatmap
    with open(os.path.join(ROOT, "tests", "golden", "superpoint_allss_train_heatmap.yaml")) as f:
        cfg = yaml.safe_load(f)
    iters = batches
    cfg.update(train_iter=iters, validation_interval=10 ** 9, save_interval=10 ** 9, tensorboard_interval=10 ** 9)
    cfg["model"]["batch_size"] = B
    rng = np.random.default_rng(5)
    n = 2 * B
    images = np.stack([synth.synth_pair(i, H, W)[0] for i in range(n)]).astype(np.float32)
    points = [np.stack([rng.uniform(0, W - 1, 300), rng.uniform(0, H - 1, 300)], 1).astype(np.float32) for _ in range(n)]
    data = {k: v for k, v in cfg["data"].items() if k not in ("dataset", "root", "root_split_txt")}

    class TorchAdam:
        """the parent commit's optimiser under the loop's interface: torch.optim.Adam, zero_grad() before every step's backward"""

        def __init__(self, params, lr):
            self.opt = torch.optim.Adam(params, lr=lr, betas=(0.9, 0.999))
            self.opt.zero_grad()

        def step(self):
            self.opt.step()
            self.opt.zero_grad()

        def state_dict(self):
            return self.opt.state_dict()

    def agent_of(kind):
        agent = Train_model_heatmap(cfg, save_path=".", device="cuda")
        agent.train_loader = BatchLoader(ALLSSTrain(task="train", images=images, points=points, **data), B)
        torch.manual_seed(0)
        agent.loadModel()
        if kind == "adam":
            agent.net = SuperPointTrainable(agent.engine, cfg["model"]["descriptor_length"]).train()
            agent.optimizer = TorchAdam(agent.net.parameters(), cfg["model"]["learning_rate"])
        return agent

    row = {}
    for rep in range(2):
        for kind in ("flat", "adam"):
            agent = agent_of(kind)
            agent.max_iter = 2
            agent.train()                                              # warm-up: allocations, workspaces
            agent.max_iter = 2 + iters
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            agent.train()
            torch.cuda.synchronize()
            row.setdefault(kind + "_it_per_s", []).append(round(iters / (time.perf_counter() - t0), 3))
    row["flat_over_adam_it_per_s"] = round(max(row["flat_it_per_s"]) / max(row["adam_it_per_s"]), 4)
    row["iterations"] = iters
    return agent.engine, row


def child(kind, B, H, W, batches):
    import torch
    torch.set_grad_enabled(True)
    eng, row = {"step": step_row, "labels": labels_row, "train": train_row}[kind](B, H, W, batches)
    print(json.dumps({"row": kind, "B": B, "H": H, "W": W, "build": eng.lib.imx_version().decode(), "device": torch.cuda.get_device_name(0), **row}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--child", default=None, metavar="KIND,B,H,W", help="time one row in this process")
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
    out = json.dumps({"tool": "sploop_time",
                      "timing": "HIP events on the stream, median of the batches after a warm-up, the variants alternating; one child process per row.  "
                                "step: one SuperPointTrainable step with FlatAdam / torch.optim.Adam / Adam(fused=True), and the optimiser call "
                                "alone (*_opt); labels: warp_labels_bi against the splat as PyTorch ops; train: iterations per second of train() "
                                "(wall clock between synchronisations, two repeats), FlatAdam against the parent's torch.optim.Adam",
                      "rows": rows, "note": note})
    print(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(out + "\n")
    return 0 if note is None else 1


if __name__ == "__main__":
    sys.exit(main())
