#!/usr/bin/env python
"""Times the photometric augmentation (libimx_photo.so) on the GPU for both images of a training batch of 16: 32 images at 240 x 320 and
at 480 x 640, with the shipped kernel_size_range (100-150) and additive_shade's default (250-350).  HIP events on the stream, a warm-up,
then the median of `--batches` (at least 20) batches, the variants alternating inside one process.

  kernels_ms        each kernel alone: the median over the batches of imx_timing_report's time between the events around its launch,
                    beside stream_bound_ms, the bytes the kernel needs at 6.29 TB/s (photo_pixels 4 + 1 per pixel, shade_mask 1,
                    shade_rows 1 + 4, shade_cols 4 + 1 + 4)
  ours              the whole Engine.photometric call: the uploads of the parameter arrays and both library calls
  ours_repeat       the same again in the same alternation: the spread between two repeats of one variant
  torch_ops         the same stages restated as PyTorch-ROCm ops on the device (quantise, table gather, randn / rand noise, conv2d under
                    reflect padding for the 3x3 and the two Gaussian passes, a broadcast ellipse test), parameters already on the device
  step              one SuperPointTrainable step (forward, backward, Adam) on 16 images of the same size, in the same alternation;
                    share_of_step = ours / step

Every row runs in a child process of its own under a time limit; a child that fails ends the run.  The parent never touches the GPU.
A record, not a gate.  Needs a GPU.  Prints one JSON line (kept as profiles/photometric_time.json)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.mhagrad_time import events_ms   # noqa: E402  (the same measurement)
from tools.sppool_time import engine, kernel_rows   # noqa: E402

ROWS = ((16, 240, 320, 100, 150), (16, 240, 320, 250, 350), (16, 480, 640, 100, 150), (16, 480, 640, 250, 350))
LIMIT_S = 300
STREAM_BYTES_PER_S = 6.29e12
BYTES_PER_PIXEL = {"photo_pixels": 5, "shade_mask": 1, "shade_rows": 5, "shade_cols": 9}


def config(k_lo, k_hi):
    return {'primitives': 'all',
            'params': {'random_brightness': {'max_abs_change': 50}, 'random_contrast': {'strength_range': [0.5, 1.5]},
                       'additive_gaussian_noise': {'stddev_range': [0, 10]}, 'additive_speckle_noise': {'prob_range': [0, 0.0035]},
                       'additive_shade': {'transparency_range': [-0.5, 0.5], 'kernel_size_range': [k_lo, k_hi]},
                       'motion_blur': {'max_kernel_size': 3}}}


def torch_restatement(x, p):
    """the stages of Engine.photometric as PyTorch ops; p: the parameter arrays as device tensors (ksize: a host list)"""
    import torch
    import torch.nn.functional as F
    B, H, W = x.shape
    q = (x * 255).clamp(0, 255).to(torch.int64)
    a = torch.gather(p['lut'].float(), 1, q.view(B, -1)).view(B, H, W)
    a = (a + torch.round(p['noise_scale'].view(B, 1, 1) * torch.randn_like(x))).clamp(0, 255)
    hit = torch.rand_like(x) < p['thresh'].view(B, 1, 1).float() / 2 ** 24
    a = torch.where(hit, p['table'].float()[torch.randint(0, 256, (B, H, W), device=x.device)], a)
    blurred = F.conv2d(F.pad(a[None], (1, 1, 1, 1), mode='reflect'), p['blur_kernel'].view(B, 1, 3, 3), groups=B)[0]
    a = torch.where(p['blur_on'].view(B, 1, 1) != 0, torch.round(blurred).clamp(0, 255), a)
    e = p['ellipses'].double()
    yy, xx = torch.meshgrid(torch.arange(H, device=x.device, dtype=torch.float64), torch.arange(W, device=x.device, dtype=torch.float64), indexing='ij')
    t = torch.pi * e[..., 4] / 180
    cs, sn = torch.cos(t)[..., None, None], torch.sin(t)[..., None, None]
    dx, dy = xx - e[..., 0, None, None], yy - e[..., 1, None, None]
    inside = ((dx * cs + dy * sn) / e[..., 2, None, None]) ** 2 + ((dy * cs - dx * sn) / e[..., 3, None, None]) ** 2 <= 1
    m = inside.any(1).float() * 255
    out = []
    for b in range(B):          # ksize differs per image: one pair of 1-D convolutions each
        k = int(p['ksize'][b])
        taps = p['taps'][b, :k]
        mb = F.conv2d(F.pad(m[b][None, None], (k // 2, k // 2, 0, 0), mode='reflect'), taps.view(1, 1, 1, k))
        mb = F.conv2d(F.pad(mb, (0, 0, k // 2, k // 2), mode='reflect'), taps.view(1, 1, k, 1))[0, 0]
        out.append(((a[b] * (1 - p['transparency'][b] * mb / 255)).clamp(0, 255) / 255))
    return torch.stack(out)[:, None]


def child(B, H, W, k_lo, k_hi, batches):
    import numpy as np
    import torch
    from image_matching_amd import photometric
    from image_matching_amd.sptrain_model import SuperPointTrainable
    torch.set_grad_enabled(True)
    eng = engine()
    n = 2 * B
    x = torch.rand(n, 1, H, W, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    params = photometric.sample_params(config(k_lo, k_hi), [(i, w) for i in range(B) for w in (0, 1)], 0, (H, W))
    on_dev = {k: (v if k == 'ksize' else torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).cuda()) for k, v in params.items()}
    torch.manual_seed(0)
    model = SuperPointTrainable(eng).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    target = 0.1 * torch.randn(B, 256, H // 8, W // 8, device="cuda")

    def step():
        opt.zero_grad()
        out = model(x[:B])
        loss = (out['semi'] ** 2).mean() + ((out['desc'] - target) ** 2).mean()
        loss.backward()
        opt.step()
        return loss

    ours = lambda: eng.photometric(x, params)
    row = events_ms({"ours": ours, "torch_ops": lambda: torch_restatement(x[:, 0], on_dev), "ours_repeat": ours, "step": step}, batches)
    row["torch_over_ours"] = round(row["torch_ops"]["median_ms"] / row["ours"]["median_ms"], 3)
    row["ours_repeat_spread_ms"] = round(abs(row["ours"]["median_ms"] - row["ours_repeat"]["median_ms"]), 4)
    row["share_of_step"] = round(row["ours"]["median_ms"] / row["step"]["median_ms"], 4)
    row["kernels_ms"], row["form"] = kernel_rows(eng, "", ours, batches)
    row["kernels_ms"] = {k: v for k, v in row["kernels_ms"].items() if k in BYTES_PER_PIXEL}
    row["stream_bound_ms"] = {k: round(v * n * H * W / STREAM_BYTES_PER_S * 1e3, 5) for k, v in BYTES_PER_PIXEL.items()}
    row["times_stream_bound"] = {k: round(v / row["stream_bound_ms"][k], 2) for k, v in row["kernels_ms"].items()}
    print(json.dumps({"images": n, "H": H, "W": W, "kernel_size_range": [k_lo, k_hi], "ksize_drawn": [int(params['ksize'].min()), int(params['ksize'].max())],
                      "build": eng.lib.imx_version().decode(), "device": torch.cuda.get_device_name(0), **row}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--child", default=None, metavar="B,H,W,KLO,KHI", help="time one row in this process")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    a = ap.parse_args()
    batches = max(a.batches, 20)
    if a.child:
        return child(*(int(v) for v in a.child.split(",")), batches)
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
    out = json.dumps({"tool": "photometric_time",
                      "timing": "HIP events on the stream, median of the batches after a warm-up, the variants alternating; one child process per row.  "
                                "ours: the whole Engine.photometric call on both images of a batch of 16 (32 images), parameter uploads included; "
                                "torch_ops: the same stages as PyTorch-ROCm ops, parameters already on the device; step: one SuperPointTrainable step "
                                "on 16 images of the same size; kernels_ms beside stream_bound_ms: the bytes the kernel needs at 6.29 TB/s",
                      "rows": rows, "note": note})
    print(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(out + "\n")
    return 0 if note is None else 1


if __name__ == "__main__":
    sys.exit(main())
