#!/usr/bin/env python
"""Times BatchNorm2d + ReLU of SuperPoint's network in its training form on the GPU at the (B, C, H x W) of SuperPoint's training shapes:
B in {16, 2} times C = 64 at 480 x 640, 240 x 320, 120 x 160; C = 128 at 120 x 160, 60 x 80; C = 256 and C = 65 at 60 x 80.  Training
mode.  HIP events on the stream, a warm-up, then the median of `--batches` (at least 20) batches, the variants alternating inside one
process.  Per shape, each with the peak of torch's allocator above what was allocated before:

  forward          imx_bn2d_forward_train (running statistics updated)
  backward         imx_bn2d_backward (dx, dgamma, dbeta)
  pixels           sptrain_net.batchnorm2d(relu=True) forward plus backward() under torch.autograd: libimx_spnorm, the work split over pixels
  channel          sgtrain_grad.bn_relu on the (B, C, H W) view, forward plus backward(): libimx_train, one workgroup per channel
  channel_repeat   the same again in the same alternation: the spread between two repeats of one variant
  torch_autograd   PyTorch-ROCm F.relu(bn(x)), forward plus backward(), in the same process
  kernels_ms       every kernel of the pixels form alone, from imx_timing_report (events around each launch), beside stream_bound_ms:
                   the bytes the kernel needs (stats x; apply x, y; bwd_sums x, dy; bwd_dx x, dy, dx) at 6.29 TB/s

and one more row for the reference's double_conv(64, 64) block at (16, 64, 240, 320) in train mode, forward plus backward() into the
input and all parameters: sptrain_net.double_conv_form with form="channel" and form="pixels", and the all-PyTorch block.

Every row runs in a child process of its own under a time limit; a child that fails ends the run.  The parent never touches the GPU.
A record, not a gate.  Needs a GPU.  Prints one JSON line (kept as profiles/bn2d_time.json)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.mhagrad_time import events_ms   # noqa: E402  (the same measurement)

MAPS = ((64, 480, 640), (64, 240, 320), (64, 120, 160), (128, 120, 160), (128, 60, 80), (256, 60, 80), (65, 60, 80))
SHAPES = tuple((B, C, H, W) for B in (16, 2) for C, H, W in MAPS)
BLOCK = (16, 64, 240, 320)
LIMIT_S = 180
STREAM_BYTES_PER_S = 6.29e12
# floats a kernel moves per element of x
MOVES = {"bn2d_stats": 1, "bn2d_apply": 2, "bn2d_bwd_sums": 2, "bn2d_bwd_dx": 3}


def seeded(shape, seed):
    import torch
    return torch.randn(*shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))


def child(B, C, H, W, batches):
    import torch
    from image_matching_amd import sgtrain_grad, sptrain_net
    from image_matching_amd.engine import Engine
    from tests import util
    torch.set_grad_enabled(True)
    eng = Engine(util.sp_config(128, 256), util.sg_config(128), "cuda")
    x, dy = seeded((B, C, H, W), 1), seeded((B, C, H, W), 2)
    gamma, beta = 1 + 0.1 * seeded((C,), 3), 0.1 * seeded((C,), 4)
    bn = torch.nn.BatchNorm2d(C).cuda().train()
    bn.load_state_dict({"weight": gamma, "bias": beta}, strict=False)
    stats = eng.bn2d_forward_train(x, gamma, beta)

    def autograd_of(fn):
        def run():
            bn.zero_grad()
            leaf = x.detach().requires_grad_(True)
            fn(leaf).backward(dy)
            return [leaf.grad, bn.weight.grad, bn.bias.grad]
        return run

    def channel_form(t):
        y = sgtrain_grad.bn_relu.apply(eng, t.view(B, C, H * W), bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, None,
                                       True, 0.1, 1e-5)
        return y.view(B, C, H, W)

    pixels = autograd_of(lambda t: sptrain_net.batchnorm2d(eng, bn, t, relu=True))
    channel = autograd_of(channel_form)
    torch_autograd = autograd_of(lambda t: torch.relu(bn(t)))
    row = events_ms({"forward": lambda: eng.bn2d_forward_train(x, gamma, beta, bn.running_mean, bn.running_var, bn.num_batches_tracked),
                     "backward": lambda: eng.bn2d_backward(x, gamma, beta, stats["mean"], stats["rstd"], dy),
                     "pixels": pixels, "channel": channel, "channel_repeat": channel, "torch_autograd": torch_autograd}, batches)
    row["channel_over_pixels"] = round(row["channel"]["median_ms"] / row["pixels"]["median_ms"], 3)
    row["torch_over_pixels"] = round(row["torch_autograd"]["median_ms"] / row["pixels"]["median_ms"], 3)
    row["channel_repeat_spread_ms"] = round(abs(row["channel"]["median_ms"] - row["channel_repeat"]["median_ms"]), 4)
    row["max_abs_diff_to_torch"] = max(float((a - b).abs().max()) for a, b in zip(pixels(), torch_autograd()))
    eng.set_timing(True)
    eng.timing_reset()
    for _ in range(batches):
        eng.bn2d_forward_train(x, gamma, beta, bn.running_mean, bn.running_var, bn.num_batches_tracked)
        eng.bn2d_backward(x, gamma, beta, stats["mean"], stats["rstd"], dy)
    torch.cuda.synchronize()
    report = [r for r in eng.timing_report(forms=True) if r[0].startswith("bn2d_")]
    row["kernels_ms"] = {r[0]: round(r[2] / r[1], 4) for r in report}
    row["stream_bound_ms"] = {k: round(m * 4 * B * C * H * W / STREAM_BYTES_PER_S * 1e3, 5) for k, m in MOVES.items()}
    row["form"] = sorted({r[3] for r in report if r[3]})          # what the library reports: 'x4' or 'x1'
    row["workgroups"] = B * C * ((H * W + 4095) // 4096)
    eng.set_timing(False)
    print(json.dumps({"B": B, "C": C, "H": H, "W": W, "build": eng.lib.imx_version().decode(), "device": torch.cuda.get_device_name(0), **row}))


def child_block(B, C, H, W, batches):
    import torch
    from image_matching_amd import sptrain_net
    from image_matching_amd.engine import Engine
    from tests import conv3grad_ref as R
    from tests import util
    torch.set_grad_enabled(True)
    eng = Engine(util.sp_config(128, 256), util.sg_config(128), "cuda")
    block = R.DoubleConv(C, C).cuda().train()
    x, dy = seeded((B, C, H, W), 1), seeded((B, C, H, W), 2)
    run = lambda fn: (lambda: R.block_grads(block, fn, x, dy))
    row = events_ms({"channel": run(lambda a: sptrain_net.double_conv_form(eng, block, a, form="channel")),
                     "pixels": run(lambda a: sptrain_net.double_conv_form(eng, block, a, form="pixels")),
                     "channel_repeat": run(lambda a: sptrain_net.double_conv_form(eng, block, a, form="channel")),
                     "torch_block": run(block)}, batches)
    row["channel_over_pixels"] = round(row["channel"]["median_ms"] / row["pixels"]["median_ms"], 3)
    row["torch_over_pixels"] = round(row["torch_block"]["median_ms"] / row["pixels"]["median_ms"], 3)
    print(json.dumps({"block": "double_conv", "B": B, "C": C, "H": H, "W": W, "build": eng.lib.imx_version().decode(),
                      "device": torch.cuda.get_device_name(0), **row}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--child", default=None, help="B,C,H,W: time one shape in this process")
    ap.add_argument("--child-block", default=None, help="B,C,H,W: time one double_conv(C, C) in this process")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    a = ap.parse_args()
    batches = max(a.batches, 20)
    if a.child:
        return child(*(int(v) for v in a.child.split(",")), batches)
    if a.child_block:
        return child_block(*(int(v) for v in a.child_block.split(",")), batches)
    rows, block, note = [], None, None
    for flag, shape in [("--child", s) for s in SHAPES] + [("--child-block", BLOCK)]:
        what = f"{flag[2:]} {','.join(map(str, shape))}"
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), flag, ",".join(map(str, shape)), "--batches", str(batches)],
                               capture_output=True, text=True, timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            note = f"{what}: no result within {LIMIT_S} s; the run ends here"
            break
        if p.returncode != 0:
            note = f"{what}: exit status {p.returncode}; the run ends here: {p.stderr[-400:]}"
            break
        res = json.loads(p.stdout.strip().splitlines()[-1])
        if flag == "--child":
            rows.append(res)
        else:
            block = res
        print(f"{what}: done", file=sys.stderr, flush=True)
    out = json.dumps({"tool": "bn2d_time",
                      "timing": "HIP events on the stream, median of the batches after a warm-up, the variants alternating; one child process per row.  "
                                "forward / backward: the two library calls through Engine (output tensors allocated per call).  pixels, channel and "
                                "torch_autograd: forward plus backward() under torch.autograd in training mode, a fresh leaf per batch; channel_repeat is "
                                "channel once more in the same alternation.  torch_peak_bytes_above_baseline: the peak of torch's allocator over one call "
                                "above what was allocated before it; the library's scratch (bn2d.part) is not in it.  kernels_ms beside stream_bound_ms: "
                                "the bytes the kernel needs at 6.29 TB/s.  block: the reference's double_conv(64, 64) in train mode, forward plus "
                                "backward() into the input and all parameters",
                      "shapes": rows, "block": block, "note": note})
    print(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(out + "\n")
    return 0 if note is None else 1


if __name__ == "__main__":
    sys.exit(main())
