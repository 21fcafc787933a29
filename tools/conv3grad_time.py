#!/usr/bin/env python
"""Times the 3x3 convolutions of SuperPoint's network in their training form (include/imx_spnet.h) on the GPU at the layer shapes of the
reference's network (superpoint_train.py:15-27): Cin -> Cout at a fraction of the image size,

    1 -> 64 and 64 -> 64 at 1/1, 64 -> 64 at 1/2, 64 -> 128 and 128 -> 128 at 1/4, 128 -> 128 and 128 -> 256 at 1/8,

for 480 x 640 images with B = 2 and B = 16 and for 240 x 320 images with B = 16.  HIP events on the stream, a warm-up, then the median of
`--batches` (at least 20) batches, the variants alternating inside one process.  Per shape, each with the peak of torch's allocator above
what was allocated before:

  forward          imx_conv3x3_forward_train
  backward         imx_conv3x3_backward (dx, dw, db; without dx at Cin = 1: the image needs no gradient)
  bridge           sptrain_net.conv2d forward plus backward() under torch.autograd
  torch_autograd   PyTorch-ROCm F.conv2d, forward plus backward(), in the same process on the same device
  kernels_ms       the four kernels alone, from imx_timing_report (events around each launch), with the TFLOP/s of the three products
                   (2 B Cout Cin 9 H W flop each) beside the 157 TFLOP/s fp32-matrix peak

and one more row for one double_conv(64, 64) block at 240 x 320, B = 16, in train mode: sptrain_net.double_conv against the all-PyTorch
block (tests/conv3grad_ref.py: DoubleConv), forward plus backward(), time and allocator peak, and per tensor how far the two sides lie from
each other and from the same block in float64 on the device.

Every row runs in a child process of its own under a time limit; a child that fails ends the run.  The parent never touches the GPU.  A
record, not a gate.  Needs a GPU.  Prints one JSON line (kept as profiles/conv3grad_time.json)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.mhagrad_time import events_ms   # noqa: E402  (the same measurement)

LAYERS = ((1, 64, 1), (64, 64, 1), (64, 64, 2), (64, 128, 4), (128, 128, 4), (128, 128, 8), (128, 256, 8))      # Cin, Cout, 1 / scale
IMAGES = ((2, 480, 640), (16, 480, 640), (16, 240, 320))                                                         # B, H, W
SHAPES = tuple((B, Cout, Cin, H // s, W // s) for B, H, W in IMAGES for Cin, Cout, s in LAYERS)
BLOCK = (16, 64, 240, 320)
PEAK_TFLOPS = 157.0
LIMIT_S = 150


def child(B, Cout, Cin, H, W, batches):
    import torch
    from image_matching_amd import sptrain_net
    from image_matching_amd.engine import Engine
    from tests import util
    torch.set_grad_enabled(True)
    eng = Engine(util.sp_config(128, 256), util.sg_config(128), "cuda")
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(B, Cin, H, W, device="cuda", generator=gen)
    w = torch.randn(Cout, Cin, 3, 3, device="cuda", generator=gen) / (9 * Cin) ** 0.5
    bias = 0.1 * torch.randn(Cout, device="cuda", generator=gen)
    dy = torch.randn(B, Cout, H, W, device="cuda", generator=gen)
    first = Cin == 1
    want = (not first, True, True)

    def autograd_of(conv):
        def run():
            leaves = [x.detach().requires_grad_(not first), w.detach().requires_grad_(True), bias.detach().requires_grad_(True)]
            conv(*leaves).backward(dy)
            return [t.grad for t in leaves if t.grad is not None]
        return run

    bridge = autograd_of(lambda a, ww, bb: sptrain_net.conv2d(eng, a, ww, bb))
    torch_autograd = autograd_of(lambda a, ww, bb: torch.nn.functional.conv2d(a, ww, bb, padding=1))
    row = events_ms({"forward": lambda: eng.conv3x3_forward_train(x, w, bias), "backward": lambda: eng.conv3x3_backward(x, w, dy, want=want),
                     "bridge": bridge, "torch_autograd": torch_autograd}, batches)
    row["backward"]["workspace_bytes"] = 4 * B * -(-H // 16) * Cout * (9 * Cin + 1)   # conv3.part, from the size the host unit requests
    row["torch_over_bridge"] = round(row["torch_autograd"]["median_ms"] / row["bridge"]["median_ms"], 3)
    row["max_abs_diff_to_torch"] = max(float((a - b).abs().max()) for a, b in zip(bridge(), torch_autograd()))
    eng.set_timing(True)
    eng.timing_reset()
    for _ in range(batches):
        eng.conv3x3_forward_train(x, w, bias)
        eng.conv3x3_backward(x, w, dy, want=want)
    torch.cuda.synchronize()
    row["kernels_ms"] = {r[0]: round(r[2] / r[1], 4) for r in eng.timing_report() if r[0].startswith("conv3_")}
    flop = 2.0 * B * Cout * Cin * 9 * H * W
    row["kernels_tflops"] = {k: round(flop / (ms * 1e-3) / 1e12, 2) for k, ms in row["kernels_ms"].items() if k != "conv3_dw_reduce" and ms > 0}
    row["peak_tflops_fp32_matrix"] = PEAK_TFLOPS
    eng.set_timing(False)
    print(json.dumps({"B": B, "Cout": Cout, "Cin": Cin, "H": H, "W": W, "build": eng.lib.imx_version().decode(),
                      "device": torch.cuda.get_device_name(0), **row}))


def child_block(B, C, H, W, batches):
    import torch
    from image_matching_amd import sptrain_net
    from image_matching_amd.engine import Engine
    from tests import conv3grad_ref as R
    from tests import util
    torch.set_grad_enabled(True)
    eng = Engine(util.sp_config(128, 256), util.sg_config(128), "cuda")
    block = R.load_block(R.DoubleConv(C, C), 1).train().cuda()
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(B, C, H, W, device="cuda", generator=gen)
    dy = torch.randn(B, C, H, W, device="cuda", generator=gen)
    ours = lambda: R.block_grads(block, lambda a: sptrain_net.double_conv(eng, block, a), x, dy)
    theirs = lambda: R.block_grads(block, block, x, dy)
    row = events_ms({"double_conv": ours, "torch_block": theirs}, batches)
    row["torch_over_ours"] = round(row["torch_block"]["median_ms"] / row["double_conv"]["median_ms"], 3)
    a, b = ours(), theirs()
    # per tensor: the largest |ours - PyTorch's|, the same over the largest |PyTorch's|, and how many elements differ by more than 1e-3 of
    # that largest value: a ReLU whose pre-activation rounds to the other side of 0 moves single elements of dx by a whole dy, while
    # the output and the parameter gradients (sums over 1.2e6 pixels) move in their low bits only
    row["diff_to_torch"] = {k: {"max_abs": float((a[k] - b[k]).abs().max()), "max_abs_over_max_value": float((a[k] - b[k]).abs().max() / b[k].abs().max()),
                                "elements_beyond_1e-3_of_max_value": int(((a[k] - b[k]).abs() > 1e-3 * b[k].abs().max()).sum()), "elements": a[k].numel()}
                            for k in a}
    row["max_abs_diff_to_torch"] = max(v["max_abs"] for v in row["diff_to_torch"].values())
    row["max_abs_diff_tensor"] = max(row["diff_to_torch"], key=lambda k: row["diff_to_torch"][k]["max_abs"])
    # both sides against the same block in float64 on the device: largest |value - float64| over the largest |float64|, per tensor
    block64 = R.load_block(R.DoubleConv(C, C), 1, torch.float64).train().cuda()
    ref = R.block_grads(block64, block64, x.double(), dy.double())
    row["error_to_float64_over_max_value"] = {k: {"double_conv": float((a[k].double() - ref[k]).abs().max() / ref[k].abs().max()),
                                                  "torch_block": float((b[k].double() - ref[k]).abs().max() / ref[k].abs().max())} for k in a}
    print(json.dumps({"B": B, "C": C, "H": H, "W": W, "build": eng.lib.imx_version().decode(), "device": torch.cuda.get_device_name(0), **row}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--child", default=None, help="B,Cout,Cin,H,W: time one shape in this process")
    ap.add_argument("--child-block", default=None, help="B,C,H,W: time one double_conv(C, C) block in this process")
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
        print(f"[conv3grad_time] {what} done", file=sys.stderr, flush=True)
        if flag == "--child":
            rows.append(res)
        else:
            block = res
    out = json.dumps({"tool": "conv3grad_time",
                      "timing": "HIP events on the stream, median of the batches after a warm-up, the variants alternating; one child process per row.  "
                                "forward / backward: the two library calls through Engine (output tensors allocated per call).  bridge and torch_autograd: "
                                "forward plus backward() under torch.autograd, fresh leaves per batch; at Cin = 1 the input asks for no gradient in either.  "
                                "torch_peak_bytes_above_baseline: the peak of torch's allocator over one call above what was allocated before it; "
                                "workspace_bytes: the library's conv3.part scratch beside it, computed, not measured.  kernels_tflops: 2 B Cout Cin 9 H W "
                                "flop over the kernel's time.  block: one double_conv(64, 64) in train mode, forward plus backward() into all parameters",
                      "shapes": rows, "block": block, "note": note})
    print(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(out + "\n")
    return 0 if note is None else 1


if __name__ == "__main__":
    sys.exit(main())
