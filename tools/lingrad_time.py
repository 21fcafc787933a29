#!/usr/bin/env python
"""Times the 1x1 convolutions of SuperGlue's GNN in their training form (include/imx_train.h) on the GPU at B in {1, 8} times
(Cout, C0, C1, N) in {(128, 128, 0, 1024), (256, 128, 128, 1024), (512, 256, 256, 2048)}.  HIP events on the stream, a warm-up, then the
median of `--batches` (at least 20) batches, the variants alternating inside one process.  Per shape, each with the peak of torch's
allocator above what was allocated before:

  forward          imx_conv1x1_forward_train
  backward         imx_conv1x1_backward (dx0, dx1, dw, db)
  bridge           sgtrain_grad.conv1d forward plus backward() under torch.autograd: the two calls and autograd's bookkeeping
  torch_autograd   PyTorch-ROCm F.conv1d on torch.cat([x0, x1], 1), forward plus backward(), in the same process
  kernels_ms       the four kernels alone, from imx_timing_report (events around each launch), and their workgroup counts

and one more row for a whole layer of the GNN at d = 128, N = M = 1024, B = 1 in train mode: sgtrain_grad.attentional_propagation against
the all-PyTorch layer (tests/lingrad_ref.py: AttentionalPropagation), forward plus backward(), time and allocator peak.

Every row runs in a child process of its own under a time limit; a child that fails ends the run.  The parent never touches the
GPU.  A record, not a gate.  Needs a GPU.  Prints one JSON line (kept as profiles/lingrad_time.json)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.mhagrad_time import events_ms   # noqa: E402  (the same measurement)

SHAPES = tuple((B,) + s for s in ((128, 128, 0, 1024), (256, 128, 128, 1024), (512, 256, 256, 2048)) for B in (1, 8))
LAYER = (1, 128, 4, 1024)
LIMIT_S = 120


def child(B, Cout, C0, C1, N, batches):
    import torch
    from image_matching_amd import sgtrain_grad
    from image_matching_amd.engine import Engine
    from tests import lingrad_ref as R
    from tests import util
    torch.set_grad_enabled(True)
    eng = Engine(util.sp_config(128, 256), util.sg_config(128), "cuda")
    x0, x1, w, bias, dy = (None if a is None else torch.from_numpy(a).cuda() for a in R.case(1, B, Cout, C0, C1, N))
    w = w[:, :, None].contiguous()                              # the (Cout, Cin, 1) parameter

    def autograd_of(conv):
        def run():
            leaves = [None if t is None else t.detach().requires_grad_(True) for t in (x0, x1, w, bias)]
            conv(*leaves).backward(dy)
            return [t.grad for t in leaves if t is not None]
        return run

    bridge = autograd_of(lambda a, a1, ww, bb: sgtrain_grad.conv1d(eng, a, ww, bb, x1=a1))
    torch_autograd = autograd_of(lambda a, a1, ww, bb: torch.nn.functional.conv1d(a if a1 is None else torch.cat([a, a1], 1), ww, bb))
    row = events_ms({"forward": lambda: eng.conv1x1_forward_train(x0, w, bias, x1=x1),
                     "backward": lambda: eng.conv1x1_backward(x0, w, dy, x1=x1),
                     "bridge": bridge, "torch_autograd": torch_autograd}, batches)
    Cin, tiles = C0 + C1, lambda n: -(-n // 64)
    row["backward"]["workspace_bytes"] = 4 * B * -(-N // 256) * Cout * (Cin + 1)   # lin.part, from the size the host unit requests
    row["torch_over_bridge"] = round(row["torch_autograd"]["median_ms"] / row["bridge"]["median_ms"], 3)
    row["max_abs_diff_to_torch"] = max(float((a - b).abs().max()) for a, b in zip(bridge(), torch_autograd()))
    eng.set_timing(True)
    eng.timing_reset()
    for _ in range(batches):
        eng.conv1x1_forward_train(x0, w, bias, x1=x1)
        eng.conv1x1_backward(x0, w, dy, x1=x1)
    torch.cuda.synchronize()
    row["kernels_ms"] = {r[0]: round(r[2] / r[1], 4) for r in eng.timing_report() if r[0].startswith("lin_")}
    row["workgroups"] = {"lin_fwd": tiles(N) * tiles(Cout) * B, "lin_dx": tiles(N) * tiles(Cin) * B,
                         "lin_dw": tiles(Cin + 1) * tiles(Cout) * -(-N // 256) * B, "lin_dw_reduce": -(-(Cin + 1) // 256) * Cout}
    eng.set_timing(False)
    print(json.dumps({"B": B, "Cout": Cout, "C0": C0, "C1": C1, "N": N, "build": eng.lib.imx_version().decode(),
                      "device": torch.cuda.get_device_name(0), **row}))


def child_layer(B, d, heads, N, batches):
    import torch
    from image_matching_amd import sgtrain_grad
    from image_matching_amd.engine import Engine
    from tests import lingrad_ref as R
    from tests import util
    torch.set_grad_enabled(True)
    eng = Engine(util.sp_config(d, 256), util.sg_config(d), "cuda")
    layer = R.AttentionalPropagation(d, heads).train()
    layer.load_state_dict({k: torch.from_numpy(v) for k, v in R.layer_parameters(1, layer).items()}, strict=False)
    layer = layer.cuda()
    x, source, dy = (torch.from_numpy(a).cuda().expand(B, -1, -1).contiguous() for a in R.layer_case(1, d, N, N))
    ours = lambda: R.layer_grads(layer, lambda a, b: sgtrain_grad.attentional_propagation(eng, layer, a, b), x, source, dy)
    theirs = lambda: R.layer_grads(layer, layer, x, source, dy)
    row = events_ms({"attentional_propagation": ours, "torch_layer": theirs}, batches)
    row["torch_over_ours"] = round(row["torch_layer"]["median_ms"] / row["attentional_propagation"]["median_ms"], 3)
    a, b = ours(), theirs()
    row["max_abs_diff_to_torch"] = max(float((a[k] - b[k]).abs().max()) for k in a)
    print(json.dumps({"B": B, "d": d, "heads": heads, "N": N, "M": N, "build": eng.lib.imx_version().decode(),
                      "device": torch.cuda.get_device_name(0), **row}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--child", default=None, help="B,Cout,C0,C1,N: time one shape in this process")
    ap.add_argument("--child-layer", default=None, help="B,d,heads,N: time one layer in this process")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    a = ap.parse_args()
    batches = max(a.batches, 20)
    if a.child:
        return child(*(int(v) for v in a.child.split(",")), batches)
    if a.child_layer:
        return child_layer(*(int(v) for v in a.child_layer.split(",")), batches)
    rows, layer, note = [], None, None
    for flag, shape in [("--child", s) for s in SHAPES] + [("--child-layer", LAYER)]:
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
            layer = res
    out = json.dumps({"tool": "lingrad_time",
                      "timing": "HIP events on the stream, median of the batches after a warm-up, the variants alternating; one child process per row.  "
                                "forward / backward: the two library calls through Engine (output tensors allocated per call).  bridge and torch_autograd: "
                                "forward plus backward() under torch.autograd, fresh leaves per batch.  torch_peak_bytes_above_baseline: the peak of torch's "
                                "allocator over one call above what was allocated before it; workspace_bytes: the library's lin.part scratch beside it, "
                                "computed, not measured.  layer: one AttentionalPropagation in train mode, forward plus backward() into all parameters",
                      "shapes": rows, "layer": layer, "note": note})
    print(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(out + "\n")
    return 0 if note is None else 1


if __name__ == "__main__":
    sys.exit(main())
