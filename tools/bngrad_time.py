#!/usr/bin/env python
"""Times BatchNorm1d + ReLU of SuperGlue's MLPs in their training form (include/imx_train.h) on the GPU at (B, C, N) in
{(1, 256, 1024), (8, 256, 1024), (1, 512, 2048), (8, 512, 2048), (1, 32, 1024)}, training mode.  HIP events on the stream, a warm-up, then
the median of `--batches` (at least 20) batches, the variants alternating inside one process.  Per shape, each with the peak of torch's
allocator above what was allocated before:

  forward          imx_bn_relu_forward_train (running statistics updated)
  backward         imx_bn_relu_backward (dx, dgamma, dbeta)
  bridge           sgtrain_grad.batchnorm_relu forward plus backward() under torch.autograd: the two calls and autograd's bookkeeping
  torch_autograd   PyTorch-ROCm F.relu(F.batch_norm(...)), forward plus backward(), in the same process
  kernels_ms       the two kernels alone, from imx_timing_report (events around each launch), their form and workgroup count, beside
                   stream_bound_ms: the bytes the algorithm needs (forward x and y, backward x, dy and dx) at 6.29 TB/s

and one more row for a whole layer of the GNN at d = 128, N = M = 1024, B = 1 in train mode, forward plus backward() into all parameters,
time and allocator peak: sgtrain_grad.gnn_layer (everything in libimx), sgtrain_grad.attentional_propagation (BatchNorm and ReLU
PyTorch's) and the all-PyTorch layer (tests/lingrad_ref.py: AttentionalPropagation).

Every row runs in a child process of its own under a time limit; a child that fails ends the run.  The parent never touches the
GPU.  A record, not a gate.  Needs a GPU.  Prints one JSON line (kept as profiles/bngrad_time.json)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.mhagrad_time import events_ms   # noqa: E402  (the same measurement)

SHAPES = ((1, 256, 1024), (8, 256, 1024), (1, 512, 2048), (8, 512, 2048), (1, 32, 1024))
LAYER = (1, 128, 4, 1024)
LIMIT_S = 120
STREAM_BYTES_PER_S = 6.29e12


def child(B, C, N, batches):
    import torch
    from image_matching_amd import sgtrain_grad
    from image_matching_amd.engine import Engine
    from tests import bngrad_ref as R
    from tests import util
    torch.set_grad_enabled(True)
    eng = Engine(util.sp_config(128, 256), util.sg_config(128), "cuda")
    x, gamma, beta, dy = (torch.from_numpy(a).cuda() for a in R.case(1, B, C, N))
    bn = torch.nn.BatchNorm1d(C).cuda().train()
    bn.load_state_dict({"weight": gamma, "bias": beta}, strict=False)
    stats = eng.bn_relu_forward_train(x, gamma, beta)

    def autograd_of(fn):
        def run():
            bn.zero_grad()
            leaf = x.detach().requires_grad_(True)
            fn(leaf).backward(dy)
            return [leaf.grad, bn.weight.grad, bn.bias.grad]
        return run

    bridge = autograd_of(lambda t: sgtrain_grad.batchnorm_relu(eng, bn, t))
    torch_autograd = autograd_of(lambda t: torch.relu(bn(t)))
    row = events_ms({"forward": lambda: eng.bn_relu_forward_train(x, gamma, beta, bn.running_mean, bn.running_var, bn.num_batches_tracked),
                     "backward": lambda: eng.bn_relu_backward(x, gamma, beta, stats["mean"], stats["rstd"], dy),
                     "bridge": bridge, "torch_autograd": torch_autograd}, batches)
    row["torch_over_bridge"] = round(row["torch_autograd"]["median_ms"] / row["bridge"]["median_ms"], 3)
    row["max_abs_diff_to_torch"] = max(float((a - b).abs().max()) for a, b in zip(bridge(), torch_autograd()))
    eng.set_timing(True)
    eng.timing_reset()
    for _ in range(batches):
        eng.bn_relu_forward_train(x, gamma, beta, bn.running_mean, bn.running_var, bn.num_batches_tracked)
        eng.bn_relu_backward(x, gamma, beta, stats["mean"], stats["rstd"], dy)
    torch.cuda.synchronize()
    report = [r for r in eng.timing_report(forms=True) if r[0].startswith("bn_relu_")]
    row["kernels_ms"] = {r[0]: round(r[2] / r[1], 4) for r in report}
    row["stream_bound_ms"] = {"bn_relu_fwd": round(2 * 4 * B * C * N / STREAM_BYTES_PER_S * 1e3, 5),
                              "bn_relu_bwd": round(3 * 4 * B * C * N / STREAM_BYTES_PER_S * 1e3, 5)}
    row["form"] = sorted({r[3] for r in report})                 # what the library reports: 'regs' or 'reread'
    row["workgroups"] = C
    eng.set_timing(False)
    print(json.dumps({"B": B, "C": C, "N": N, "build": eng.lib.imx_version().decode(), "device": torch.cuda.get_device_name(0), **row}))


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
    ours = lambda: R.layer_grads(layer, lambda a, b: sgtrain_grad.gnn_layer(eng, layer, a, b), x, source, dy)
    parent = lambda: R.layer_grads(layer, lambda a, b: sgtrain_grad.attentional_propagation(eng, layer, a, b), x, source, dy)
    theirs = lambda: R.layer_grads(layer, layer, x, source, dy)
    row = events_ms({"gnn_layer": ours, "attentional_propagation": parent, "torch_layer": theirs}, batches)
    row["torch_over_gnn_layer"] = round(row["torch_layer"]["median_ms"] / row["gnn_layer"]["median_ms"], 3)
    row["attentional_propagation_over_gnn_layer"] = round(row["attentional_propagation"]["median_ms"] / row["gnn_layer"]["median_ms"], 3)
    a, b = ours(), theirs()
    row["max_abs_diff_to_torch"] = max(float((a[k] - b[k]).abs().max()) for k in a)
    print(json.dumps({"B": B, "d": d, "heads": heads, "N": N, "M": N, "build": eng.lib.imx_version().decode(),
                      "device": torch.cuda.get_device_name(0), **row}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--child", default=None, help="B,C,N: time one shape in this process")
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
    out = json.dumps({"tool": "bngrad_time",
                      "timing": "HIP events on the stream, median of the batches after a warm-up, the variants alternating; one child process per row.  "
                                "forward / backward: the two library calls through Engine (output tensors allocated per call).  bridge and torch_autograd: "
                                "forward plus backward() under torch.autograd in training mode, a fresh leaf per batch.  torch_peak_bytes_above_baseline: the "
                                "peak of torch's allocator over one call above what was allocated before it; the library draws no workspace.  kernels_ms "
                                "beside stream_bound_ms: the bytes the algorithm needs at 6.29 TB/s.  layer: one AttentionalPropagation in train mode, "
                                "forward plus backward() into all parameters",
                      "shapes": rows, "layer": layer, "note": note})
    print(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(out + "\n")
    return 0 if note is None else 1


if __name__ == "__main__":
    sys.exit(main())
