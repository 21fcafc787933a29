#!/usr/bin/env python
"""Times the score product of SuperGlue's training step (include/imx_sgtrain.h) on the GPU at (B, D, N0 = N1) in {1, 8} x {(256, 1024),
(256, 2048)} and (1, 64, 512).  HIP events on the stream, a warm-up, then the median of `--batches` (at least 20) batches, the variants
alternating inside one process.  Per shape, each with the peak of torch's allocator above what was allocated before:

  forward          imx_score_product_forward_train
  backward         imx_score_product_backward (da, db)
  bridge           sgtrain_grad.scores forward plus backward() under torch.autograd: the two calls and autograd's bookkeeping
  torch_autograd   PyTorch-ROCm torch.einsum('bdn,bdm->bnm') / D ** .5, forward plus backward(), in the same process
  kernels_ms       the three kernels alone, from imx_timing_report (events around each launch), and their workgroup counts

and one more row for a whole training step -- forward, loss.backward() into all parameters -- of sgtrain_model.SuperGlueTrainable against
the all-PyTorch restated model (tests/scoregrad_ref.py: SuperGlue) at d = 256, the keypoint encoder [32, 64, 128, 256], 18 layers, 100
Sinkhorn iterations and 1024 keypoints on both sides, B = 1, train mode: time and allocator peak.

Every row runs in a child process of its own under a time limit; a child that fails ends the run.  The parent never touches the GPU.
A record, not a gate.  Needs a GPU.  Prints one JSON line (kept as profiles/scoregrad_time.json)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.mhagrad_time import events_ms   # noqa: E402  (the same measurement)

SHAPES = ((1, 64, 512), (1, 256, 1024), (8, 256, 1024), (1, 256, 2048), (8, 256, 2048))
STEP = (256, 18, 100, 1024)                # descriptor_dim, GNN layers, Sinkhorn iterations, keypoints per side
LIMIT_S = 180


def child(B, D, N, batches):
    import torch
    from image_matching_amd import sgtrain_grad
    from image_matching_amd.engine import Engine
    from tests import scoregrad_ref as R
    from tests import util
    torch.set_grad_enabled(True)
    eng = Engine(util.sp_config(128, 256), util.sg_config(128), "cuda")
    a, b, ds = (torch.from_numpy(t).cuda() for t in R.case(1, B, D, N, N))

    def autograd_of(fn):
        def run():
            leaves = [t.detach().requires_grad_(True) for t in (a, b)]
            fn(*leaves).backward(ds)
            return [t.grad for t in leaves]
        return run

    bridge = autograd_of(lambda x, y: sgtrain_grad.scores(eng, x, y))
    torch_autograd = autograd_of(R.score_einsum)
    row = events_ms({"forward": lambda: eng.score_product_forward_train(a, b), "backward": lambda: eng.score_product_backward(a, b, ds),
                     "bridge": bridge, "torch_autograd": torch_autograd}, batches)
    row["torch_over_bridge"] = round(row["torch_autograd"]["median_ms"] / row["bridge"]["median_ms"], 3)
    row["max_abs_diff_to_torch"] = max(float((x - y).abs().max()) for x, y in zip(bridge(), torch_autograd()))
    eng.set_timing(True)
    eng.timing_reset()
    for _ in range(batches):
        eng.score_product_forward_train(a, b)
        eng.score_product_backward(a, b, ds)
    torch.cuda.synchronize()
    row["kernels_ms"] = {r[0]: round(r[2] / r[1], 4) for r in eng.timing_report() if r[0].startswith("score_")}
    tiles = lambda n: -(-n // 64)
    row["workgroups"] = {"score_fwd": tiles(N) * tiles(N) * B, "score_da": tiles(N) * tiles(D) * B, "score_db": tiles(N) * tiles(D) * B}
    eng.set_timing(False)
    print(json.dumps({"B": B, "D": D, "N0": N, "N1": N, "build": eng.lib.imx_version().decode(), "device": torch.cuda.get_device_name(0), **row}))


def child_step(d, layers, iters, N, batches):
    import torch
    from image_matching_amd.engine import Engine
    from image_matching_amd.sgtrain_model import SuperGlueTrainable
    from tests import scoregrad_ref as R
    from tests import util
    torch.set_grad_enabled(True)
    config = {"descriptor_dim": d, "keypoint_encoder": [32, 64, 128, 256], "GNN_layers": ["self", "cross"] * (layers // 2), "sinkhorn_iterations": iters}
    eng = Engine(util.sp_config(128, 256), util.sg_config(128), "cuda")
    ours = R.load_parameters(SuperGlueTrainable(config, eng).train(), 1)
    theirs = R.load_parameters(R.SuperGlue(config).train(), 1).cuda()
    case = R.model_case(1, N0=N, N1=N, H=480, W=640, planted=N // 2, d=d)
    data = {k: torch.from_numpy(v).cuda() for k, v in case.items()}
    pair = {k: v.cuda() if isinstance(v, torch.Tensor) else v for k, v in R.as_pair(case, torch.float32).items()}

    def step_ours():
        ours.zero_grad()
        loss = ours(data, want_matches=False)["loss"]
        loss.backward()
        return loss

    def step_theirs():
        theirs.zero_grad()
        loss = theirs([pair])[0][0]
        loss.backward()
        return loss

    row = events_ms({"trainable": step_ours, "torch_model": step_theirs}, batches)
    row["torch_over_ours"] = round(row["torch_model"]["median_ms"] / row["trainable"]["median_ms"], 3)
    row["loss"] = {"trainable": float(step_ours()), "torch_model": float(step_theirs())}
    print(json.dumps({"descriptor_dim": d, "layers": layers, "sinkhorn_iterations": iters, "N0": N, "N1": N, "build": eng.lib.imx_version().decode(),
                      "device": torch.cuda.get_device_name(0), **row}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--child", default=None, help="B,D,N: time one shape in this process")
    ap.add_argument("--child-step", default=None, help="d,layers,iters,N: time one training step in this process")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    a = ap.parse_args()
    batches = max(a.batches, 20)
    if a.child:
        return child(*(int(v) for v in a.child.split(",")), batches)
    if a.child_step:
        return child_step(*(int(v) for v in a.child_step.split(",")), batches)
    rows, step, note = [], None, None
    for flag, shape in [("--child", s) for s in SHAPES] + [("--child-step", STEP)]:
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
            step = res
    out = json.dumps({"tool": "scoregrad_time",
                      "timing": "HIP events on the stream, median of the batches after a warm-up, the variants alternating; one child process per row.  "
                                "forward / backward: the two library calls through Engine (output tensors allocated per call).  bridge and torch_autograd: "
                                "forward plus backward() under torch.autograd, fresh leaves per batch.  torch_peak_bytes_above_baseline: the peak of torch's "
                                "allocator over one call above what was allocated before it.  step: one training step in train mode, forward plus "
                                "backward() into all parameters, no optimiser",
                      "shapes": rows, "step": step, "note": note})
    print(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(out + "\n")
    return 0 if note is None else 1


if __name__ == "__main__":
    sys.exit(main())
