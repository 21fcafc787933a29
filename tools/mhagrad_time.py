#!/usr/bin/env python
"""Times the attention of SuperGlue's GNN in its training form (include/imx_train.h) on the GPU at (B, D, H, N = M) = (1, 32, 4, 1024),
(8, 32, 4, 1024) and (1, 64, 4, 2048).  HIP events on the stream, a warm-up, then the median of `--batches` (at least 20) batches, the
variants alternating inside one process.  Per shape, each with the peak of torch's allocator above what was allocated before:

  forward          imx_mha_forward_train (out and lse)
  backward         imx_mha_backward (dq, dk, dv) from the forward's out and lse
  backward_over_forward   their ratio (7 products per tile pair against the forward's 2, and two walks instead of one)
  bridge           sgtrain_grad.attention forward plus backward() under torch.autograd: the two calls and autograd's bookkeeping
  torch_autograd   PyTorch-ROCm autograd of the restated attention (tests/mhagrad_ref.py: attention_einsum), forward plus backward()
  kernels_ms       the four kernels alone, from imx_timing_report (events around each launch), and their workgroup counts
  inference_attention_per_layer   for scale: the inference path's attention launch (both sides of B pairs in one launch, so twice the
                   queries) from imx_timing_report over one SuperGlue forward at the same keypoint count and descriptor dimension

Every shape runs in a child process of its own under a time limit; a child that fails ends the run.  The parent never touches the
GPU.  A record, not a gate.  Needs a GPU.  Prints one JSON line (kept as profiles/mhagrad_time.json)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((1, 32, 4, 1024), (8, 32, 4, 1024), (1, 64, 4, 2048))
LIMIT_S = 240


def events_ms(fns, batches, warmup=2):
    import numpy as np
    import torch
    peak = {}
    for k, f in fns.items():
        for _ in range(warmup):
            f()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        f()
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated() - base
    times = {k: [] for k in fns}
    for _ in range(batches):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    return {k: {"median_ms": round(float(np.median(t)), 4), "min_ms": round(min(t), 4), "batches": len(t), "torch_peak_bytes_above_baseline": int(peak[k])}
            for k, t in times.items()}


def child(B, D, H, N, batches):
    import numpy as np
    import torch
    from image_matching_amd import _lib as L
    from image_matching_amd import sgtrain_grad
    from image_matching_amd.engine import Engine
    from tests import mhagrad_ref as R
    from tests import util
    torch.set_grad_enabled(True)
    d = D * H
    eng = Engine(util.sp_config(d, N), util.sg_config(d), "cuda")
    q, k, v, dout = (torch.from_numpy(a).cuda() for a in R.case(1, B, D, H, N, N))
    fwd = eng.mha_forward_train(q, k, v)

    def autograd_of(attention):
        def run():
            leaves = [t.detach().requires_grad_(True) for t in (q, k, v)]
            attention(*leaves)[0].backward(dout)
            return [t.grad for t in leaves]
        return run

    bridge = autograd_of(lambda a, b, c: sgtrain_grad.attention(eng, a, b, c))
    torch_autograd = autograd_of(R.attention_einsum)
    row = events_ms({"forward": lambda: eng.mha_forward_train(q, k, v),
                     "backward": lambda: eng.mha_backward(q, k, v, fwd["out"], fwd["lse"], dout),
                     "bridge": bridge, "torch_autograd": torch_autograd}, batches)
    row["backward"]["workspace_bytes"] = 4 * B * H * N          # mha.delta, from the size the host unit requests (before the workspace's rounding)
    row["backward_over_forward"] = round(row["backward"]["median_ms"] / row["forward"]["median_ms"], 3)
    row["torch_over_bridge"] = round(row["torch_autograd"]["median_ms"] / row["bridge"]["median_ms"], 3)
    row["max_abs_diff_to_torch"] = max(float((a - b).abs().max()) for a, b in zip(bridge(), torch_autograd()))
    # the kernels alone (imx_timing_report: HIP events around each launch, no Python between them), the mean of `batches` calls
    eng.set_timing(True)
    eng.timing_reset()
    for _ in range(batches):
        eng.mha_forward_train(q, k, v)
        eng.mha_backward(q, k, v, fwd["out"], fwd["lse"], dout)
    torch.cuda.synchronize()
    row["kernels_ms"] = {r[0]: round(r[2] / r[1], 4) for r in eng.timing_report() if r[0].startswith("mha_")}
    row["workgroups"] = {"mha_fwd": -(-N // 128) * B * H, "mha_dkdv": -(-N // 128) * B * H, "mha_dq": -(-N // 128) * B * H}
    eng.set_timing(False)
    eng.timing_reset()
    try:                                                        # for scale only: the inference attention on the same keypoint count
        eng.load_state_dict(L.NET_SUPERGLUE, util.sg_sd(d))
        rng = np.random.default_rng(0)
        kp = torch.from_numpy((rng.random((B, N, 2)) * np.array([639.0, 479.0])).astype(np.float32)).cuda()
        sc = torch.from_numpy(rng.random((B, N)).astype(np.float32)).cuda()
        de = torch.nn.functional.normalize(torch.from_numpy(rng.standard_normal((B, d, N)).astype(np.float32)), dim=1).cuda()
        shp = (B, 1, 480, 640)
        eng.superglue(kp, sc, de, shp, kp, sc, de, shp)
        eng.set_timing(True)
        eng.timing_reset()
        for _ in range(3):
            eng.superglue(kp, sc, de, shp, kp, sc, de, shp)
        torch.cuda.synchronize()
        att = [r for r in eng.timing_report(forms=True) if r[0] == "attention"]
        eng.set_timing(False)
        row["inference_attention_per_layer"] = {"ms": round(sum(r[2] for r in att) / sum(r[1] for r in att), 4), "form": att[0][3],
                                                "queries_per_launch": 2 * B * N}
    except Exception as e:                                      # noqa: BLE001  (a record: the row says what happened)
        row["inference_attention_per_layer"] = f"not measured: {type(e).__name__}: {e}"
    print(json.dumps({"B": B, "D": D, "H": H, "N": N, "M": N, "build": eng.lib.imx_version().decode(), "device": torch.cuda.get_device_name(0), **row}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--child", default=None, help="B,D,H,N: time one shape in this process")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    a = ap.parse_args()
    batches = max(a.batches, 20)
    if a.child:
        return child(*(int(v) for v in a.child.split(",")), batches)
    rows, note = [], None
    for B, D, H, N in SHAPES:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", f"{B},{D},{H},{N}", "--batches", str(batches)],
                               capture_output=True, text=True, timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            note = f"B={B} D={D} H={H} N={N}: no result within {LIMIT_S} s; the run ends here"
            break
        if p.returncode != 0:
            note = f"B={B} D={D} H={H} N={N}: exit status {p.returncode}; the run ends here: {p.stderr[-400:]}"
            break
        rows.append(json.loads(p.stdout.strip().splitlines()[-1]))
    out = json.dumps({"tool": "mhagrad_time",
                      "timing": "HIP events on the stream, median of the batches after a warm-up, the variants alternating; one child process per shape.  "
                                "forward / backward: the two library calls through Engine (output tensors allocated per call).  bridge and torch_autograd: "
                                "forward plus backward() under torch.autograd, fresh leaves per batch.  torch_peak_bytes_above_baseline: the peak of torch's "
                                "allocator over one call above what was allocated before it (q, k, v, dout and the forward's results are before it); "
                                "workspace_bytes: the library's mha.delta scratch beside it, computed, not measured.  inference_attention_per_layer: one "
                                "launch of the inference path covers both sides, twice the queries of the training rows",
                      "shapes": rows, "note": note})
    print(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(out + "\n")
    return 0 if note is None else 1


if __name__ == "__main__":
    sys.exit(main())
