#!/usr/bin/env python
"""Times the SuperGlue match loss through the unrolled Sinkhorn (include/imx_train.h) on the GPU: B in {1, 8} at 1024 x 1024 / T = 30 and
B = 1 at 2048 x 2048 / T = 100.  HIP events on the stream, a warm-up, then the median of `--batches` (at least 20) batches, the
variants alternating inside one process.  Per shape, each with its peak device memory:

  value            imx_ot_match_loss_grad with grad_scores = NULL: the recorded forward and the gather
  value_and_grad   the full call
  grad_over_value  their ratio (four matrix passes per iteration plus the assembly against the forward's two: 2-3 expected)
  torch_backward   PyTorch-ROCm autograd of the same arithmetic: the reference's log_optimal_transport restated here
                   (tests/otgrad_ref.py's ops, batched), the listed entries gathered with ONE indexed gather instead of the reference's
                   Python loop over a device tensor -- this flatters the reference -- then loss.backward()
  superglue        one SuperGlue forward of the same batch (d = 128, random keypoints, the same iteration count), and the call's share

Every shape runs in a child process of its own under a time limit; a child that fails ends the run.  The parent never touches the
GPU.  A record, not a gate.  Needs a GPU.  Prints one JSON line (kept as profiles/otgrad_time.json)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((1, 1024, 30), (8, 1024, 30), (1, 2048, 100))
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
        f()
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated()
    times = {k: [] for k in fns}
    for _ in range(batches):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    return {k: {"median_ms": round(float(np.median(t)), 4), "min_ms": round(min(t), 4), "batches": len(t), "torch_peak_bytes": int(peak[k])}
            for k, t in times.items()}


def child(B, N, T, batches):
    import numpy as np
    import torch
    from image_matching_amd import _lib as L
    from image_matching_amd.engine import Engine
    from tests import otgrad_ref as O
    from tests import util
    torch.set_grad_enabled(True)
    d = 128
    eng = Engine(util.sp_config(d, N), util.sg_config(d, sinkhorn_iterations=T), "cuda")
    eng.load_state_dict(L.NET_SUPERGLUE, util.sg_sd(d))
    pairs = [O.case_scores(100 + b, N, N) for b in range(B)]
    Lc = max(mt.shape[1] for _, mt in pairs)
    am = np.zeros((B, 2, Lc), np.int64)
    for b, (_, mt) in enumerate(pairs):
        am[b, :, :mt.shape[1]] = mt
    scores = torch.from_numpy(np.stack([s for s, _ in pairs])).cuda()
    n_all = torch.tensor([mt.shape[1] for _, mt in pairs], dtype=torch.int32).cuda()
    am_d = torch.from_numpy(am).cuda()
    bin_score = torch.ones(1, device="cuda")
    bidx = torch.arange(B, device="cuda")[:, None].expand(B, Lc)
    listed = torch.arange(Lc, device="cuda")[None, :] < n_all[:, None]

    def torch_backward():
        S = scores.clone().requires_grad_(True)
        a = bin_score.clone().requires_grad_(True)
        C = torch.cat([torch.cat([S, a.expand(B, N, 1)], 2), a.expand(B, 1, N + 1)], 1)
        norm = -torch.log(torch.tensor(2.0 * N, device="cuda"))
        log_mu = torch.cat([norm.expand(N), torch.log(torch.tensor(float(N), device="cuda"))[None] + norm])[None].expand(B, -1)
        u, v = torch.zeros_like(log_mu), torch.zeros_like(log_mu)
        for _ in range(T):
            u = log_mu - torch.logsumexp(C + v.unsqueeze(1), dim=2)
            v = log_mu - torch.logsumexp(C + u.unsqueeze(2), dim=1)
        Z = C + u.unsqueeze(2) + v.unsqueeze(1) - norm
        terms = -torch.log(Z[bidx, am_d[:, 0], am_d[:, 1]].exp())
        loss = (torch.where(listed, terms, torch.zeros_like(terms)).sum(1) / n_all).sum()
        loss.backward()
        return S.grad, a.grad

    rng = np.random.default_rng(0)
    kp = torch.from_numpy((rng.random((B, N, 2)) * np.array([639.0, 479.0])).astype(np.float32)).cuda()
    sc = torch.from_numpy(rng.random((B, N)).astype(np.float32)).cuda()
    de = torch.nn.functional.normalize(torch.from_numpy(rng.standard_normal((B, d, N)).astype(np.float32)), dim=1).cuda()
    shp = (B, 1, 480, 640)
    row = events_ms({"value": lambda: eng.ot_match_loss_grad(scores, bin_score, am_d, n_all, T, want_grad=False),
                     "value_and_grad": lambda: eng.ot_match_loss_grad(scores, bin_score, am_d, n_all, T),
                     "torch_backward": torch_backward,
                     "superglue": lambda: eng.superglue(kp, sc, de, shp, kp, sc, de, shp)}, batches)
    # computed from the sizes imx_otgrad.cpp asks for, not measured: otg.u + otg.v (the value); as many again for the cotangents, the three
    # count vectors (4 N + 3 words per pair) and the dustbin terms (2 N + 1)
    ws = 4 * B * (T + 1) * (2 * N + 2)
    row["value"]["workspace_bytes"] = ws
    row["value_and_grad"]["workspace_bytes"] = 2 * ws + 4 * B * (6 * N + 4)
    row["grad_over_value"] = round(row["value_and_grad"]["median_ms"] / row["value"]["median_ms"], 3)
    row["torch_over_grad"] = round(row["torch_backward"]["median_ms"] / row["value_and_grad"]["median_ms"], 3)
    row["share_of_superglue_forward"] = round(row["value_and_grad"]["median_ms"] / row["superglue"]["median_ms"], 4)
    g = eng.ot_match_loss_grad(scores, bin_score, am_d, n_all, T)
    tg = torch_backward()[0]
    row["max_abs_diff_to_torch_at_gout_n_all"] = float(((g["grad_scores"] - tg) * n_all[:, None, None]).abs().max())
    print(json.dumps({"B": B, "N0": N, "N1": N, "iters": T, "build": eng.lib.imx_version().decode(), "device": torch.cuda.get_device_name(0), **row}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--child", default=None, help="B,N,T: time one shape in this process")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    a = ap.parse_args()
    batches = max(a.batches, 20)
    if a.child:
        return child(*(int(v) for v in a.child.split(",")), batches)
    rows, note = [], None
    for B, N, T in SHAPES:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", f"{B},{N},{T}", "--batches", str(batches)],
                               capture_output=True, text=True, timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            note = f"B={B} N={N} T={T}: no result within {LIMIT_S} s; the run ends here"
            break
        if p.returncode != 0:
            note = f"B={B} N={N} T={T}: exit status {p.returncode}; the run ends here: {p.stderr[-400:]}"
            break
        rows.append(json.loads(p.stdout.strip().splitlines()[-1]))
    out = json.dumps({"tool": "otgrad_time",
                      "timing": "HIP events on the stream, median of the batches after a warm-up, the variants alternating; one child process per shape.  "
                                "torch_backward restates the reference's log_optimal_transport and gathers the listed entries with one indexed gather "
                                "instead of the reference's Python loop, which flatters the reference.  torch_peak_bytes: the peak of torch's allocator "
                                "(inputs and outputs included); workspace_bytes: the library's otg.* scratch beside it, computed from the sizes the host unit requests (before the workspace's own rounding), not measured",
                      "shapes": rows, "note": note})
    print(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(out + "\n")
    return 0 if note is None else 1


if __name__ == "__main__":
    sys.exit(main())
