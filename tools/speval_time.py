#!/usr/bin/env python
"""Times libimx_speval.so and what validate_metrics() adds to SuperPoint's training, on the GPU.  HIP events on the stream, a warm-up,
then the median of `--batches` (at least 20) calls, the variants alternating inside one process; every row runs in a child process of
its own under a time limit.

  match B,N,D       Engine.mutual_nn_match on B pairs of N unit descriptors a side (half of side 1 noisy copies of side 0) beside two
                    alternatives: `knn_both`, Engine.knn_ratio_match in both directions with ratio 1 and the mutual test as torch ops (what
                    could be written before this library), and `bmm_max`, torch.bmm + max over both axes + the mutual test.  Per variant
                    the peak of torch's allocator above the baseline (the library's own workspace is outside it: reported beside it), and
                    the search kernels' TFLOP/s (2 x 2 B N^2 D flop over both directions) beside the 157 TFLOP/s fp32-matrix peak
  metric B,K        Engine.keypoint_pair_metrics on B pairs of K keypoints a side beside the same statement as torch ops in float64
                    (projection, shared view, torch.cdist, two minima, the match test)
  pass H,W          one validate_metrics() pass of 16 pairs at H x W (batch 8, 1000 keypoints at most) beside the median training step of
                    the same agent, as a share of the shipped validation_interval (2000) training steps: wall clock between synchronisations

A record, not a gate.  Needs a GPU.  Prints one JSON line (kept as profiles/speval_time.json)."""
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
from tools.sppool_time import kernel_rows   # noqa: E402

ROWS = (("match", 1, 1024, 128), ("match", 16, 1024, 128), ("match", 1, 1024, 256), ("match", 16, 1024, 256),
        ("metric", 1, 1024, 0), ("metric", 16, 1024, 0), ("pass", 240, 320, 0), ("pass", 480, 640, 0))
LIMIT_S = 240
PEAK_TFLOPS = 157.0


def engine(d):
    from image_matching_amd.engine import Engine
    from tests import util
    return Engine(util.sp_config(d, 256), util.sg_config(d), "cuda")


def mutual_of(nn0, nn1):
    import torch
    i = torch.arange(nn0.shape[1], device=nn0.device).expand_as(nn0)
    ok = (nn0 >= 0) & (torch.gather(nn1, 1, nn0.clamp(min=0)) == i)
    return torch.where(ok, nn0, torch.full_like(nn0, -1))


def match_row(B, N, D, batches):
    import numpy as np
    import torch
    from tests import speval_ref as R
    eng = engine(D)
    a, b = R.descriptor_case(1, D, N, N)
    d0, d1 = (torch.from_numpy(np.repeat(v[None], B, 0)).cuda().transpose(1, 2) for v in (a, b))       # (B,K,D) storage, (B,D,N) views

    def knn_both():
        m0, _, _ = eng.knn_ratio_match(d0, d1, ratio=1.0)
        m1, _, _ = eng.knn_ratio_match(d1, d0, ratio=1.0)
        return mutual_of(m0, m1), mutual_of(m1, m0)

    def bmm_max():
        S = torch.bmm(d0.transpose(1, 2), d1)
        s0, nn0 = S.max(2)
        s1, nn1 = S.max(1)
        return mutual_of(nn0, nn1), mutual_of(nn1, nn0), s0, s1

    ours = lambda: eng.mutual_nn_match(d0, d1)
    row = events_ms({"mutual_nn_match": ours, "knn_both": knn_both, "bmm_max": bmm_max, "mutual_nn_match_repeat": ours}, batches)
    m_ours, m_bmm = ours()[0], bmm_max()[0]
    row["agree_with_bmm_max"] = float((m_ours == m_bmm).double().mean())
    row["kernels_ms"], _ = kernel_rows(eng, "mnn_", ours, batches)
    search = row["kernels_ms"].get("mnn_search_0", 0) + row["kernels_ms"].get("mnn_search_1", 0)
    row["search_tflops"] = round(4.0 * B * N * N * D / (search * 1e-3) / 1e12, 3) if search > 0 else None
    row["fp32_matrix_peak_tflops"] = PEAK_TFLOPS
    row["library_workspace_bytes"] = {"mutual_nn_match": 4 * B * 2 * N, "knn_both": "the (B,N0p,N1p) dot matrix and its operands, in the handle"}
    for k in ("mutual_nn_match", "knn_both", "bmm_max"):
        row[k]["slower_than_library"] = None if k == "mutual_nn_match" else row[k]["median_ms"] > row["mutual_nn_match"]["median_ms"]
    return eng, row


def metric_row(B, K, batches):
    import numpy as np
    import torch
    from tests import speval_ref as R
    eng = engine(128)
    c = R.metric_case(3, 1, K, K, (K,), (K,))
    k0, k1, m, Hm = (torch.from_numpy(np.repeat(c[k], B, 0)).cuda() for k in ("kpts0", "kpts1", "matches0", "H"))
    w, h, eps = 640, 480, 3.0

    def proj(Hs, p):
        q = torch.cat([p.double(), torch.ones_like(p[..., :1]).double()], -1) @ Hs.transpose(1, 2)
        return q[..., :2] / q[..., 2:], q[..., 2]

    def vis(xy, ww):
        return (ww > 0) & (xy[..., 0] >= 0) & (xy[..., 0] <= w - 1) & (xy[..., 1] >= 0) & (xy[..., 1] <= h - 1)

    def torch_ops():
        w0, ww0 = proj(Hm, k0)
        w1, ww1 = proj(torch.linalg.inv(Hm), k1)
        v0, v1 = vis(w0, ww0), vis(w1, ww1)
        dist = torch.cdist(w0, k1.double())
        dist = torch.where(v0[:, :, None] & v1[:, None, :], dist, torch.full_like(dist, float("inf")))
        d0, d1 = dist.min(2)[0], dist.min(1)[0]
        ok = (m >= 0) & (m < K)
        dm = (w0 - torch.gather(k1.double(), 1, m.clamp(0, K - 1)[..., None].expand(-1, -1, 2))).norm(dim=-1)
        counts = torch.stack([v0.sum(1), v1.sum(1), (d0 <= eps).sum(1), (d1 <= eps).sum(1), ok.sum(1), (ok & (ww0 > 0) & (dm <= eps)).sum(1)], 1)
        sums = torch.stack([torch.where(d0 <= eps, d0, torch.zeros_like(d0)).sum(1), torch.where(d1 <= eps, d1, torch.zeros_like(d1)).sum(1)], 1)
        return counts, sums

    ours = lambda: eng.keypoint_pair_metrics(k0, None, k1, None, Hm, (h, w), eps, matches0=m)
    row = events_ms({"keypoint_pair_metrics": ours, "torch_ops": torch_ops, "keypoint_pair_metrics_repeat": ours}, batches)
    row["counts_equal_torch_ops"] = bool(torch.equal(ours()[0][:, :6].long(), torch_ops()[0]))
    row["kernels_ms"], _ = kernel_rows(eng, "pair_metrics", ours, batches)
    row["torch_ops"]["slower_than_library"] = row["torch_ops"]["median_ms"] > row["keypoint_pair_metrics"]["median_ms"]
    return eng, row


def pass_row(H, W, batches):
    import numpy as np
    import torch
    import yaml
    from image_matching_amd import synth
    from image_matching_amd.datasets.ALLSS_train import ALLSSTrain
    from image_matching_amd.superpoint.Train_model_heatmap_loop import BatchLoader, Train_model_heatmap
    with open(os.path.join(ROOT, "tests", "golden", "superpoint_allss_train_heatmap.yaml")) as f:
        cfg = yaml.safe_load(f)
    interval = int(cfg["validation_interval"])
    cfg["validation_metrics"] = {"enable": True, "pairs": 16, "max_keypoints": 1000, "keep_best": False}
    cfg["tensorboard_interval"] = 1 << 30
    rng = np.random.default_rng(5)
    images = np.stack([synth.synth_pair(i, H, W)[0] for i in range(16)]).astype(np.float32)
    points = [np.stack([rng.uniform(0, W - 1, 200), rng.uniform(0, H - 1, 200)], 1).astype(np.float32) for _ in range(16)]
    data = {k: v for k, v in cfg["data"].items() if k not in ("dataset", "root", "root_split_txt")}
    sets = [ALLSSTrain(task=t, images=images, points=points, **data) for t in ("train", "val")]
    repeats = max(3, batches // 4)
    with tempfile.TemporaryDirectory() as tmp:
        agent = Train_model_heatmap(cfg, save_path=tmp, device="cuda")
        agent.train_loader = BatchLoader(sets[0], cfg["model"]["batch_size"])
        agent.val_loader = BatchLoader(sets[1], cfg["model"]["eval_batch_size"])
        torch.manual_seed(0)
        agent.loadModel()
        batch = agent.train_loader.dataset.batch(range(cfg["model"]["batch_size"]))
        for i in range(2):                                               # warm-up: allocations, workspaces
            agent.train_val_sample(batch, 1 + i, True)
        last = agent.validate_metrics()
        step_s, pass_s = [], []
        for r in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            agent.train_val_sample(batch, 10 + r, True)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            last = agent.validate_metrics()
            torch.cuda.synchronize()
            step_s.append(t1 - t0)
            pass_s.append(time.perf_counter() - t1)
    row = {"pairs": last["pairs"], "batch_size": cfg["model"]["batch_size"], "repeats": repeats, "validation_interval": interval,
           "train_step_ms": round(float(np.median(step_s)) * 1e3, 3), "validate_metrics_ms": round(float(np.median(pass_s)) * 1e3, 3)}
    row["share_of_validation_interval_steps"] = round(row["validate_metrics_ms"] / (row["train_step_ms"] * interval), 6)
    row["last_row"] = {k: (v if np.isfinite(v) else str(v)) for k, v in last.items()}
    return agent.validator.engine, row


def child(kind, a, b, c, batches):
    import torch
    torch.set_grad_enabled(True)
    if kind == "match":
        eng, row = match_row(a, b, c, batches)
        head = {"B": a, "N": b, "D": c}
    elif kind == "metric":
        eng, row = metric_row(a, b, batches)
        head = {"B": a, "K": b}
    else:
        eng, row = pass_row(a, b, batches)
        head = {"H": a, "W": b}
    print(json.dumps({"row": kind, **head, "build": eng.lib.imx_version().decode(), "device": torch.cuda.get_device_name(0), **row}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--child", default=None, metavar="KIND,A,B,C", help="time one row in this process")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    a = ap.parse_args()
    batches = max(a.batches, 20)
    if a.child:
        kind, *shape = a.child.split(",")
        return child(kind, *(int(v) for v in shape), batches)
    rows, notes = [], []
    for shape in ROWS:
        what = ",".join(map(str, shape))
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, "--batches", str(batches)],
                               capture_output=True, text=True, timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            notes.append(f"{what}: not measured: no result within {LIMIT_S} s; the run ends here")
            break
        if p.returncode != 0:
            notes.append(f"{what}: not measured: exit status {p.returncode}; the run ends here: {p.stderr[-400:]}")
            break
        rows.append(json.loads(p.stdout.strip().splitlines()[-1]))
        print(f"{what}: done", file=sys.stderr, flush=True)
    out = json.dumps({"tool": "speval_time",
                      "timing": "match, metric: HIP events on the stream, median of the batches after a warm-up, the variants alternating; the "
                                "kernels' own times from the library's events.  pass: wall clock between synchronisations, the median of the "
                                "repeats.  One child process per row",
                      "rows": rows, "notes": notes})
    print(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(out + "\n")
    return 0 if not notes else 1


if __name__ == "__main__":
    sys.exit(main())
