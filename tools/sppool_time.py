#!/usr/bin/env python
"""Times nn.MaxPool2d(2), the descriptor normalisation and one step of the trainable SuperPoint on the GPU at SuperPoint's training
shapes.  HIP events on the stream, a warm-up, then the median of `--batches` (at least 20) batches, the variants alternating inside one
process.  Each variant with the peak of torch's allocator above what was allocated before.

  pool rows (16, 64, 240, 320) and (16, 64, 480, 640)
    forward / backward   the two library calls through Engine (output tensors allocated per call)
    ours                 sptrain_net.max_pool2 forward plus backward() under torch.autograd: one index byte per output saved
    ours_repeat          the same again in the same alternation: the spread between two repeats of one variant
    torch_autograd       PyTorch-ROCm F.max_pool2d, forward plus backward(), in the same process (an int64 index per output saved)
    kernels_ms           the two kernels alone: the median over the batches of imx_timing_report's time between the events around each
                         launch, one report per call, beside stream_bound_ms: the bytes
                         the kernel needs (forward 16 + 4 + 1 per output, backward 4 + 1 + 16) at 6.29 TB/s
  norm row (16, 256, 30 x 40)
    ours / torch_autograd   sptrain_net.normalize_descriptors against desc.div(torch.unsqueeze(torch.norm(desc, p=2, dim=1), 1)),
                         forward plus backward(); kernels_ms beside stream_bound_ms (forward x, y, norm once each; backward y, dy, dx, norm)
  step row (16, 1, 240, 320), descriptor_length 256
    pooled               one SuperPointTrainable step: forward, backward() of mean(semi^2) + mean((desc - t)^2), Adam
    down_form            the same model with sptrain_net.down_form (F.max_pool2d) in place of down_pooled: the path before libimx_sppool
    torch_net            the restated all-PyTorch network (tests/sppool_ref.py: Net), the same step

Every row runs in a child process of its own under a time limit; a child that fails ends the run.  The parent never touches the GPU.
A record, not a gate.  Needs a GPU.  Prints one JSON line (kept as profiles/sppool_time.json)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.mhagrad_time import events_ms   # noqa: E402  (the same measurement)

POOL_SHAPES = ((16, 64, 240, 320), (16, 64, 480, 640))
NORM_SHAPE = (16, 256, 30, 40)
STEP_SHAPE = (16, 1, 240, 320)
LIMIT_S = 180
STREAM_BYTES_PER_S = 6.29e12


def seeded(shape, seed):
    import torch
    return torch.randn(*shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))


def engine():
    from image_matching_amd.engine import Engine
    from tests import util
    return Engine(util.sp_config(128, 256), util.sg_config(128), "cuda")


def kernel_rows(eng, prefix, fn, batches):
    """per kernel the median over `batches` calls of fn() of the time between the events around its launch (one report per call), and
    the forms the library reported"""
    import numpy as np
    import torch
    times, forms = {}, set()
    eng.set_timing(True)
    for _ in range(batches):
        eng.timing_reset()
        fn()
        torch.cuda.synchronize()
        for name, launches, ms, form in eng.timing_report(forms=True):
            if name.startswith(prefix):
                times.setdefault(name, []).append(ms / launches)
                forms |= {form} if form else set()
    eng.set_timing(False)
    eng.timing_reset()
    return {k: round(float(np.median(v)), 4) for k, v in times.items()}, sorted(forms)


def autograd_of(x, dy, fn):
    def run():
        leaf = x.detach().requires_grad_(True)
        fn(leaf).backward(dy)
        return leaf.grad
    return run


def child_pool(B, C, H, W, batches):
    import torch
    import torch.nn.functional as F
    from image_matching_amd import sptrain_net
    torch.set_grad_enabled(True)
    eng = engine()
    x, dy = torch.relu(seeded((B, C, H, W), 1)), seeded((B, C, H // 2, W // 2), 2)
    idx = eng.maxpool2_forward_train(x)["idx"]
    ours = autograd_of(x, dy, lambda t: sptrain_net.max_pool2(eng, t))
    theirs = autograd_of(x, dy, lambda t: F.max_pool2d(t, 2))
    row = events_ms({"forward": lambda: eng.maxpool2_forward_train(x), "backward": lambda: eng.maxpool2_backward(idx, dy, x.shape),
                     "ours": ours, "ours_repeat": ours, "torch_autograd": theirs}, batches)
    row["torch_over_ours"] = round(row["torch_autograd"]["median_ms"] / row["ours"]["median_ms"], 3)
    row["ours_repeat_spread_ms"] = round(abs(row["ours"]["median_ms"] - row["ours_repeat"]["median_ms"]), 4)
    row["equal_to_torch"] = bool(torch.equal(ours(), theirs()))
    row["kernels_ms"], row["form"] = kernel_rows(eng, "maxpool2_", lambda: (eng.maxpool2_forward_train(x), eng.maxpool2_backward(idx, dy, x.shape)), batches)
    bound = round(21 * B * C * (H // 2) * (W // 2) / STREAM_BYTES_PER_S * 1e3, 5)
    row["stream_bound_ms"] = {"maxpool2_fwd": bound, "maxpool2_bwd": bound}
    row["times_stream_bound"] = {k: round(v / bound, 3) for k, v in row["kernels_ms"].items()}
    print(json.dumps({"B": B, "C": C, "H": H, "W": W, "build": eng.lib.imx_version().decode(), "device": torch.cuda.get_device_name(0), **row}))


def child_norm(B, C, H, W, batches):
    import torch
    from image_matching_amd import sptrain_net
    torch.set_grad_enabled(True)
    eng = engine()
    x, dy = seeded((B, C, H, W), 1), seeded((B, C, H, W), 2)
    fwd = eng.l2norm_forward_train(x)
    ours = autograd_of(x, dy, lambda t: sptrain_net.normalize_descriptors(eng, t))
    theirs = autograd_of(x, dy, lambda t: t.div(torch.unsqueeze(torch.norm(t, p=2, dim=1), 1)))
    row = events_ms({"forward": lambda: eng.l2norm_forward_train(x), "backward": lambda: eng.l2norm_backward(fwd["y"], fwd["norm"], dy),
                     "ours": ours, "ours_repeat": ours, "torch_autograd": theirs}, batches)
    row["torch_over_ours"] = round(row["torch_autograd"]["median_ms"] / row["ours"]["median_ms"], 3)
    row["ours_repeat_spread_ms"] = round(abs(row["ours"]["median_ms"] - row["ours_repeat"]["median_ms"]), 4)
    row["max_abs_diff_to_torch"] = float((ours() - theirs()).abs().max())
    row["kernels_ms"], row["form"] = kernel_rows(eng, "l2norm_", lambda: (eng.l2norm_forward_train(x), eng.l2norm_backward(fwd["y"], fwd["norm"], dy)), batches)
    full, pix = 4 * B * C * H * W, 4 * B * H * W
    row["stream_bound_ms"] = {"l2norm_fwd": round((2 * full + pix) / STREAM_BYTES_PER_S * 1e3, 5), "l2norm_bwd": round((3 * full + pix) / STREAM_BYTES_PER_S * 1e3, 5)}
    row["times_stream_bound"] = {k: round(v / row["stream_bound_ms"][k], 3) for k, v in row["kernels_ms"].items()}
    print(json.dumps({"B": B, "C": C, "H": H, "W": W, "build": eng.lib.imx_version().decode(), "device": torch.cuda.get_device_name(0), **row}))


def child_step(B, C, H, W, batches):
    import torch
    from image_matching_amd import sptrain_net as N
    from image_matching_amd.sptrain_model import SuperPointTrainable
    from tests import sppool_ref as RP
    torch.set_grad_enabled(True)
    eng = engine()
    x, t = seeded((B, C, H, W), 1), 0.1 * seeded((B, 256, H // 8, W // 8), 2)

    def unpooled(m, a):          # SuperPointTrainable.forward with down_form in place of down_pooled
        x4 = N.down_form(eng, m.down3, N.down_form(eng, m.down2, N.down_form(eng, m.down1, N.double_conv_form(eng, m.inc.conv, a, m.form), m.form), m.form), m.form)
        return {'semi': N.head(eng, m.convPa, m.bnPa, m.convPb, m.bnPb, x4),
                'desc': N.normalize_descriptors(eng, N.head(eng, m.convDa, m.bnDa, m.convDb, m.bnDb, x4))}

    def stepper(model, forward):
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)

        def run():
            opt.zero_grad()
            out = forward(x)
            loss = (out['semi'] ** 2).mean() + ((out['desc'] - t) ** 2).mean()
            loss.backward()
            opt.step()
            return loss
        return run

    torch.manual_seed(0)
    pooled = SuperPointTrainable(eng).train()
    plain = SuperPointTrainable(eng).train()
    net = RP.Net(256).cuda().train()
    row = events_ms({"pooled": stepper(pooled, pooled), "down_form": stepper(plain, lambda a: unpooled(plain, a)),
                     "pooled_repeat": stepper(pooled, pooled), "torch_net": stepper(net, net)}, batches)
    row["down_form_over_pooled"] = round(row["down_form"]["median_ms"] / row["pooled"]["median_ms"], 3)
    row["torch_over_pooled"] = round(row["torch_net"]["median_ms"] / row["pooled"]["median_ms"], 3)
    row["pooled_repeat_spread_ms"] = round(abs(row["pooled"]["median_ms"] - row["pooled_repeat"]["median_ms"]), 4)
    print(json.dumps({"B": B, "C": C, "H": H, "W": W, "build": eng.lib.imx_version().decode(), "device": torch.cuda.get_device_name(0), **row}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--child", nargs=2, default=None, metavar=("KIND", "B,C,H,W"), help="pool | norm | step: time one row in this process")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    a = ap.parse_args()
    batches = max(a.batches, 20)
    if a.child:
        return {"pool": child_pool, "norm": child_norm, "step": child_step}[a.child[0]](*(int(v) for v in a.child[1].split(",")), batches)
    rows, note = {"pool": [], "norm": [], "step": []}, None
    for kind, shape in [("pool", s) for s in POOL_SHAPES] + [("norm", NORM_SHAPE), ("step", STEP_SHAPE)]:
        what = f"{kind} {','.join(map(str, shape))}"
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, ",".join(map(str, shape)), "--batches", str(batches)],
                               capture_output=True, text=True, timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            note = f"{what}: no result within {LIMIT_S} s; the run ends here"
            break
        if p.returncode != 0:
            note = f"{what}: exit status {p.returncode}; the run ends here: {p.stderr[-400:]}"
            break
        rows[kind].append(json.loads(p.stdout.strip().splitlines()[-1]))
        print(f"{what}: done", file=sys.stderr, flush=True)
    out = json.dumps({"tool": "sppool_time",
                      "timing": "HIP events on the stream, median of the batches after a warm-up, the variants alternating; one child process per row.  "
                                "forward / backward: the two library calls through Engine (output tensors allocated per call).  ours and torch_autograd: "
                                "forward plus backward() under torch.autograd, a fresh leaf per batch; *_repeat is the variant once more in the same "
                                "alternation.  torch_peak_bytes_above_baseline: the peak of torch's allocator over one call above what was allocated "
                                "before it.  kernels_ms beside stream_bound_ms: the bytes the kernel needs at 6.29 TB/s.  step: forward, backward() and "
                                "one Adam step of the whole network; down_form is the same model pooling through F.max_pool2d",
                      "pool": rows["pool"], "norm": rows["norm"], "step": rows["step"], "note": note})
    print(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(out + "\n")
    return 0 if note is None else 1


if __name__ == "__main__":
    sys.exit(main())
