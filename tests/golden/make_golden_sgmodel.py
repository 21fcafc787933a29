"""Writes the fixture of one whole training step of SuperGlue from the REFERENCE's own model under torch.autograd (imported unchanged;
never runs where the reference is absent):

    python tests/golden/make_golden_sgmodel.py --reference /path/to/reference

It builds the reference's training SuperGlue (superglue/models/superglue_train.py:174-307) at CONFIG -- descriptor_dim 64, keypoint
encoder [32, 64], one self and one cross layer, 20 Sinkhorn iterations -- in .train() mode, loads the seeded parameters of
tests/scoregrad_ref.py: model_parameters and runs the seeded sample of model_case (48 and 40 keypoints on a 120 x 160 image, 30 planted
matches and the dustbin listings) in float64 and in fp32 on the CPU: forward, loss.backward().  Inputs and parameters are NOT stored: the
tests re-derive them from the seed.  sgmodel_step.npz holds

  seed, refused                        the seed taken and how many seeds the rule below refused before it
  names                                "loss" and the 41 parameter names; per name t:
  t_g, t_d32, t_sum                    the float64 value at positions(index, size) (up to 400), the reference's fp32 value minus it at the
                                       same positions, and the float64 sum of the whole tensor (1)
  buffer_names, buffer_<i>             every BatchNorm buffer of the float64 module after the step (num_batches_tracked is 2: the model
                                       calls each of its modules once per image)
  matches0/1, mscores0/1_g, _d32       the reference's matches and matching scores (float64; the fp32 difference of the scores)
  margin0, margin1                     the float64 gap between the two largest entries of each row / column of the inner block of Z: a
                                       keypoint whose gap is below MARGIN may choose another partner in fp32, and the tests leave it out
  adam_lr, adam_losses, adam_d32       the float64 losses of 4 consecutive torch.optim.Adam steps at lr = 1e-3 on the same sample from
                                       the same start, and the fp32 losses minus them

The seed rule, as in make_golden_bngrad.py: ReLU's derivative jumps at 0, so from the starting seed upward the generator takes the first
seed with no BatchNorm pre-activation within KINK = 1e-5 of 0 (in the step) and no non-finite reference value, and records how many it
refused.  It asserts that at most 5 % of the keypoints fall under MARGIN and that the Adam losses strictly decrease."""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import bngrad_ref   # noqa: E402
from tests import scoregrad_ref as R   # noqa: E402

CONFIG = R.MODEL_CONFIG
SEED0 = 1
N_SAMPLE = 400
MAX_REFUSED = 3
MARGIN, MARGIN_CAP = 1e-3, 0.05
ADAM_STEPS, ADAM_LR = 4, 1e-3


def positions(index, size):
    """the fixed pseudo-random sample of flat positions of tensor `index` of names (the tests call this too)"""
    return np.sort(np.random.default_rng([43, int(index)]).choice(size, min(N_SAMPLE, size), replace=False))


def sample(seed, dtype):
    """model_case(seed) as the dict of tensors the reference's forward takes"""
    return {k: torch.from_numpy(v) if v.dtype == np.int64 else torch.from_numpy(v).to(dtype) for k, v in R.model_case(seed).items()}


def run(ref_module, seed, dtype):
    """one step of the reference's model -> (dict name -> float64 array of loss and gradients, the BatchNorm outputs, the module, the
    forward's dict, Z)"""
    model = R.load_parameters(ref_module.SuperGlue(dict(CONFIG)).train(), seed, dtype)
    seen = {}
    inner = ref_module.log_optimal_transport

    def recording(*args, **kw):                  # the reference's own function, its result kept for the margins
        seen["Z"] = inner(*args, **kw)
        return seen["Z"]
    ref_module.log_optimal_transport = recording
    try:
        out = {}
        zs = bngrad_ref.bn_outputs(model, lambda: out.update(model(sample(seed, dtype))))
    finally:
        ref_module.log_optimal_transport = inner
    out["loss"].backward()
    res = {"loss": out["loss"].detach().double().numpy()}
    res.update({n: p.grad.double().numpy() for n, p in model.named_parameters()})
    return res, zs, model, out, seen["Z"][0].detach()


def adam(ref_module, seed, dtype):
    model = R.load_parameters(ref_module.SuperGlue(dict(CONFIG)).train(), seed, dtype)
    opt, data, losses = torch.optim.Adam(model.parameters(), lr=ADAM_LR), sample(seed, dtype), []
    for _ in range(ADAM_STEPS):
        loss = model(data)["loss"]
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    return np.array(losses)


def build(ref_module):
    for seed in range(SEED0, SEED0 + 64):
        r64, zs, m64, out64, Z64 = run(ref_module, seed, torch.float64)
        r32, _, _, out32, _ = run(ref_module, seed, torch.float32)
        a64, a32 = adam(ref_module, seed, torch.float64), adam(ref_module, seed, torch.float32)
        finite = all(np.isfinite(a).all() for a in list(r64.values()) + list(r32.values()) + [a64, a32])
        if any(bngrad_ref.kink(z.numpy()).any() for z in zs) or not finite:
            continue
        assert len(r64) == 42 and len(zs) == 2 * (len(CONFIG["keypoint_encoder"]) + len(CONFIG["GNN_layers"]))
        assert all(np.abs(a).max() > 0 for a in r64.values()), "a gradient of the reference is identically 0"
        fx = {"seed": np.int64(seed), "refused": np.int64(seed - SEED0), "names": np.array(list(r64))}
        for i, (name, a) in enumerate(r64.items()):
            pos = positions(i, a.size)
            fx.update({f"{name}_g": a.reshape(-1)[pos], f"{name}_d32": (r32[name] - a).reshape(-1)[pos].astype(np.float32),
                       f"{name}_sum": a.sum(keepdims=True).reshape(1)})
        buffers = R.model_buffers(m64)
        fx["buffer_names"] = np.array(list(buffers))
        fx.update({f"buffer_{i}": b for i, b in enumerate(buffers.values())})
        margin0, margin1 = (t.numpy() for t in R.top_two_margins(Z64))
        low = int((margin0 < MARGIN).sum() + (margin1 < MARGIN).sum())
        assert low <= MARGIN_CAP * (len(margin0) + len(margin1)), f"{low} keypoints under the margin"
        for side in "01":
            keep = (margin0 if side == "0" else margin1) >= MARGIN
            assert np.array_equal(out64[f"matches{side}"].numpy()[keep], out32[f"matches{side}"].numpy()[keep]), "fp32 and float64 disagree above the margin"
            ms = out64[f"matching_scores{side}"].detach().numpy()
            fx.update({f"matches{side}": out64[f"matches{side}"].numpy().astype(np.int64), f"mscores{side}_g": ms,
                       f"mscores{side}_d32": (out32[f"matching_scores{side}"].detach().double().numpy() - ms).astype(np.float32)})
        fx.update({"margin0": margin0, "margin1": margin1})
        assert np.all(np.diff(a64) < 0), f"the Adam losses do not decrease: {a64}"
        fx.update({"adam_lr": np.float64(ADAM_LR), "adam_losses": a64, "adam_d32": (a32 - a64).astype(np.float32)})
        return fx
    return f"no seed from {SEED0} passed"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    from superglue.models import superglue_train as ref_module     # noqa: E402  (the reference's, unchanged)
    fx = build(ref_module)
    assert not isinstance(fx, str), f"sgmodel_step.npz REFUSED: {fx}"
    path = os.path.join(HERE, "sgmodel_step.npz")
    np.savez_compressed(path, **fx)
    size = os.path.getsize(path)
    assert size < 400000, f"{path}: {size} bytes"
    assert int(fx["refused"]) <= MAX_REFUSED, f"{int(fx['refused'])} seeds refused"
    worst = max(float(np.max(np.abs(fx[f"{n}_d32"]) / R.bar(fx[f"{n}_g"]))) for n in fx["names"])
    print(f"sgmodel_step.npz: {size} bytes, {len(fx)} arrays, seed {int(fx['seed'])}, {int(fx['refused'])} seeds refused; loss {float(fx['loss_g'][0]):.6f}; "
          f"fp32 - float64 uses at most {worst:.3g} of 1e-4 + 1e-4 |g|; Adam {fx['adam_losses']}, fp32 within {np.abs(fx['adam_d32']).max():.2g}; "
          f"{int((fx['margin0'] < MARGIN).sum() + (fx['margin1'] < MARGIN).sum())} keypoints under the margin")


if __name__ == "__main__":
    main()
