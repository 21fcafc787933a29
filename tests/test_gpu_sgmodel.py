"""image_matching_amd.sgtrain_model.SuperGlueTrainable on the GPU: one whole training step of SuperGlue -- forward, loss.backward(), Adam --
with every layer in the libraries, against what the reference's own model wrote under torch.autograd (tests/golden/sgmodel_step.npz,
tests/golden/make_golden_sgmodel.py) and against the project's restatement of that model (tests/scoregrad_ref.py: SuperGlue, held to
the fixture by tests/test_scoregrad_host.py).  The default bar, element-wise: |x - x64| <= max(1e-4 + 1e-4 |x64|, 2.5 |ref32 - x64|).
Every test prints the fractions of the bar it used.  Needs an MI355X; a few seconds per test."""
import numpy as np
import pytest
import torch

from tests import bngrad_ref
from tests import scoregrad_ref as R
from tests import util
from tests.golden.make_golden_sgmodel import ADAM_LR, ADAM_STEPS, MARGIN, MARGIN_CAP, positions

pytestmark = pytest.mark.gpu
# the biases in front of a BatchNorm: in train mode their gradient is exactly 0
CANCELLED = ("kenc.encoder.0.bias", "kenc.encoder.3.bias", "gnn.layers.0.mlp.0.bias", "gnn.layers.1.mlp.0.bias")
# the ragged case; its seed is the first from 11 upward that leaves no BatchNorm pre-activation of the float64 restatement within KINK of 0
# (the rule of the fixtures' generators; 11 was refused; test_ragged_batch asserts it of the seed taken)
RAGGED_SEED, RAGGED_COUNTS, RAGGED_PLANTED, RAGGED_FRAME = 12, ((40, 33), (23, 48)), (20, 15), (48, 48)


@pytest.fixture(autouse=True)
def grad_enabled():
    """(a test module that imports one of the inference scripts switches autograd off for the whole process)"""
    with torch.enable_grad():
        yield


@pytest.fixture(scope="module")
def eng():
    from image_matching_amd.engine import Engine
    return Engine(util.sp_config(128, 256), util.sg_config(128), "cuda")


@pytest.fixture(scope="module")
def golden():
    return util.golden("sgmodel_step.npz")


def trainable(eng, seed):
    from image_matching_amd.sgtrain_model import SuperGlueTrainable
    return R.load_parameters(SuperGlueTrainable(R.MODEL_CONFIG, eng).train(), seed)


def sample(seed):
    """model_case(seed) as the dict of device tensors the model's forward takes"""
    return {k: torch.from_numpy(v).cuda() for k, v in R.model_case(seed).items()}


def on_device(pair):
    return {k: v.cuda() if isinstance(v, torch.Tensor) else v for k, v in pair.items()}


def frac(a, ref, d32=None):
    return float(np.max(np.abs(np.asarray(a, np.float64) - ref) / R.bar(ref, d32)))


def frac_buffers(a, ref):
    return float(np.max(np.abs(np.asarray(a, np.float64) - ref) / (1e-5 + 1e-5 * np.abs(ref))))


def show(what, f):
    worst = sorted(f.items(), key=lambda kv: -kv[1])[:4]
    print(f"{what}: of the bar -- worst of {len(f)}: " + ", ".join(f"{t} {v:.3g}" for t, v in worst))


# ---------------------------------------------------------------------------------------------- one step against the reference
def test_one_step_against_the_reference(eng, golden):
    """forward(data) and loss.backward() at the fixture's config and seed: the loss and all 41 parameter gradients against the reference's
    float64 values -- the samples at the default bar with the reference's own fp32 term, the whole-tensor sums at the default bar with
    the term of the all-PyTorch restated model on this device; the BatchNorm buffers after the step at 1e-5 + 1e-5 |ref|
    (num_batches_tracked as the reference leaves it, 2: every module runs once per image); the biases in front of a train-mode
    BatchNorm have gradient exactly 0"""
    g, seed = golden, int(golden["seed"])
    model = trainable(eng, seed)
    out = model(sample(seed), want_matches=False)
    assert out["skip_train"] is False and tuple(out["loss"].shape) == (1,) and set(out) == {"loss", "skip_train"}
    out["loss"].backward()
    ours = {n: p.grad.cpu().numpy().astype(np.float64) for n, p in model.named_parameters()}
    ours["loss"] = out["loss"].detach().cpu().numpy().astype(np.float64)
    torch_model = R.load_parameters(R.SuperGlue().train(), seed).cuda()
    losses, theirs, _ = R.model_step(torch_model, [on_device(R.as_pair(R.model_case(seed), torch.float32))])
    theirs["loss"] = losses
    names = [str(n) for n in g["names"]]
    assert len(names) == 42 and set(names) == set(ours) == set(theirs)
    fo, ft = {}, {}
    for i, name in enumerate(names):
        ref, ref_sum, pos = g[f"{name}_g"], g[f"{name}_sum"], positions(i, ours[name].size)
        a, t = ours[name], theirs[name]
        assert np.isfinite(a).all(), name
        fo[name] = max(frac(a.reshape(-1)[pos], ref, g[f"{name}_d32"]), frac(a.sum(keepdims=True).reshape(1), ref_sum, t.sum() - ref_sum))
        ft[name] = max(frac(t.reshape(-1)[pos], ref, g[f"{name}_d32"]), frac(t.sum(keepdims=True).reshape(1), ref_sum))
    show("one step, SuperGlueTrainable", fo)
    show("one step, all PyTorch on the device (sums at the first term alone, not asserted)", ft)
    print(f"loss {float(ours['loss'][0]):.7f}, the reference's float64 {float(g['loss_g'][0]):.7f}")
    assert max(fo.values()) <= 1.0
    for name in CANCELLED:
        assert not ours[name].any(), f"{name}: in front of a train-mode BatchNorm, exactly 0"
    buffers, fb = R.model_buffers(model), 0.0
    assert [str(n) for n in g["buffer_names"]] == list(buffers)
    for i, (name, b) in enumerate(buffers.items()):
        if name.endswith("num_batches_tracked"):
            assert int(b) == int(g[f"buffer_{i}"]) == 2, name
        else:
            fb = max(fb, frac_buffers(b, g[f"buffer_{i}"]))
    print(f"the buffers after the step use {fb:.3g} of 1e-5 + 1e-5 |ref|")
    assert fb <= 1.0


def test_eval_mode_and_the_early_return(eng, golden):
    """.eval() works: the running statistics are used and left alone, and the biases in front of a BatchNorm get real gradients; a
    sample without keypoints on one side gives the reference's early return"""
    seed = int(golden["seed"])
    model = trainable(eng, seed).eval()
    before = R.model_buffers(model)
    out = model(sample(seed), want_matches=False)
    out["loss"].backward()
    after = R.model_buffers(model)
    assert all(np.array_equal(before[k], after[k]) for k in before)
    ref = {}
    for dtype in (torch.float64, torch.float32):                         # the restated model on the CPU: the value and the bar's second term
        losses, grads, _ = R.model_step(R.load_parameters(R.SuperGlue().eval(), seed, dtype), [R.as_pair(R.model_case(seed), dtype)])
        ref[dtype] = dict(grads, loss=losses)
    r64, r32 = ref[torch.float64], ref[torch.float32]
    f = {n: frac(p.grad.cpu().numpy(), r64[n], r32[n] - r64[n]) for n, p in model.named_parameters()}
    f["loss"] = frac(out["loss"].detach().cpu().numpy(), r64["loss"], r32["loss"] - r64["loss"])
    show("eval mode", f)
    assert max(f.values()) <= 1.0 and all(model.get_parameter(n).grad.any() for n in CANCELLED)
    data = sample(seed)
    data["keypoints1"], data["descriptors1"], data["scores1"] = data["keypoints1"][:, :, :0], data["descriptors1"][:, :, :0], data["scores1"][:0]
    out = model(data)
    assert out["skip_train"] is True and "loss" not in out
    assert tuple(out["matches0"].shape) == (48,) and bool((out["matches0"] == -1).all()) and tuple(out["matches1"].shape) == (0,)


# ---------------------------------------------------------------------------------------------- matches
def test_matches(eng, golden):
    """want_matches=True: matches0/1 equal the reference's, leaving out only the keypoints whose float64 top-two margin in Z is below
    1e-3 (at most 5 % of them); the matching scores of the kept ones at the default bar"""
    g, seed = golden, int(golden["seed"])
    model = trainable(eng, seed)
    out = model(sample(seed), want_matches=True)
    assert set(out) == {"loss", "skip_train", "matches0", "matches1", "matching_scores0", "matching_scores1"}
    assert not out["matches0"].requires_grad and not out["matching_scores0"].requires_grad
    keep0, keep1 = g["margin0"] >= MARGIN, g["margin1"] >= MARGIN
    left_out = int((~keep0).sum() + (~keep1).sum())
    assert left_out <= MARGIN_CAP * (len(keep0) + len(keep1))
    f = {}
    for side, keep in (("0", keep0), ("1", keep1)):
        got = out[f"matches{side}"].cpu().numpy()
        assert got.shape == g[f"matches{side}"].shape and np.array_equal(got[keep], g[f"matches{side}"][keep]), side
        ms, ref = out[f"matching_scores{side}"].cpu().numpy().astype(np.float64), g[f"mscores{side}_g"]
        f[f"matching_scores{side}"] = frac(ms[keep], ref[keep], g[f"mscores{side}_d32"][keep])
    print(f"matches: {left_out} of {len(keep0) + len(keep1)} keypoints left out; {int((g['matches0'] >= 0).sum())} matches, "
          f"{int((g['mscores0_g'] > 0).sum())} mutual pairs")
    show("matches", f)
    assert max(f.values()) <= 1.0


# ---------------------------------------------------------------------------------------------- four Adam steps
def test_four_adam_steps(eng, golden):
    """4 consecutive torch.optim.Adam steps at lr = 1e-3 on the fixture's sample: each loss within 1e-4 + 1e-4 |ref| of the reference's
    float64 sequence, and the sequence strictly decreasing.  (Losses, not parameters: Adam turns the reference's rounding-noise
    gradients of the BatchNorm-cancelled biases into real updates, ours are exactly 0, and the loss cannot see the difference.)"""
    g, seed = golden, int(golden["seed"])
    assert ADAM_STEPS == 4 and ADAM_LR == 1e-3 == float(g["adam_lr"])
    model, data = trainable(eng, seed), sample(seed)
    opt, losses = torch.optim.Adam(model.parameters(), lr=ADAM_LR), []
    for _ in range(ADAM_STEPS):
        out = model(data, want_matches=False)
        opt.zero_grad()
        out["loss"].backward()
        opt.step()
        losses.append(out["loss"].item())
    ref = g["adam_losses"]
    used = np.abs(np.array(losses) - ref) / (1e-4 + 1e-4 * np.abs(ref))
    print(f"Adam: losses {losses}, the reference's {ref.tolist()}; of 1e-4 + 1e-4 |ref|: {used.round(4).tolist()}")
    assert used.max() <= 1.0 and np.all(np.diff(losses) < 0)


# ---------------------------------------------------------------------------------------------- a ragged batch
def ragged_pairs(dtype):
    return [R.as_pair(R.model_case(RAGGED_SEED + b, N0=n0, N1=n1, planted=k), dtype) for b, ((n0, n1), k) in enumerate(zip(RAGGED_COUNTS, RAGGED_PLANTED))]


def test_ragged_batch(eng):
    """two pairs with counts ((40, 33), (23, 48)) in a NaN-padded frame (48, 48), train mode: forward_pairs(...) and .mean().backward()
    against the restated model in float64 on the CPU, run per pair on the valid columns with each BatchNorm call's statistics taken
    over the concatenation of both pairs' columns (tests/scoregrad_ref.py: SuperGlue on a list of pairs) -- the two losses, all 41
    gradients and the BatchNorm buffers; the default bar's second term from the same restated model in fp32 on the CPU; no BatchNorm
    pre-activation lies at the kink (asserted)"""
    ref, zs = {}, None
    for dtype in (torch.float64, torch.float32):
        m = R.load_parameters(R.SuperGlue().train(), RAGGED_SEED, dtype)
        res = {}
        seen = bngrad_ref.bn_outputs(m, lambda: res.update(zip(("losses", "grads", "Z"), R.model_step(m, ragged_pairs(dtype)))))
        ref[dtype] = dict(res["grads"], loss=res["losses"], buffers=R.model_buffers(m))
        zs = seen if dtype == torch.float64 else zs
    assert len(zs) == 8 and not any(bngrad_ref.kink(z.numpy()).any() for z in zs), "the seed keeps the pre-activations off the kink"
    r64, r32 = ref[torch.float64], ref[torch.float32]
    pairs = ragged_pairs(torch.float32)
    (F0, F1), B = RAGGED_FRAME, len(pairs)
    L = max(p["all_matches"].shape[1] for p in pairs)

    def padded(key, frame, axis):
        out = torch.full([B] + [frame if i == axis else s for i, s in enumerate(pairs[0][key].shape) if i > 0], float("nan"))
        for b, p in enumerate(pairs):
            out[b].narrow(axis - 1, 0, p[key].shape[axis]).copy_(p[key][0])
        return out.cuda()
    all_matches = torch.full((B, 2, L), -1, dtype=torch.int64)
    for b, p in enumerate(pairs):
        all_matches[b, :, :p["all_matches"].shape[1]] = p["all_matches"]
    n_all = torch.tensor([p["all_matches"].shape[1] for p in pairs], dtype=torch.int32)
    n0, n1 = (torch.tensor([c[i] for c in RAGGED_COUNTS], dtype=torch.int32).cuda() for i in (0, 1))
    model = trainable(eng, RAGGED_SEED)
    loss = model.forward_pairs(padded("kpts0", F0, 1), padded("scores0", F0, 1), padded("desc0", F0, 2), padded("kpts1", F1, 1), padded("scores1", F1, 1),
                               padded("desc1", F1, 2), all_matches.cuda(), n_all.cuda(), pairs[0]["shape0"], pairs[0]["shape1"], n0=n0, n1=n1)
    assert tuple(loss.shape) == (B,)
    loss.mean().backward()
    f = {"loss": frac(loss.detach().cpu().numpy(), r64["loss"], r32["loss"] - r64["loss"])}
    for n, p in model.named_parameters():
        a = p.grad.cpu().numpy()
        assert np.isfinite(a).all(), f"{n}: NaN padding leaked"
        f[n] = frac(a, r64[n], r32[n] - r64[n])
    show("ragged batch", f)
    assert len(f) == 42 and max(f.values()) <= 1.0
    assert all(not model.get_parameter(n).grad.any() for n in CANCELLED)
    fb = 0.0
    for name, b in R.model_buffers(model).items():
        if name.endswith("num_batches_tracked"):
            assert int(b) == int(r64["buffers"][name]) == 2, name
        else:
            fb = max(fb, frac_buffers(b, r64["buffers"][name]))
    print(f"ragged batch: the buffers after the step use {fb:.3g} of 1e-5 + 1e-5 |ref|")
    assert fb <= 1.0


# ---------------------------------------------------------------------------------------------- from the dataset to a step
def test_training_steps_on_dataset_samples(tmp_path):
    """README's example: GlueSparse on one image file, the model at d = 128, Adam.  The sample as the reference's loop hands it over
    (batch-1 DataLoader, superpoint_glue_train.py:106-112) goes through forward(); the same pair twice as a padded batch with counts
    (GlueSparse.batch -> Engine.train_pairs) goes through forward_pairs() and gives the sample's loss twice (two copies of one pair leave
    the BatchNorm statistics where they were); three Adam steps on the batch lower the loss"""
    from image_matching_amd import hostops
    from image_matching_amd.datasets.GlueSparse import GlueSparse
    from image_matching_amd.sgtrain_model import SuperGlueTrainable
    D, CAP = 128, 256
    hostops.imwrite(str(tmp_path / "im0.png"), util.golden("trainpairs_small.npz")["image_0"])
    ds = GlueSparse(str(tmp_path), util.sp_config(D, CAP), (160, 120), "cuda")
    ds.superpoint.load_state_dict(util.sp_sd(D))
    config = {"descriptor_dim": D, "keypoint_encoder": [32, 64], "GNN_layers": ["self", "cross"], "sinkhorn_iterations": 20}
    model = R.load_parameters(SuperGlueTrainable(config, ds._engine()).train(), 7)
    start = {k: v.clone() for k, v in model.state_dict().items()}
    pred = torch.utils.data.default_collate([ds[0]])
    for k in pred:
        if k not in ("file_name", "image0", "image1"):
            pred[k] = pred[k].cuda().float() if isinstance(pred[k], torch.Tensor) else torch.stack(pred[k]).cuda()
    pred["all_matches"] = pred["all_matches"].long()
    alone = model(pred, want_matches=False)["loss"]
    assert tuple(alone.shape) == (1,) and np.isfinite(alone.item())
    model.load_state_dict(start)                                         # (the buffers moved)
    b = ds.batch([0, 0])
    shape = tuple(b["image0"].shape[-2:])
    run = lambda: model.forward_pairs(b["keypoints0"], b["scores0"], b["descriptors0"].transpose(1, 2), b["keypoints1"], b["scores1"],
                                      b["descriptors1"].transpose(1, 2), b["all_matches"], b["n_all"], shape, shape, n0=b["counts0"], n1=b["counts1"])
    both = run()
    print(f"loss of the sample: {alone.item():.6f} alone, {both.tolist()} twice in a batch padded to the cap; "
          f"{int(b['counts0'][0])} / {int(b['counts1'][0])} keypoints")
    assert tuple(both.shape) == (2,) and both[0].item() == both[1].item()
    assert abs(both[0].item() - alone.item()) <= 1e-4 + 1e-4 * abs(alone.item())
    model.load_state_dict(start)
    opt, losses = torch.optim.Adam(model.parameters(), lr=1e-3), []
    for _ in range(3):
        loss = run().mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print(f"three Adam steps on the batch: {losses}")
    assert all(np.isfinite(losses)) and losses[2] < losses[1] < losses[0]
