"""The training loop on the GPU (imx_warp_labels_bi, imx_adam_flat, Engine.warp_labels_bi / adam_flat, optim.FlatAdam,
datasets/ALLSS_train.py, superpoint/Train_model_heatmap_loop.py) against the fixtures the reference wrote, the project's restatement
(tests/sploop_ref.py) and torch.optim.Adam.

The soft labels are held bit for bit.  The Adam kernel is held to a bar that comes from the reference's own error: per tensor,
max |p - p64| against the float64 restatement may be at most twice what torch.optim.Adam in fp32 on the CPU shows against the same
float64 run on the same inputs.  The bar is asserted on the tensors of 4097 and 2^20 + 3 floats; at n <= 5 the maximum over a handful of
roundings is no statistic (torch's may be 0), so those sizes are held to the large run's bits instead: an element's result does not
depend on n, on the form or on its place.  Whether the kernel equals the fp32 restatement bit for bit is printed, not asserted.
A resumed run equals the uninterrupted one bit for bit.  Needs an MI355X; a few seconds per test."""
import copy
import os

import numpy as np
import pytest
import torch

from tests import sploop_ref as S
from tests import util
from tests.test_sploop_host import DUP_MAT, DUP_PTS, GOLDEN, SIZES, dup_expected

pytestmark = pytest.mark.gpu
ADAM_SIZES = (0, 1, 3, 4, 5, 4097, (1 << 20) + 3)
BIG = (1 << 20) + 3


@pytest.fixture(scope="module")
def eng():
    from image_matching_amd.engine import Engine
    return Engine(util.sp_config(128, 256), util.sg_config(128), "cuda")


def bits(t):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------ warp_labels_bi
def load(size):
    fx = np.load(os.path.join(GOLDEN, f"sploop_labels_{size}.npz"))
    H, W = (int(v) for v in fx["size"])
    pts = fx["pts"].copy()
    for b, n in enumerate(fx["counts"]):
        pts[b, n:] = np.nan                                            # rows past the count are never read
    return fx, H, W, pts


@pytest.mark.parametrize("size", SIZES)
def test_warp_labels_bi_equals_the_reference(eng, size):
    fx, H, W, pts = load(size)
    for levels, key in ((0, "labels_bi"), (255, "labels_gaussian")):
        out, flag = eng.warp_labels_bi(pts, fx["counts"], fx["mats_px"], H, W, levels=levels, pixel_space=True)
        assert int(flag) == 0
        assert np.array_equal(bits(out), fx[key].view(np.uint32)), (size, levels)
    # an image alone, after an unrelated call that left its own order indices in the workspace, has the bits it has in the batch
    b = 11
    eng.warp_labels_bi(DUP_PTS[None], None, DUP_MAT[None], H, W, pixel_space=True)
    alone, _ = eng.warp_labels_bi(pts[b:b + 1], fx["counts"][b:b + 1], fx["mats_px"][b:b + 1], H, W, levels=255, pixel_space=True)
    assert np.array_equal(bits(alone[0]), fx["labels_gaussian"][b].view(np.uint32))
    # another handle
    from image_matching_amd.engine import Engine
    other = Engine(util.sp_config(128, 256), util.sg_config(128), "cuda")
    again, _ = other.warp_labels_bi(pts[::-1].copy(), fx["counts"][::-1].copy(), fx["mats_px"][::-1].copy(), H, W, levels=0, pixel_space=True)
    assert np.array_equal(bits(again), fx["labels_bi"][::-1].view(np.uint32))
    # the matrices on [-1,1]^2, scaled here as warp_labels scales them: the host's 3x3 products differ in their last bits between
    # processors, so this path is held to the restatement on the matrices this host made, not to the fixture
    from tests import sptrain_ref as R
    here = R.scale_pixels(fx["homographies"], H, W)
    out, _ = eng.warp_labels_bi(pts, fx["counts"], fx["homographies"], H, W, levels=255)
    for b in (5, 16):
        assert np.array_equal(bits(out[b]), S.labels_bi(fx["pts"][b, :b], here[b], H, W, 255)[0].view(np.uint32))
    # counts = 0: an all-zero map, whatever the rows hold
    zero, flag = eng.warp_labels_bi(pts[:3], np.zeros(3, np.int32), fx["mats_px"][:3], H, W, levels=255, pixel_space=True)
    assert int(flag) == 0 and not zero.any()


def test_warp_labels_bi_duplicates_and_flags(eng):
    H, W = 16, 24
    for levels in (0, 255):
        out, flag = eng.warp_labels_bi(DUP_PTS[None], None, DUP_MAT[None], H, W, levels=levels, pixel_space=True)
        ref, ref_flag = S.labels_bi(DUP_PTS, DUP_MAT, H, W, levels)
        assert int(flag) == ref_flag == 0
        assert np.array_equal(bits(out[0]), ref.view(np.uint32)) and np.array_equal(ref, dup_expected(H, W, levels))
    rev, _ = eng.warp_labels_bi(DUP_PTS[::-1].copy()[None], None, DUP_MAT[None], H, W, pixel_space=True)
    assert np.array_equal(bits(rev[0]), S.labels_bi(DUP_PTS[::-1], DUP_MAT, H, W)[0].view(np.uint32))
    # many points on few pixels: the winner does not depend on scheduling
    rng = np.random.default_rng(0)
    pts = np.stack([rng.uniform(18, 26, 700), rng.uniform(18, 24, 700)], 1).astype(np.float32)
    mat = np.array([[0.53, 0.01, 0.2], [0.02, 0.47, 0.3], [0, 0, 1]], np.float32)
    ref, _ = S.labels_bi(pts, mat, H, W, 255)
    for _ in range(2):
        out, _ = eng.warp_labels_bi(pts[None], None, mat[None], H, W, levels=255, pixel_space=True)
        assert np.array_equal(bits(out[0]), ref.view(np.uint32))
    # a coordinate in (-1, 0): bit 0, the clamp; a zero denominator: bit 1, the point dropped
    shift = np.array([[1, 0, -0.5], [0, 1, 0], [0, 0, 1]], np.float32)
    for levels in (0, 255):
        out, flag = eng.warp_labels_bi([[[0, 4]]], None, shift[None], H, W, levels=levels, pixel_space=True)
        ref, ref_flag = S.labels_bi([[0, 4]], shift, H, W, levels)
        assert int(flag) == ref_flag == 1 and np.array_equal(bits(out[0]), ref.view(np.uint32))
    assert float(out[0, 4, 0]) == 1.0 and float(out.sum()) == 1.0     # 1.5 -> 382 -> clamped to 255; -0.5 -> clamped to 0
    out, flag = eng.warp_labels_bi([[[3, 4], [5, 6]]], None, np.array([[[1, 0, 0], [0, 1, 0], [0, 0, 0]]], np.float32), H, W, pixel_space=True)
    assert int(flag) == 2 and not out.any()


# ------------------------------------------------------------------------------------------------------------ adam_flat
def adam_gpu(eng, case, weight_decay, t0, offset=0, zero_grad=False, n=None):
    """ADAM_STEPS steps of Engine.adam_flat on the first n floats of a case, the four buffers `offset` floats into their allocations
    and followed by a sentinel; returns (p, m, v, g) after the last step"""
    p0, grads, m0, v0 = case
    n = len(p0) if n is None else n
    bufs = []
    for a in (p0, grads[0], m0, v0):
        t = torch.full((offset + n + 8,), 7.0, dtype=torch.float32, device="cuda")
        t[offset:offset + n] = torch.from_numpy(a[:n]).cuda()
        bufs.append(t)
    p, g, m, v = (t[offset:offset + n] for t in bufs)
    for k in range(S.ADAM_STEPS):
        g.copy_(torch.from_numpy(grads[k][:n]).cuda())
        eng.adam_flat(p, g, m, v, weight_decay=weight_decay, step=t0 + k + 1, zero_grad=zero_grad, **S.ADAM_HYPER)
    for t in bufs:
        assert (t[:offset] == 7.0).all() and (t[offset + n:] == 7.0).all()        # nothing outside the n floats was written
    return tuple(t.cpu().numpy() for t in (p, m, v, g))


@pytest.fixture(scope="module")
def adam_big(eng):
    """the 5-step run on 2^20 + 3 floats in the 16-byte form, with and without weight decay: computed once"""
    out = {}
    for wd in (0.0, 0.01):
        case = S.adam_case(BIG, 3, 0)
        out[wd] = (case, adam_gpu(eng, case, wd, 0))
    return out


@pytest.mark.parametrize("n", ADAM_SIZES)
def test_adam_flat_sizes_and_forms(eng, adam_big, n):
    """any n, the tail, both forms: an element's bits do not depend on n or on the alignment of the four pointers"""
    case, (p_big, m_big, v_big, _) = adam_big[0.01]
    forms = []
    for offset in (0, 1):
        eng.timing_reset()
        eng.set_timing(True)
        p, m, v, g = adam_gpu(eng, case, 0.01, 0, offset=offset, n=n)
        torch.cuda.synchronize()
        forms.append({form for name, _, _, form in eng.timing_report(forms=True) if name == "adam_flat"})
        eng.set_timing(False)
        eng.timing_reset()
        assert np.array_equal(p.view(np.uint32), p_big[:n].view(np.uint32))
        assert np.array_equal(m.view(np.uint32), m_big[:n].view(np.uint32)) and np.array_equal(v.view(np.uint32), v_big[:n].view(np.uint32))
        assert np.array_equal(g, case[1][-1][:n])                     # zero_grad off: the gradient is left alone
    if n:
        assert forms == [{"x4"}, {"x1"}], forms


@pytest.mark.parametrize("t0", [0, 99999])
@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
@pytest.mark.parametrize("n", [4097, BIG])
def test_adam_flat_meets_the_bar(eng, adam_big, n, weight_decay, t0):
    case = S.adam_case(n, 3, t0)
    p64, bar = S.adam_bar(case, weight_decay, t0)
    p = adam_big[weight_decay][1][0] if (n == BIG and t0 == 0) else adam_gpu(eng, case, weight_decay, t0)[0]
    err = float(np.abs(p.astype(np.float64) - p64).max())
    same = np.array_equal(p.view(np.uint32), S.adam_run(case, weight_decay, t0, np.float32)[-1].view(np.uint32))
    rocm = S.adam_torch(case, weight_decay, t0, torch.float32, device="cuda")[-1]               # PyTorch-ROCm's own Adam: printed, not asserted
    print(f"adam_flat n {n} weight_decay {weight_decay} t0 {t0}: max |p - p64| {err:.3e}, bar (2 x torch fp32 on the CPU) {bar:.3e}, "
          f"fraction {err / bar:.3f}; torch.optim.Adam on the GPU: fraction {float(np.abs(rocm.astype(np.float64) - p64).max()) / bar:.3f}; "
          f"equals the fp32 restatement bit for bit: {same}")
    assert bar > 0 and err <= bar


def test_adam_flat_zero_grad_and_errors(eng):
    from image_matching_amd.engine import ImxError
    case = S.adam_case(4097, 5, 0)
    for offset in (0, 1):
        keep = adam_gpu(eng, case, 0.01, 0, offset=offset)
        zeroed = adam_gpu(eng, case, 0.01, 0, offset=offset, zero_grad=True)
        for a, b in zip(keep[:3], zeroed[:3]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert np.array_equal(zeroed[3].view(np.uint32), np.zeros(4097, np.uint32))        # exactly +0
    p, g, m, v = (torch.zeros(8, device="cuda") for _ in range(4))
    with pytest.raises(ImxError, match="alias"):
        eng.adam_flat(p, p, m, v, 1e-3, (0.9, 0.999), 1e-8, 0, 1)
    with pytest.raises(ImxError, match="step"):
        eng.adam_flat(p, g, m, v, 1e-3, (0.9, 0.999), 1e-8, 0, 0)
    with pytest.raises(ImxError):
        eng.adam_flat(p, g[:4], m, v, 1e-3, (0.9, 0.999), 1e-8, 0, 1)
    with pytest.raises(ImxError, match="bad scalar"):
        eng.adam_flat(p, g, m, v, 1e-3, (1.0, 0.999), 1e-8, 0, 1)


# ------------------------------------------------------------------------------------------------------------ FlatAdam
def test_flat_adam_on_the_trainable_superpoint(eng):
    from image_matching_amd.engine import ImxError
    from image_matching_amd.optim import FlatAdam
    from image_matching_amd.sptrain_model import SuperPointTrainable
    torch.manual_seed(0)
    model = SuperPointTrainable(eng, 64).train()
    opt = FlatAdam(model.parameters(), eng, lr=1e-3)
    x = torch.from_numpy(np.random.default_rng(0).random((2, 1, 48, 64), np.float32)).cuda()
    target = torch.from_numpy(np.random.default_rng(1).standard_normal((2, 65, 6, 8)).astype(np.float32)).cuda()
    conv_biases = {n: p.detach().clone() for n, p in model.named_parameters()
                   if n.endswith(".bias") and isinstance(model.get_submodule(n.rsplit(".", 1)[0]), torch.nn.Conv2d)}
    assert len(conv_biases) == 12
    start = opt.p_arena.clone()
    used = torch.zeros(opt.numel, dtype=torch.bool, device="cuda")
    for p, o in zip(opt.params, opt.offsets):
        used[o:o + p.numel()] = True
    for step in range(3):
        with torch.enable_grad():                                      # (whatever an imported module left as the global mode)
            out = model(x)
            loss = ((out["semi"] - target) ** 2).mean() + out["desc"][:, :, ::2].sum() * 1e-3
        loss.backward()
        opt.check_arenas()                                             # every p.grad is still a view of the arena
        assert float(opt.g_arena.abs().max()) > 0
        opt.step()
        assert not opt.g_arena.any()                                   # the kernel left the gradients zero
        opt.check_arenas()
        for arena in (opt.p_arena, opt.m_arena, opt.v_arena):
            assert torch.isfinite(arena).all() and not arena[~used].any()          # the padding stays 0
    assert opt.step_count == 3 and not torch.equal(start, opt.p_arena)
    for n, b in conv_biases.items():                                   # a conv bias in front of a training BatchNorm: gradient exactly 0
        assert torch.equal(model.get_parameter(n), b), n
    moved = sum(not torch.equal(p, s) for p, s in zip(opt._views(opt.p_arena), opt._views(start)))
    assert moved == 48 - 12
    sd = opt.state_dict()
    assert float(sd["state"][0]["step"]) == 3.0 and len(sd["state"]) == 48
    model.to("cpu")
    before = opt.p_arena.clone()
    with pytest.raises(ImxError, match="no longer lives"):
        opt.step()
    assert torch.equal(before, opt.p_arena) and opt.step_count == 3   # nothing was launched


# ------------------------------------------------------------------------------------------------------------ the loop
H, W, N_IMAGES = 120, 160, 4


def loop_config(**over):
    import yaml
    with open(os.path.join(GOLDEN, "superpoint_allss_train_heatmap.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg.update(train_iter=6, validation_interval=3, save_interval=3, tensorboard_interval=3)
    cfg["model"].update(batch_size=2, eval_batch_size=2)
    cfg.update(over)
    return cfg


def loop_sets(cfg):
    from image_matching_amd import synth
    from image_matching_amd.datasets.ALLSS_train import ALLSSTrain
    rng = np.random.default_rng(5)
    images = np.stack([synth.synth_pair(i, H, W)[0] for i in range(N_IMAGES)]).astype(np.float32)
    points = [np.stack([rng.uniform(0, W - 1, 30), rng.uniform(0, H - 1, 30)], 1).astype(np.float32) for _ in range(N_IMAGES)]
    data = {k: v for k, v in cfg["data"].items() if k not in ("dataset", "root", "root_split_txt")}
    return tuple(ALLSSTrain(task=t, images=images, points=points, **data) for t in ("train", "val"))


def make_agent(cfg, save_path):
    from image_matching_amd.superpoint.Train_model_heatmap_loop import BatchLoader, Train_model_heatmap
    train_set, val_set = loop_sets(cfg)
    agent = Train_model_heatmap(cfg, save_path=save_path, device="cuda")
    agent.train_loader = BatchLoader(train_set, cfg["model"]["batch_size"])
    agent.val_loader = BatchLoader(val_set, cfg["model"]["eval_batch_size"])
    torch.manual_seed(0)                                               # the initial weights
    agent.loadModel()
    agent.dataParallel()
    return agent


@pytest.fixture(scope="module")
def full_run(tmp_path_factory):
    """train() once: 6 iterations, validation, checkpoints and scalar read-backs at 3 and 6"""
    path = tmp_path_factory.mktemp("run")
    agent = make_agent(loop_config(), path)
    agent.train()
    torch.cuda.synchronize()
    return agent, path


def test_loop_runs_the_shipped_configuration(eng, full_run):
    from image_matching_amd.sptrain_model import SuperPointTrainable
    from image_matching_amd.superpoint.models.superpoint_train import SuperPoint
    agent, path = full_run
    assert agent.n_iter == 6 and agent.gaussian and agent.optimizer.step_count == 6
    names = sorted(os.listdir(path))
    assert names == ["superPointNet_3_checkpoint.pth.tar", "superPointNet_6_checkpoint.pth.tar"]
    for name, n in zip(names, (3, 6)):
        ck = torch.load(os.path.join(path, name), map_location="cuda")
        assert set(ck) == {"n_iter", "model_state_dict", "optimizer_state_dict", "loss"} and ck["n_iter"] == n + 1
        assert set(ck["optimizer_state_dict"]) == {"state", "param_groups"} and float(ck["optimizer_state_dict"]["state"][47]["step"]) == n
        SuperPoint(128).to("cuda").load_state_dict(ck["model_state_dict"])            # the inference class takes it
        opt = torch.optim.Adam(SuperPointTrainable(None, 128).parameters())
        opt.load_state_dict(ck["optimizer_state_dict"])                               # and torch's Adam the optimiser state
    keys = {"loss", "loss_det", "loss_det_warp", "positive_dist", "negative_dist", "precision", "recall"}
    assert [(t, n) for t, n, _ in agent.history] == [("train", 0), ("val", 3), ("val", 4), ("train", 3), ("val", 6), ("val", 7)]
    for _, _, row in agent.history:
        assert set(row) == keys and all(np.isfinite(v) for v in row.values())
    assert set(agent.scalar_dict) >= keys - {"precision", "recall"} and all(v.dim() == 0 and v.is_cuda for v in agent.scalar_dict.values())


def test_loop_trains_on_the_gaussian_labels(eng, full_run):
    agent, _ = full_run
    state = copy.deepcopy(agent.net.state_dict())
    batch = agent.val_loader.dataset.batch([0, 1])
    assert {"labels_2D_gaussian", "warped_labels_bi", "warped_labels_gaussian"} <= set(batch)
    assert torch.equal(batch["labels_2D_gaussian"], batch["labels_2D"])
    g, bi, hard = batch["warped_labels_gaussian"], batch["warped_labels_bi"], batch["warped_labels"]
    assert g.shape == hard.shape == bi.shape == (2, 1, H, W)
    assert np.array_equal(bits(g), S.quantise(bi.cpu().numpy()).view(np.uint32))        # the 8-bit round trip of the splat (the clamp included)
    assert not torch.equal(g, hard) and float(bi.sum()) > 0
    scalars = agent.train_val_sample(batch, 100, train=False)
    semi_warp, mask = agent.outputs["semi_warp"], batch["warped_valid_mask"]
    soft = agent.engine.detector_loss(semi_warp, g, mask)[0]
    assert np.array_equal(bits(scalars["loss_det_warp"]), bits(soft))
    assert not np.array_equal(bits(soft), bits(agent.engine.detector_loss(semi_warp, hard, mask)[0]))
    # one sample through __getitem__: the reference's shapes
    item = agent.val_loader.dataset[1]
    for k in ("labels_2D_gaussian", "warped_labels_bi", "warped_labels_gaussian"):
        assert item[k].shape == (1, H, W) and item[k].device.type == "cpu" and torch.equal(item[k], batch[k][1].cpu())
    # the flag off: the hard labels
    cfg = loop_config()
    cfg["data"]["gaussian_label"]["enable"] = False
    plain = make_agent(cfg, agent.save_path)
    plain.net.load_state_dict(state)
    hard_batch = plain.val_loader.dataset.batch([0, 1])
    assert "warped_labels_gaussian" not in hard_batch and torch.equal(hard_batch["warped_labels"], hard)
    s2 = plain.train_val_sample(hard_batch, 100, train=False)
    assert np.array_equal(bits(s2["loss_det_warp"]), bits(plain.engine.detector_loss(plain.outputs["semi_warp"], hard, mask)[0]))


def test_resumed_run_equals_the_uninterrupted_one(full_run, tmp_path):
    agent, path = full_run
    cfg = loop_config(retrain=False, reset_iter=False, pretrained=os.path.join(path, "superPointNet_3_checkpoint.pth.tar"))
    resumed = make_agent(cfg, tmp_path)
    assert resumed.n_iter == 3 and resumed.optimizer.step_count == 3
    resumed.train()
    torch.cuda.synchronize()
    assert resumed.n_iter == 6 and os.listdir(tmp_path) == ["superPointNet_6_checkpoint.pth.tar"]
    a = torch.load(os.path.join(path, "superPointNet_6_checkpoint.pth.tar"), map_location="cpu")
    b = torch.load(os.path.join(tmp_path, "superPointNet_6_checkpoint.pth.tar"), map_location="cpu")
    assert a["n_iter"] == b["n_iter"] == 7
    assert list(a["model_state_dict"]) == list(b["model_state_dict"])
    for k, v in a["model_state_dict"].items():                        # parameters and BatchNorm buffers
        assert torch.equal(v, b["model_state_dict"][k]), k
    assert a["optimizer_state_dict"]["param_groups"] == b["optimizer_state_dict"]["param_groups"]
    for i, s in a["optimizer_state_dict"]["state"].items():
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(s[k], b["optimizer_state_dict"]["state"][i][k]), (i, k)
    assert torch.equal(a["loss"], b["loss"])
    assert [r for r in resumed.history] == [r for r in agent.history if 3 <= r[1] <= 7 and not (r[0] == "val" and r[1] < 6)]     # (another test validates at 100)


def test_the_loop_learns(tmp_path):
    """40 iterations on one fixed batch at learning_rate 1e-3: the mean of the last five training losses is below the mean of the first five"""
    cfg = loop_config(tensorboard_interval=1000)
    cfg["model"]["learning_rate"] = 1e-3
    agent = make_agent(cfg, tmp_path)
    batch = agent.train_loader.dataset.batch([0, 1])
    losses = [agent.train_val_sample(batch, 1 + i, train=True)["loss"] for i in range(40)]
    losses = torch.stack(losses).cpu().numpy()
    print("training losses:", np.array2string(losses, precision=4))
    assert np.isfinite(losses).all() and losses[-5:].mean() < losses[:5].mean()
