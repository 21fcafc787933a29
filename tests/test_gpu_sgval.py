"""The validation epochs of SuperGlue's training loop on the GPU (superglue/train_loop.py: SuperGlueTrainer.validate, on
Engine.estimate_homography and Engine.homography_corner_error, include/imx_homog.h; superpoint_glue_train.py --val_synthetic) at the
model and image sizes of tests/test_gpu_sgloop.py: 4 synthetic 120 x 160 training images and 3 others for validation, 64 keypoints, two
GNN layers.  Needs an MI355X; a few seconds per test."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import homography_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 128
LOOP_CONFIG = {"descriptor_dim": D, "keypoint_encoder": [32, 64], "GNN_layers": ["self", "cross"], "sinkhorn_iterations": 20, "match_threshold": 0.2}
SP_CONFIG = {"weights": None, "descriptor_dim": D, "nms_radius": 4, "keypoint_threshold": 0.005, "max_keypoints": 64}
SCALARS = ("val_loss", "val_precision", "val_recall", "val_corner_error_median", "val_homography_correct_1", "val_homography_correct_3",
           "val_homography_correct_5")


@pytest.fixture(autouse=True)
def grad_enabled():
    """(a test module that imports one of the inference scripts switches autograd off for the whole process)"""
    with torch.enable_grad():
        yield


def loop_trainer(result_dir, validation, **kw):
    """the trainer of tests/test_gpu_sgloop.py (4 synthetic images, batch 2), with 3 other synthetic images to validate on in batches of 2"""
    from image_matching_amd.superglue.train_loop import SuperGlueTrainer
    from superglue_export_pairs import SyntheticPairs
    ds = SyntheticPairs(4, SP_CONFIG, [160, 120], torch.device("cuda:0"))
    ds.seed = 2
    if validation:
        val = SyntheticPairs(3, SP_CONFIG, [160, 120], torch.device("cuda:0"), first=4, superpoint=ds.superpoint)
        val.seed = 77
        kw = {"val_dataset": val, "val_interval": 1, **kw}
    torch.manual_seed(0)                                                 # (the parameters' initial values)
    return SuperGlueTrainer(LOOP_CONFIG, ds, ds._engine(), optimizer="flat", lr=1e-3, batch_size=2, shuffle=True, seed=3, result_dir=str(result_dir),
                            log_interval=2, **kw)


def state(t):
    """everything a validation must leave alone, as host tensors: parameters and buffers, the optimiser state, the generator"""
    out = {"net." + k: v.detach().cpu().clone() for k, v in t.net.state_dict().items()}
    for i, s in t.optimizer.state_dict()["state"].items():
        out.update({f"opt.{i}.{k}": torch.as_tensor(v).detach().cpu().clone() for k, v in s.items()})
    out["rng"] = t.generator.get_state().clone()
    return out


def same_state(a, b):
    assert list(a) == list(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


def test_two_epochs_with_validation_leave_the_bits_of_two_epochs_without(tmp_path):
    plain, with_val = loop_trainer(tmp_path / "a", False), loop_trainer(tmp_path / "b", True)
    assert plain.train(2) == 2 and with_val.train(2) == 2
    same_state(state(plain), state(with_val))
    assert plain.dataset.seed == with_val.dataset.seed and with_val.val_dataset.seed == 77
    tags = [(tag, step) for tag, step, _ in with_val.history if tag.startswith("val_")]
    assert tags == [(s, e) for e in (1, 2) for s in SCALARS]
    assert [h for h in with_val.history if not h[0].startswith("val_")] == plain.history
    assert not any(tag.startswith("val_") for tag, _, _ in plain.history)


def test_validate_twice_and_against_a_recomputation(tmp_path):
    """validate() twice returns identical scalars and leaves the BatchNorm buffers and net.training as they were; val_loss, val_precision
    and val_recall equal a recomputation from forward_pairs_matches in eval mode on the same batches; the per-pair corner errors equal
    homography_ref's refit on the returned matches to the refit bar"""
    t = loop_trainer(tmp_path / "v", True)
    t.train(1)
    before = state(t)
    assert t.net.training
    first, second = t.validate(5), t.validate(6)
    assert first == second and list(first) == list(SCALARS) and t.net.training
    same_state(before, state(t))
    assert all(np.isfinite(first[k]) for k in SCALARS[:3]) and all(0.0 <= first[k] <= 1.0 for k in SCALARS[1:3] + SCALARS[4:])
    assert first["val_homography_correct_1"] <= first["val_homography_correct_3"] <= first["val_homography_correct_5"]
    t.net.eval()
    assert t.validate(7) == first and not t.net.training
    # the recomputation, batch by batch, in eval mode
    ds, eng = t.val_dataset, t.engine
    loss_sum = w_sum = 0.0
    stats, errors = np.zeros(3, np.int64), []
    with torch.no_grad():
        for indices in ([0, 1], [2]):
            b = ds.batch(indices)
            shape = tuple(b["image0"].shape[-2:])
            loss, found = t.net.forward_pairs_matches(
                b["keypoints0"], b["scores0"], b["descriptors0"].transpose(1, 2), b["keypoints1"], b["scores1"], b["descriptors1"].transpose(1, 2),
                b["all_matches"], b["n_all"], shape, shape, n0=b["counts0"], n1=b["counts1"], gt0=b["gt0"])
            _, _, err = t._validate_batch(b)
            H, inl, ninl, best = eng.estimate_homography(b["keypoints0"], b["keypoints1"], found["matches0"], counts0=b["counts0"], ransac_thresh=3.0)
            torch.cuda.synchronize()
            w = ((b["counts0"] > 0) & (b["counts1"] > 0)).cpu().numpy()
            loss_sum += float((loss.cpu().numpy().astype(np.float64) * w).sum())
            w_sum += float(w.sum())
            stats += found["stats"].sum(0).cpu().numpy()
            k0, k1, m0, c0 = (x.cpu().numpy() for x in (b["keypoints0"], b["keypoints1"], found["matches0"], b["counts0"]))
            for i in range(len(indices)):
                got = float(err[i])
                if int(best[i]) < 0:
                    assert got == np.inf
                else:
                    pair = R.Pair(k0[i], k1[i], m0[i], c0[i], 3.0, 512, 0)
                    ref = pair.refit(inl[i].cpu().numpy().astype(bool)[pair.index0], 3)
                    Hk = H[i].cpu().numpy()
                    assert R.corner_distances(Hk, ref, shape[1], shape[0]).max() <= R.REFIT_BAR
                    want = R.corner_error(ref, b["M"][i], shape[1], shape[0])
                    assert abs(got - want) <= R.REFIT_BAR, (got, want)
                errors.append(got)
    n_gt, n_pred, n_ok = (int(v) for v in stats)
    print(f"validation {first}; recomputed loss {loss_sum / max(w_sum, 1.0)}, stats {stats.tolist()}, corner errors {errors}")
    assert abs(first["val_loss"] - loss_sum / max(w_sum, 1.0)) <= 1e-6 * max(1.0, abs(first["val_loss"])), "fp32 on the device against float64 here"
    assert first["val_precision"] == n_ok / max(n_pred, 1) and first["val_recall"] == n_ok / max(n_gt, 1)
    e = np.sort(np.array(errors))
    median = e[1]                                                        # three pairs: the middle one, +inf included in the order
    assert first["val_corner_error_median"] == median or abs(first["val_corner_error_median"] - median) <= R.REFIT_BAR
    for k in (1, 3, 5):
        near = np.abs(e - k) <= R.REFIT_BAR
        assert near.any() or first[f"val_homography_correct_{k}"] == float((e < k).mean())
    t.net.train()
    # the same chain where the fits succeed (an untrained net predicts no match at all): side 1's keypoints replaced by side 0's under
    # the pair's own warp, and slot i matched to slot i
    forward, batch = t.net.forward_pairs_matches, ds.batch

    def planted_batch(indices):
        b = batch(indices)
        k0 = b["keypoints0"].cpu().numpy().astype(np.float64)
        b["keypoints1"] = torch.from_numpy(np.stack([R.project(M, k)[0] for M, k in zip(b["M"], k0)]).astype(np.float32)).to(b["keypoints0"].device)
        b["counts1"] = b["counts0"].clone()
        return b

    def oracle(*args, **kw):
        loss, found = forward(*args, **kw)
        slots = torch.arange(kw["gt0"].shape[1], device=kw["gt0"].device)[None].expand_as(kw["gt0"])
        return loss, {**found, "matches0": torch.where(slots < kw["n0"][:, None], slots, torch.full_like(slots, -1)).contiguous()}
    t.net.forward_pairs_matches, ds.batch = oracle, planted_batch
    try:
        scalars = t.validate(8)
        errors = []
        with torch.no_grad():
            for indices in ([0, 1], [2]):
                b = ds.batch(indices)
                shape = tuple(b["image0"].shape[-2:])
                _, found, err = t._validate_batch(b)
                H, inl, _, best = eng.estimate_homography(b["keypoints0"], b["keypoints1"], found["matches0"], counts0=b["counts0"], ransac_thresh=3.0)
                k0, k1, m0, c0 = (x.cpu().numpy() for x in (b["keypoints0"], b["keypoints1"], found["matches0"], b["counts0"]))
                for i in range(len(indices)):
                    assert c0[i] >= 4 and int(best[i]) >= 0
                    pair = R.Pair(k0[i], k1[i], m0[i], c0[i], 3.0, 512, 0)
                    pair.check_mask(int(best[i]), inl[i].cpu().numpy())
                    ref = pair.refit(inl[i].cpu().numpy().astype(bool)[pair.index0], 3)
                    assert R.corner_distances(H[i].cpu().numpy(), ref, shape[1], shape[0]).max() <= R.REFIT_BAR
                    assert abs(float(err[i]) - R.corner_error(ref, b["M"][i], shape[1], shape[0])) <= R.REFIT_BAR
                    errors.append(float(err[i]))
    finally:
        del t.net.forward_pairs_matches, ds.batch
    e = np.sort(np.array(errors))
    print(f"with planted matches: {scalars}; corner errors {errors}")
    assert scalars["val_corner_error_median"] == e[1] < 1e-2, "fp32 keypoints under the exact warp"
    assert scalars["val_homography_correct_1"] == scalars["val_homography_correct_3"] == scalars["val_homography_correct_5"] == 1.0


def test_the_script_validates_on_synthetic_images(tmp_path):
    """python superpoint_glue_train.py --synthetic 4 --val_synthetic 2 --epoch 1 as a child process: the validation line and the checkpoint"""
    out = tmp_path / "run"
    cmd = [sys.executable, os.path.join(ROOT, "superpoint_glue_train.py"), "--synthetic", "4", "--val_synthetic", "2", "--epoch", "1", "--Result_dir",
           str(out), "--resize", "160", "120", "--max_keypoints", "64", "--keypoint_encoder", "32", "64", "--sinkhorn_iterations", "20"]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    print(res.stdout[-2500:], res.stderr[-1500:])
    assert res.returncode == 0
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("Validation [1]: ")]
    assert len(lines) == 1 and all(tag + " " in lines[0] for tag in SCALARS)
    ckpt = torch.load(str(out / "checkpoints" / "SuperGlue_epoch_1.pth"), map_location="cpu")
    assert list(ckpt)[:2] == ["epoch", "net"] and ckpt["epoch"] == 1
    last = json.loads(res.stdout.strip().splitlines()[-1])
    assert set(last["validation"]) == set(SCALARS)
