"""The validation of a SuperPoint training run by what the deployed network does (image_matching_amd/superpoint/validation.py,
Train_model_heatmap_loop.validate_metrics, superpoint_evaluate.py, superpoint_train_descriptor.py --val_metrics) on the small synthetic
sets of tests/test_gpu_sploop.py.

evaluate() is repeatable; every scalar equals a recomputation in numpy float64 from the read-back outputs of the Engine calls, the pair
metrics through tests/speval_ref.py (integers equal, the localisation error to 1e-9 px, the ratios to a few float64 roundings); an identity
warp gives repeatability 1 and localisation error 0 exactly; a run with the metrics equals the run without them bit for bit in
everything the run without them has.  Needs an MI355X; the two six-iteration runs are made once and shared."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import speval_ref as R
from tests.test_gpu_sploop import H, W, loop_config, loop_sets, make_agent

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BEST = "superPointNet_best_checkpoint.pth.tar"
NUMBERED = ["superPointNet_3_checkpoint.pth.tar", "superPointNet_6_checkpoint.pth.tar"]


def weights(seed=None):
    """the synthetic weights of the inference class (a detector that finds points), or with a seed a fresh trainable net's"""
    from image_matching_amd.sptrain_model import SuperPointTrainable
    from image_matching_amd.superpoint.models.superpoint_train import SuperPoint
    if seed is None:
        return SuperPoint(128).state_dict()
    torch.manual_seed(seed)
    return SuperPointTrainable(None, 128).state_dict()


def val_config():
    cfg = loop_config()
    cfg["model"]["detection_threshold"] = 0.001        # the synthetic and the untrained weights both find points at it
    return cfg


@pytest.fixture(scope="module")
def validator():
    from image_matching_amd.superpoint.validation import SuperPointValidator
    cfg = val_config()
    return SuperPointValidator(cfg, loop_sets(cfg)[1], "cuda", max_keypoints=300, pairs=3, batch_size=2, seed=7)


def test_evaluate_is_repeatable_and_leaves_the_dataset_alone(validator):
    from image_matching_amd.superpoint.validation import SCALARS
    ds = validator.dataset
    assert "seed" not in vars(ds)
    gen = torch.cuda.get_rng_state(), torch.get_rng_state()
    a = validator.evaluate(weights())
    b = validator.evaluate(weights())
    assert a == b
    assert set(a) == set(SCALARS) | {"pairs"} and a["pairs"] == 3
    assert "seed" not in vars(ds) and ds.seed == 0
    assert torch.equal(gen[0], torch.cuda.get_rng_state()) and torch.equal(gen[1], torch.get_rng_state())
    assert a["val_keypoints"] > 20 and 0 < a["val_repeatability"] <= 1
    ds.seed = 5                                        # an instance's own seed is put back as it was
    assert validator.evaluate(weights()) == a
    assert vars(ds)["seed"] == 5
    del ds.seed


def test_every_scalar_equals_a_recomputation_from_the_parts(validator):
    row = validator.evaluate(weights(), keep_parts=True)
    counts, sums, err, nk = [], [], [], []
    for p in validator.parts:
        host = {k: v.cpu().numpy() for k, v in p.items() if isinstance(v, torch.Tensor)}
        assert p["size"] == (H, W)
        for b in range(len(host["n0"])):
            c, s, margin = R.pair_metrics(host["kpts0"][b], int(host["n0"][b]), host["kpts1"][b], int(host["n1"][b]), host["H_gt"][b], W, H,
                                          validator.eps, host["matches0"][b])
            assert margin > R.EPS_BAND, "a decision inside the band: a bad case"
            assert np.array_equal(host["counts"][b], c), (host["counts"][b], c)
            assert np.abs(host["sums"][b] - s).max() <= R.SUM_BAR * max(1, c[2:4].max())
            counts.append(c), sums.append(s), err.append(host["err"][b]), nk.append(int(host["n0"][b]) + int(host["n1"][b]))
    c, s, e = np.stack(counts).astype(np.float64), np.stack(sums), np.sort(np.array(err))
    P = len(e)
    assert P == row["pairs"] == 3
    v, r = c[:, 0] + c[:, 1], c[:, 2] + c[:, 3]
    lo, hi = e[(P - 1) // 2], e[P // 2]
    want = {"val_repeatability": np.mean(np.where(v > 0, r / np.maximum(v, 1), 0.0)), "val_localization_error": s.sum() / max(r.sum(), 1),
            "val_keypoints": sum(nk) / (2.0 * P), "val_matching_score": np.mean(c[:, 5] / np.maximum(c[:, 0], 1)),
            "val_match_precision": c[:, 5].sum() / max(c[:, 4].sum(), 1), "val_corner_error_median": lo if lo == hi else 0.5 * (lo + hi),
            "val_homography_correct_1": np.mean(e < 1), "val_homography_correct_3": np.mean(e < 3), "val_homography_correct_5": np.mean(e < 5)}
    print({k: (row[k], float(w)) for k, w in want.items()})
    for k, w in want.items():
        if np.isinf(w):
            assert row[k] == w, k
        elif k == "val_localization_error":
            assert abs(row[k] - w) <= R.SUM_BAR, k
        else:
            assert abs(row[k] - w) <= 4 * np.finfo(np.float64).eps * max(1.0, abs(w)), (k, row[k], w)
    assert c[:, 4].sum() > 0 and r.sum() > 0, "the case measures something: there are matches and repeated points"


class IdentityPairs:
    """a dataset whose warp is the identity: the warped image IS the image"""
    seed = 0

    def __init__(self, images):
        self.images = torch.from_numpy(images).cuda()

    def __len__(self):
        return len(self.images)

    def batch(self, indices):
        img = self.images[list(indices)][:, None]
        return {"image": img, "warped_img": img.clone(), "homographies": torch.eye(3, device="cuda").repeat(len(img), 1, 1)}


@pytest.mark.parametrize("seed", [None, 0, 1])
def test_identity_warp_repeats_every_point_exactly(seed):
    """64 x 128 images: the pixel-space warp is inverse(trans) @ I @ trans in fp32 (Engine._scaled, the expression the labels of the
    warped image are made with), which is the identity EXACTLY only where 2 / W and 2 / H are powers of two; at 120 x 160 it is the
    identity to a few 1e-8 (measured: a localisation error of 3.7e-6 px), and a dataset that hands out the image itself as the warped
    image would then contradict its own matrix.  The precondition is asserted."""
    from image_matching_amd import synth
    from image_matching_amd.superpoint.validation import SuperPointValidator
    images = np.stack([synth.synth_pair(i, 64, 128)[0] for i in range(3)]).astype(np.float32)
    v = SuperPointValidator(val_config(), IdentityPairs(images), "cuda", max_keypoints=257, pairs=3, batch_size=2)
    row = v.evaluate(weights(seed), keep_parts=True)
    print(seed, row)
    for p in v.parts:
        assert torch.equal(p["H_gt"], torch.eye(3, dtype=torch.float64, device="cuda").expand_as(p["H_gt"]))
    assert row["val_keypoints"] > 0, "no keypoint: the case measures nothing"
    assert row["val_repeatability"] == 1.0 and row["val_localization_error"] == 0.0


# ------------------------------------------------------------------------------------------------------------ the loop
@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """two 6-iteration runs from the same initial weights: without the key, and with validation_metrics on"""
    out = []
    for over in ({}, {"validation_metrics": {"enable": True, "pairs": 3, "max_keypoints": 300}}):
        path = tmp_path_factory.mktemp("with" if over else "without")
        agent = make_agent(loop_config(**over), path)
        agent.train()
        torch.cuda.synchronize()
        out.append((agent, path))
    return out


def test_without_the_key_the_run_is_what_it_was(runs):
    agent, path = runs[0]
    assert sorted(os.listdir(path)) == NUMBERED
    assert [(t, n) for t, n, _ in agent.history] == [("train", 0), ("val", 3), ("val", 4), ("train", 3), ("val", 6), ("val", 7)]
    assert agent.validator is None and agent.best is None


def test_the_metrics_change_nothing_of_the_run(runs):
    (plain, p0), (withm, p1) = runs
    assert sorted(os.listdir(p1)) == NUMBERED + [BEST]
    for name in NUMBERED:
        a, b = (torch.load(os.path.join(p, name), map_location="cpu") for p in (p0, p1))
        assert set(a) == set(b) == {"n_iter", "model_state_dict", "optimizer_state_dict", "loss"} and a["n_iter"] == b["n_iter"]
        assert list(a["model_state_dict"]) == list(b["model_state_dict"])
        for k, v in a["model_state_dict"].items():                    # parameters and BatchNorm buffers
            assert torch.equal(v, b["model_state_dict"][k]), k
        assert a["optimizer_state_dict"]["param_groups"] == b["optimizer_state_dict"]["param_groups"]
        for i, s in a["optimizer_state_dict"]["state"].items():
            for k in ("step", "exp_avg", "exp_avg_sq"):
                assert torch.equal(s[k], b["optimizer_state_dict"]["state"][i][k]), (i, k)
        assert torch.equal(a["loss"], b["loss"])
    assert [r for r in withm.history if r[0] != "metrics"] == plain.history
    assert withm.train_loader.dataset.seed == plain.train_loader.dataset.seed
    assert "seed" not in vars(withm.val_loader.dataset) and withm.val_loader.dataset.seed == plain.val_loader.dataset.seed


def test_metric_rows_and_the_best_checkpoint(runs):
    from image_matching_amd.superpoint.models.superpoint_train import SuperPoint
    from image_matching_amd.superpoint.validation import SCALARS
    agent, path = runs[1]
    rows = [r for r in agent.history if r[0] == "metrics"]
    assert [n for _, n, _ in rows] == [3, 6]
    order = [(t, n) for t, n, _ in agent.history]
    assert order.index(("metrics", 3)) == order.index(("val", 4)) + 1            # after the loss validation of that iteration
    for _, _, row in rows:
        assert set(row) == set(SCALARS) | {"pairs"} and row["pairs"] == 3 and not any(np.isnan(v) for v in row.values())
    ck = torch.load(os.path.join(path, BEST), map_location="cuda")
    assert set(ck) == {"n_iter", "model_state_dict", "optimizer_state_dict", "loss", "metrics"}
    keys = [(r["val_homography_correct_3"], r["val_repeatability"]) for _, _, r in rows]
    best = 1 if keys[1] > keys[0] else 0                                         # the first validation always writes; a tie keeps it
    assert ck["n_iter"] == (3, 6)[best] + 1 and ck["metrics"] == rows[best][2] and agent.best == keys[best]
    numbered = torch.load(os.path.join(path, NUMBERED[best]), map_location="cuda")
    for k, v in numbered["model_state_dict"].items():
        assert torch.equal(v, ck["model_state_dict"][k]), k
    SuperPoint(128).to("cuda").load_state_dict(ck["model_state_dict"])           # the inference class takes it


def test_a_resumed_run_takes_up_the_incumbent(runs, tmp_path):
    import shutil
    agent, path = runs[1]
    for name in (NUMBERED[0], BEST):
        shutil.copy(os.path.join(path, name), tmp_path / name)
    kept = torch.load(tmp_path / BEST, map_location="cpu")["metrics"]
    cfg = loop_config(retrain=False, reset_iter=False, pretrained=str(tmp_path / NUMBERED[0]),
                      validation_metrics={"enable": True, "pairs": 3, "max_keypoints": 300})
    resumed = make_agent(cfg, tmp_path)
    resumed.n_iter = 6                                  # no further step: one validation of the loaded weights
    row = resumed.validate_metrics()
    key = (row["val_homography_correct_3"], row["val_repeatability"])
    incumbent = (kept["val_homography_correct_3"], kept["val_repeatability"])
    assert resumed.best == max(key, incumbent)
    now = torch.load(tmp_path / BEST, map_location="cpu")["metrics"]
    assert now == (row if key > incumbent else kept)


# ------------------------------------------------------------------------------------------------------------ the scripts
def test_the_scripts_run(tmp_path):
    """the training script with --val_metrics, then superpoint_evaluate.py on the best checkpoint it wrote (two child processes)"""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cfg = os.path.join(ROOT, "tests", "golden", "superpoint_allss_train_heatmap.yaml")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "superpoint_train_descriptor.py"), "--synthetic", "4", "--iters", "6", "--val_metrics",
                        "--config", cfg, "--output_dir", str(tmp_path), "--exper_name", "t"], capture_output=True, text=True, cwd=ROOT, env=env,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    last = json.loads(r.stdout.strip().splitlines()[-1])
    assert last["n_iter"] == 6 and BEST in last["checkpoints"] and "val_homography_correct_3" in last["last"]
    out = tmp_path / "row.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "superpoint_evaluate.py"), "--synthetic", "2", "--size", "120", "160", "--config", cfg,
                        "--max_keypoints", "300", "--weights", str(tmp_path / "t" / "checkpoints" / BEST), "--out", str(out)],
                       capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    row = json.loads(r.stdout.strip().splitlines()[-1])
    assert row == json.load(open(out)) and row["pairs"] == 2 and "val_repeatability" in row
