"""tests/homography_ref.py itself -- the numpy float64 reference of the RANSAC homography fit (include/imx_homog.h) -- and the host
side of the validation epochs: the reference recovers planted homographies and leaves no point of its fixtures undecided, the index draw
gives four distinct indices, the corner error matches a hand example, and SuperGlueTrainer's validation arguments are checked without
an engine.  No GPU."""
import numpy as np
import pytest
import torch

from tests import homography_ref as R


@pytest.fixture(autouse=True)
def grad_enabled():
    """(a test module that imports one of the inference scripts switches autograd off for the whole process)"""
    with torch.enable_grad():
        yield


@pytest.mark.parametrize("noise", [0.0, 0.5])
def test_the_reference_recovers_planted_homographies(noise):
    """the shapes of tests/test_gpu_homography.py: the reference's own fit finds the planted set (without noise: exactly), its winner
    passes its own rules, and NO matched point of the winner is undecided -- continuous random coordinates keep clear of the band"""
    counts = (257, 100, 40)
    case = R.planted_case(3 if noise else 2, 3, 257, 257, counts, noise=noise)
    for b in range(3):
        pair = R.Pair(case["kpts0"][b], case["kpts1"][b], case["matches0"][b], counts[b], 3.0, 300, 11)
        H, mask, n, best = pair.estimate()
        assert H is not None and n == mask.sum() and best >= 0
        pair.check_winner(best)
        pair.check_mask(best, mask)
        assert pair.hyp(best).undecided.sum() == 0 and pair.hyp(best).gamma < 1e-6
        err = R.corner_distances(H, case["H_gt"][b], 640, 480).max()
        if noise == 0.0:
            assert np.array_equal(mask, case["planted"][b]) and err < 1e-3
        else:
            assert not mask[~case["planted"][b]].any() and mask.sum() >= 0.9 * case["planted"][b].sum() and err < 3.0


def test_the_two_float64_solutions_of_the_refit_agree_far_below_the_bar():
    """where the refit bar comes from: normal equations and lstsq on one normalised problem differ by orders less than 1e-7 px at the
    corners (an fp32 accumulation of the same sums does not)"""
    case = R.planted_case(5, 1, 300, 300, (300,), noise=0.5)
    pair = R.Pair(case["kpts0"][0], case["kpts1"][0], case["matches0"][0], 300, 3.0, 64, 0)
    _, mask, _, _ = pair.estimate(refine_iters=0)
    inl = mask[pair.index0]
    a, b = R.normalise(pair.src, pair.n0)[inl], R.normalise(pair.dst, pair.n1)[inl]
    A, rhs = R.dlt_rows(a[:, 0], a[:, 1], b[:, 0], b[:, 1])
    ref = pair.refit(inl, 0)
    for dtype, below in ((np.float64, True), (np.float32, False)):
        A_, r_ = A.astype(dtype), rhs.astype(dtype)
        g = np.linalg.solve((A_.T @ A_).astype(np.float64), (A_.T @ r_).astype(np.float64))
        H = R.denormalise(np.append(g, 1.0).reshape(3, 3), pair.n0, pair.n1)
        d = R.corner_distances(H / H[2, 2], ref, 640, 480).max()
        assert (d <= 1e-3 * R.REFIT_BAR) if below else (d > R.REFIT_BAR), (dtype, d)


def test_failure_cases_of_the_reference():
    k = np.random.default_rng(0).uniform(0, 500, (9, 2)).astype(np.float32)
    m = np.full(9, -1, np.int64)
    m[:3] = [0, 1, 2]
    assert R.Pair(k, k, m, None, 3.0, 16, 0).estimate()[0] is None                   # three matches
    same = np.tile(np.float32([[5, 7]]), (9, 1))
    assert R.Pair(same, same, np.arange(9), None, 3.0, 16, 0).estimate()[0] is None  # mean distance 0
    line = np.stack([np.arange(9.0), 2 * np.arange(9.0)], -1).astype(np.float32)
    assert R.Pair(line, line, np.arange(9), None, 3.0, 16, 0).estimate()[0] is None  # every hypothesis degenerate


def test_the_index_draw_gives_four_distinct_indices():
    for n in list(range(4, 10)) + [257, 8193, 1 << 20]:
        seen = set()
        for h in range(400 if n < 10 else 50):
            for seed in (0, 11, 0xFFFFFFFF):
                d = R.draw4(seed, h, n)
                assert len(set(d)) == 4 and all(0 <= i < n for i in d), (n, h, d)
                seen.update(d)
        assert n >= 10 or seen == set(range(n))              # a small set is covered
    assert R.draw4(0, 0, 4) != R.draw4(0, 1, 4) or R.draw4(0, 0, 4) != R.draw4(0, 2, 4)
    assert R.draw4(1, 5, 100) == R.draw4(1, 5, 100) and R.draw4(1, 5, 100) != R.draw4(2, 5, 100)
    assert R.mix32(0) == 0 and R.mix32(1) == 0x514E28B7      # murmur3's finaliser


def test_corner_error_by_hand():
    """a shift by (3, 4) moves every corner 5 px; a scale about the origin by 1.01 moves the corners of a 101 x 51 image by 0, 1, sqrt
    1.25 and 0.5 px; an all-zero estimate is +inf"""
    eye = np.eye(3)
    shift = np.array([[1, 0, 3], [0, 1, 4], [0, 0, 1.0]])
    assert abs(R.corner_error(shift, eye, 640, 480) - 5.0) < 1e-12
    scale = np.diag([1.01, 1.01, 1.0])
    assert abs(R.corner_error(scale, eye, 101, 51) - (0 + 1 + np.sqrt(1.25) + 0.5) / 4) < 1e-12
    assert abs(R.corner_error(2 * shift, eye, 640, 480) - 5.0) < 1e-12            # the scale of a homography is free
    assert R.corner_error(np.zeros((3, 3)), eye, 640, 480) == np.inf


CONFIG = {"descriptor_dim": 64, "keypoint_encoder": [32, 64], "GNN_layers": ["self", "cross"], "sinkhorn_iterations": 20, "match_threshold": 0.2}


class _Set:
    seed = 9

    def __len__(self):
        return 5


def test_trainer_validation_arguments_without_an_engine():
    from image_matching_amd.superglue.train_loop import SuperGlueTrainer
    t = SuperGlueTrainer(CONFIG, None, None, batch_size=2)
    assert t.val_dataset is None and t.val_interval == 1 and t.val_batch_size == 2 and t.val_thresh == 3.0 and t.last_validation is None
    with pytest.raises(RuntimeError):
        t.validate(1)
    t = SuperGlueTrainer(CONFIG, None, None, batch_size=2, val_dataset=_Set(), val_interval=3, val_batch_size=4, val_thresh=5)
    assert (t.val_interval, t.val_batch_size, t.val_thresh, t._val_seed) == (3, 4, 5.0, 9)
    assert t._val_batches() == [[0, 1, 2, 3], [4]]           # index order, every sample
    for bad in ({"val_interval": 0}, {"val_batch_size": 0}, {"val_thresh": 0.0}, {"val_thresh": float("nan")}, {"val_thresh": float("inf")}):
        with pytest.raises(ValueError):
            SuperGlueTrainer(CONFIG, None, None, val_dataset=_Set(), **bad)
    # the checkpoint carries nothing of the validation
    assert list(t.checkpoint(0)) == ["epoch", "net", "optimizer", "rng"]


def test_the_training_script_takes_the_validation_flags():
    import superpoint_glue_train as script
    opt = script.build_parser().parse_args([])
    assert script.validation_options(opt) == ("", 1, 0) and not hasattr(opt, "val_path")
    opt = script.build_parser().parse_args("--synthetic 4 --val_synthetic 2 --val_interval 3".split())
    assert script.validation_options(opt) == ("", 3, 2)
    assert script.validation_options(script.build_parser().parse_args(["--val_path", "data/val"])) == ("data/val", 1, 0)


def test_the_registration_script_takes_the_transform_flag():
    import superpoint_glue_register as cli
    import superpoint_glue_test as base
    opt = cli.build_parser().parse_args([])
    assert opt.transform == "similarity" and opt.models == "trained"
    # every flag and default of the script it extends, and the two of its own
    assert {k: v for k, v in vars(opt).items() if k not in ("transform", "models")} == vars(base.build_parser().parse_args([]))
    assert cli.build_parser().parse_args(["--transform", "homography"]).transform == "homography"
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["--transform", "affine"])
    assert cli.models_of(["--models", "official", "--synthetic", "2"]) == "official" and cli.models_of(["--models=official"]) == "official"
    assert cli.models_of(["--synthetic", "2"]) == "trained"
    assert cli.build_parser("official").parse_args(["--models", "official"]).descriptor_dim == 256
    assert not hasattr(base.build_parser().parse_args([]), "transform")          # the reference's script is as it was
    opt = cli.build_parser().parse_args(["--transform", "homography", "--ransac", "host"])
    with pytest.raises(SystemExit):
        cli.run_registration(opt, None, "cuda")
