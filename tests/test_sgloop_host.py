"""The host side of SuperGlue's training loop (superpoint_glue_train.py, image_matching_amd/superglue/train_loop.py): the script's flags,
the batch loss's weights, the checkpoint layout and the resume arithmetic.  No GPU: engine = None builds parameters and optimiser state
only."""
import pytest
import torch

# the reference's flags and defaults (superpoint_glue_train.py:20-48), the types as this project repairs them
REFERENCE_FLAGS = {
    "image_path": "datasets/ALLSS/", "Result_dir": "Results/ALLSS/superglue_descriptor_128", "epoch": 200, "batch_size": 1, "learning_rate": 0.0001,
    "shuffle": True, "show_keypoints": True, "viz_extension": "png",
    "superpoint_weights": "superpoint/models/weights/superPointNet_allss_descriptor_128.pth.tar", "descriptor_dim": 128,
    "keypoint_encoder": [32, 64, 128], "max_keypoints": 1200, "keypoint_threshold": 0.005, "nms_radius": 4, "sinkhorn_iterations": 30,
    "match_threshold": 0.2, "resize": [640, 480], "pretrain_weights": "", "checkpoints_dir": "checkpoints/", "checkpoints_name": "",
    "save_epoch_freq": 5, "resume": False,
}
ADDED_FLAGS = {"synthetic": 0, "iters": 0, "seed": 0, "optimizer": "flat"}
CONFIG = {"descriptor_dim": 64, "keypoint_encoder": [32, 64], "GNN_layers": ["self", "cross"], "sinkhorn_iterations": 20, "match_threshold": 0.2}


@pytest.fixture(autouse=True)
def grad_enabled():
    """(a test module that imports one of the inference scripts switches autograd off for the whole process)"""
    with torch.enable_grad():
        yield


def trainer(optimizer, **kw):
    from image_matching_amd.superglue.train_loop import SuperGlueTrainer
    return SuperGlueTrainer(CONFIG, None, None, optimizer=optimizer, lr=1e-3, **kw)


def test_the_script_parses_the_reference_flags_and_defaults():
    import superpoint_glue_train as script
    opt = script.build_parser().parse_args([])
    assert vars(opt) == {**REFERENCE_FLAGS, **ADDED_FLAGS}
    assert isinstance(opt.learning_rate, float)
    opt = script.build_parser().parse_args("--keypoint_encoder 32 64 --resize 160 120 --learning_rate 1e-3 --resume --shuffle false --show_keypoints 0 "
                                           "--checkpoints_name SuperGlue_epoch_3.pth --Result_dir out --optimizer torch --iters 2 --synthetic 4 --seed 7".split())
    assert opt.keypoint_encoder == [32, 64] and opt.resize == [160, 120] and opt.learning_rate == 1e-3
    assert opt.resume is True and opt.shuffle is False and opt.show_keypoints is False
    assert script.build_parser().parse_args(["--resume", "true"]).resume is True and script.build_parser().parse_args(["--resume", "False"]).resume is False
    # the checkpoint to resume from is built from opt.checkpoints_dir (the reference's line names an undefined variable)
    assert script.checkpoint_path(opt) == "out/checkpoints/SuperGlue_epoch_3.pth"
    cfg = script.configs(opt)
    assert cfg["superglue"] == {"descriptor_dim": 128, "keypoint_encoder": [32, 64], "sinkhorn_iterations": 30, "match_threshold": 0.2}
    assert set(cfg["superpoint"]) == {"weights", "descriptor_dim", "nms_radius", "keypoint_threshold", "max_keypoints"}
    with pytest.raises(SystemExit):
        script.build_parser().parse_args(["--optimizer", "sgd"])


def test_batch_loss_weights():
    from image_matching_amd.superglue.train_loop import batch_loss
    loss = torch.tensor([2.0, 0.0, 4.0, 0.0])
    c0, c1 = torch.tensor([5, 0, 3, 7], dtype=torch.int32), torch.tensor([4, 9, 1, 0], dtype=torch.int32)
    assert batch_loss(loss, c0, c1).item() == 3.0                        # pairs 0 and 2 count
    assert batch_loss(loss[:1], c0[:1], c1[:1]).item() == 2.0            # batch size 1: the pair's own loss
    assert batch_loss(loss[1:2], c0[1:2], c1[1:2]).item() == 0.0         # every pair empty: 0 / max(1, 0)
    x = torch.tensor([1.0, 5.0, 3.0], requires_grad=True)
    batch_loss(x, torch.tensor([1, 0, 2]), torch.tensor([1, 3, 2])).backward()
    assert x.grad.tolist() == [0.5, 0.0, 0.5]


def _some_steps(t, steps=2):
    """a few torch.optim.Adam steps on made-up gradients, so that the optimiser has state (the CPU has no kernels to take a real step)"""
    g = torch.Generator().manual_seed(3)
    for _ in range(steps):
        for p in t.net.parameters():
            p.grad = torch.randn(p.shape, generator=g) * 0.01
        t.optimizer.step()


def test_checkpoint_layout_round_trips_without_an_engine(tmp_path):
    from image_matching_amd.sgtrain_model import SuperGlueTrainable
    a = trainer("torch", result_dir=str(tmp_path), seed=5)
    _some_steps(a)
    a.generator.manual_seed(11)
    torch.randperm(7, generator=a.generator)
    assert a.save(3) == str(tmp_path) + "/checkpoints"
    ckpt = torch.load(str(tmp_path / "checkpoints" / "SuperGlue_epoch_3.pth"), map_location="cpu")
    assert list(ckpt) == ["epoch", "net", "optimizer", "rng"], "the reference's two keys first"
    assert ckpt["epoch"] == 3 and list(ckpt["net"]) == list(a.net.state_dict())
    plain = SuperGlueTrainable(CONFIG, None)
    plain.load_state_dict(ckpt["net"])
    assert all(torch.equal(v, a.net.state_dict()[k]) for k, v in plain.state_dict().items())
    assert set(ckpt["optimizer"]) == {"state", "param_groups"} and len(ckpt["optimizer"]["state"]) == len(list(a.net.parameters()))
    # torch's Adam format from either optimiser, into either optimiser
    for kind in ("torch", "flat"):
        b = trainer(kind, result_dir=str(tmp_path / kind))
        assert b.resume(tmp_path / "checkpoints" / "SuperGlue_epoch_3.pth") == 3 and b.epoch == 3
        assert all(torch.equal(v, a.net.state_dict()[k]) for k, v in b.net.state_dict().items())
        assert torch.equal(b.generator.get_state(), a.generator.get_state())
        sa, sb = a.optimizer.state_dict(), b.optimizer.state_dict()
        assert sorted(sb["state"]) == sorted(sa["state"])
        for i in sa["state"]:
            assert float(sb["state"][i]["step"]) == float(sa["state"][i]["step"]) == 2.0
            assert torch.equal(sb["state"][i]["exp_avg"], sa["state"][i]["exp_avg"]) and torch.equal(sb["state"][i]["exp_avg_sq"], sa["state"][i]["exp_avg_sq"])
        b.save(4)
        again = torch.load(str(tmp_path / kind / "checkpoints" / "SuperGlue_epoch_4.pth"), map_location="cpu")
        assert list(again) == list(ckpt) and again["epoch"] == 4
        assert all(torch.equal(again["optimizer"]["state"][i]["exp_avg"], sa["state"][i]["exp_avg"]) for i in sa["state"])
    # a checkpoint of the reference: two keys; the optimiser starts fresh
    torch.save({"epoch": 9, "net": a.net.state_dict()}, str(tmp_path / "reference.pth"))
    c = trainer("flat")
    before = c.generator.get_state()
    assert c.resume(tmp_path / "reference.pth") == 9
    assert c.optimizer.state_dict()["state"] == {} and torch.equal(c.generator.get_state(), before)
    with pytest.raises(ValueError):
        trainer("sgd")


def test_resume_arithmetic():
    from image_matching_amd.superglue.train_loop import epoch_order, epochs_to_run, global_step
    assert list(epochs_to_run(0, 3)) == [1, 2, 3] and list(epochs_to_run(2, 3)) == [3] and list(epochs_to_run(3, 3)) == []
    # the reference's len(train_loader) * (epoch - 1) + i + 1
    assert global_step(1, 4, 10) == 5 and global_step(3, 9, 10) == 30
    # the shuffle: a run resumed with the generator's state draws the orders the uninterrupted run draws
    g = torch.Generator().manual_seed(4)
    first = epoch_order(9, g, True)
    state = g.get_state()
    second = epoch_order(9, g, True)
    assert sorted(first) == sorted(second) == list(range(9)) and first != list(range(9))
    h = torch.Generator()
    h.set_state(state)
    assert epoch_order(9, h, True) == second
    assert epoch_order(4, g, False) == [0, 1, 2, 3] and torch.equal(g.get_state(), h.get_state()), "no draw without the shuffle"


def test_the_dropin_still_raises_and_the_writer_is_shared():
    """SuperGlue.train() of the drop-in raises as pinned; both training scripts use one JsonlWriter"""
    import superpoint_train_descriptor as sp_script
    from image_matching_amd import scalars
    from image_matching_amd.superglue.models.superglue_train import SuperGlue
    assert sp_script.JsonlWriter is scalars.JsonlWriter and sp_script.make_writer is scalars.make_writer
    with pytest.raises(NotImplementedError):
        SuperGlue.train(object.__new__(SuperGlue), True)
