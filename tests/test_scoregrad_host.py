"""tests/scoregrad_ref.py, the project's restatement of the score product and its derivative, against torch.einsum and torch.autograd in
float64 on the CPU; and the trainable model's modules (image_matching_amd.sgtrain_model.build_modules), whose state_dict has to be the
reference's key for key.  No GPU."""
import numpy as np
import pytest
import torch

from tests import scoregrad_ref as R

# (B, D, N0, N1, n0, n1): the shapes of tests/test_gpu_scoregrad.py
CASES = [(1, 64, 70, 100, None, None), (2, 160, 130, 150, None, None), (1, 1, 33, 1, None, None), (1, 3, 1, 65, None, None),
         (3, 64, 48, 80, (40, 0, 48), (70, 9, 80)), (2, 5, 7, 9, (9, -1), (3, 100))]


@pytest.mark.parametrize("B,D,N0,N1,n0,n1", CASES)
def test_restatement_against_einsum_and_autograd(B, D, N0, N1, n0, n1):
    """on the valid block of every pair the three closed forms equal einsum + autograd in float64 to rounding; elsewhere they are 0 and
    NaN on the padding is never read"""
    a, b, ds = R.case(11 + B + D, B, D, N0, N1)
    c0, c1 = R._counts(n0, B, N0), R._counts(n1, B, N1)
    if n0 is not None:
        a, b = R.ragged_pad(a, (c0,), (N0,), (2,)), R.ragged_pad(b, (c1,), (N1,), (2,))
        ds = R.ragged_pad(ds, (c0, c1), (N0, N1), (1, 2))
    got = R.batch_reference(a, b, ds, n0, n1)
    want = R.ragged_autograd(a, b, ds, c0, c1)
    for key in ("scores", "da", "db"):
        assert np.isfinite(got[key]).all(), key
        assert np.all(np.abs(got[key] - want[key]) <= 1e-12 + 1e-12 * np.abs(want[key])), key
    for p in range(B):
        assert not got["scores"][p, c0[p]:].any() and not got["scores"][p, :, c1[p]:].any()
        assert not got["da"][p, :, c0[p]:].any() and not got["db"][p, :, c1[p]:].any()
        if c0[p] == 0 or c1[p] == 0:
            assert not got["scores"][p].any() and not got["da"][p].any() and not got["db"][p].any()


def test_scale_is_a_plain_factor():
    a, b, ds = R.case(5, 1, 16, 9, 11)
    one, three = R.batch_reference(a, b, ds, scale=1.0), R.batch_reference(a, b, ds, scale=-3.0)
    assert all(np.allclose(three[k], -3.0 * one[k], rtol=1e-15, atol=0) for k in one)
    dflt = R.batch_reference(a, b, ds)
    assert all(np.allclose(dflt[k], 0.25 * one[k], rtol=1e-15, atol=0) for k in one)
    want = R.autograd(a, b, ds, scale=-3.0)
    assert all(np.allclose(three[k], want[k], rtol=1e-12, atol=1e-12) for k in one)


# ---------------------------------------------------------------------------------------------- the restated model against the reference's fixture
def frac64(a, ref):
    """the worst fraction of 1e-9 + 1e-9 |ref|"""
    return float(np.max(np.abs(np.asarray(a, np.float64) - ref) / (1e-9 + 1e-9 * np.abs(ref))))


def test_restated_model_against_the_reference_fixture():
    """tests/scoregrad_ref.py: SuperGlue at the fixture's seed in float64 against what the reference's own model wrote
    (tests/golden/make_golden_sgmodel.py): the loss and all 41 gradients (samples and sums), the BatchNorm buffers after the step, the
    matches, the matching scores, the top-two margins and the losses of 4 Adam steps, at 1e-9 + 1e-9 |ref|"""
    from tests import util
    from tests.golden.make_golden_sgmodel import ADAM_LR, ADAM_STEPS, positions
    g = util.golden("sgmodel_step.npz")
    seed = int(g["seed"])
    pair = R.as_pair(R.model_case(seed))
    model = R.load_parameters(R.SuperGlue().train(), seed, torch.float64)
    losses, grads, Zs = R.model_step(model, [pair])
    names = [str(n) for n in g["names"]]
    assert len(names) == 42 and set(names) == {"loss"} | set(grads)
    got = dict(grads, loss=losses)
    worst = 0.0
    for i, name in enumerate(names):
        a = got[name]
        worst = max(worst, frac64(a.reshape(-1)[positions(i, a.size)], g[f"{name}_g"]), frac64(a.sum(keepdims=True).reshape(1), g[f"{name}_sum"]))
    buffers = R.model_buffers(model)
    assert [str(n) for n in g["buffer_names"]] == list(buffers)
    for i, b in enumerate(buffers.values()):
        worst = max(worst, frac64(b, g[f"buffer_{i}"]))
    assert all(int(b) == 2 for n, b in buffers.items() if n.endswith("num_batches_tracked")), "each module runs once per image"
    m0, m1, ms0, ms1 = R.matches_of(Zs[0], R.MODEL_CONFIG["match_threshold"])
    assert np.array_equal(m0.numpy(), g["matches0"]) and np.array_equal(m1.numpy(), g["matches1"])
    margin0, margin1 = R.top_two_margins(Zs[0])
    worst = max(worst, frac64(ms0.numpy(), g["mscores0_g"]), frac64(ms1.numpy(), g["mscores1_g"]), frac64(margin0.numpy(), g["margin0"]),
                frac64(margin1.numpy(), g["margin1"]))
    fresh = R.load_parameters(R.SuperGlue().train(), seed, torch.float64)
    assert float(g["adam_lr"]) == ADAM_LR
    worst = max(worst, frac64(R.adam_losses(fresh, [pair], ADAM_STEPS, ADAM_LR), g["adam_losses"]))
    print(f"the restated model uses {worst:.3g} of 1e-9 + 1e-9 |ref|")
    assert worst <= 1.0


def test_one_pair_alone_and_in_a_list():
    """a list of pairs shares nothing but the BatchNorm statistics: in .eval() mode each pair's loss in a list equals its loss alone"""
    pairs = [R.as_pair(R.model_case(5, N0=17, N1=12, planted=6)), R.as_pair(R.model_case(6, N0=9, N1=21, planted=4))]
    model = R.load_parameters(R.SuperGlue().eval(), 5, torch.float64)
    with torch.no_grad():
        both = [l.item() for l in model(pairs)[0]]
        alone = [model([p])[0][0].item() for p in pairs]
    assert np.allclose(both, alone, rtol=1e-12, atol=0)


# ---------------------------------------------------------------------------------------------- the trainable model's parameters
def test_trainable_model_has_the_reference_state_dict():
    """SuperGlueTrainable builds without an engine (and without a GPU) as far as its parameters go: state_dict has exactly the keys and
    shapes of synth.superglue_shapes, the reference's checkpoint forms load, the restated model's state_dict loads, the initialisation
    follows the reference's rules, and a head dimension the attention kernels do not have is refused at construction"""
    from image_matching_amd import synth
    from image_matching_amd.engine import ImxError
    from image_matching_amd.sgtrain_model import SuperGlueTrainable, build_modules
    model = SuperGlueTrainable(R.MODEL_CONFIG)
    sd, shapes = model.state_dict(), synth.superglue_shapes(64, [32, 64], 2)
    assert set(sd) == set(shapes) and all(tuple(sd[k].shape) == tuple(shapes[k]) for k in shapes)
    assert len(list(model.parameters())) == 41 and all(p.requires_grad for p in model.parameters())
    assert float(model.bin_score) == 1.0 and not model.kenc.encoder[-1].bias.any()
    for layer in model.gnn.layers:
        assert not layer.mlp[-1].bias.any()
        assert all(torch.equal(p.weight, layer.attn.merge.weight) and torch.equal(p.bias, layer.attn.merge.bias) for p in layer.attn.proj)
    restated = R.load_parameters(R.SuperGlue(), 3)
    model.load_state_dict(restated.state_dict())                         # plain
    assert all(torch.equal(v, restated.state_dict()[k]) for k, v in model.state_dict().items())
    other = SuperGlueTrainable(R.MODEL_CONFIG)
    other.load_state_dict({"net": restated.state_dict(), "epoch": 7})   # as the training script saves it
    assert all(torch.equal(v, restated.state_dict()[k]) for k, v in other.state_dict().items())
    restated.load_state_dict(model.state_dict())                         # and back
    with pytest.raises(RuntimeError):
        model.load_state_dict({"bin_score": torch.tensor(1.)})
    with pytest.raises(ImxError, match="16, 32 or 64"):
        SuperGlueTrainable({"descriptor_dim": 96})
    with pytest.raises(ImxError, match="16, 32 or 64"):
        build_modules({**R.MODEL_CONFIG, "descriptor_dim": 32})
    full = SuperGlueTrainable({})                                        # the default configuration: d = 256, 18 layers
    assert set(full.state_dict()) == set(synth.superglue_shapes(256, [32, 64, 128, 256], 18))
    with pytest.raises(ImxError, match="without an engine"):
        model.forward_pairs(*[None] * 10)


def test_inference_dropin_takes_the_trainable_state_dict():
    """superglue_test.SuperGlue.load_state_dict(trainable.state_dict()) succeeds (the keys and shapes are checked on the host; the
    upload happens at the first forward)"""
    from image_matching_amd.sgtrain_model import SuperGlueTrainable
    from image_matching_amd.superglue.models.superglue_test import SuperGlue
    model = SuperGlueTrainable(R.MODEL_CONFIG)
    SuperGlue({**R.MODEL_CONFIG, "weights": None}).load_state_dict(model.state_dict())
