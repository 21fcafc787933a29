"""The restatements of tests/sppool_ref.py against torch on the CPU, the network fixtures against the restated network, and the parts of
the trainable SuperPoint that need no GPU: the pooling scan equals F.max_pool2d(return_indices=True) and its autograd bit for bit
(seeded maps, odd H and W, the nine special windows); the normalisation's closed forms equal torch.autograd of the reference's two lines
at 1e-9 + 1e-9 |ref| and central differences; tests/golden/spmodel_*.npz are reproduced in float64 by sppool_ref.Net, which is built from
the restated blocks, at the same bar; SuperPointTrainable's state_dict has the keys and shapes of synth.superpoint_bn_shapes; layout
errors are raised before anything is called.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv3grad_ref as R3
from tests import sppool_ref as RP
from tests import util

TIGHT = lambda ref: 1e-9 + 1e-9 * np.abs(np.asarray(ref, np.float64))


def bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def torch_pool(x, dy):
    """F.max_pool2d(return_indices=True) and its autograd on the CPU -> y, idx as 2 row + col, dx"""
    with torch.enable_grad():                            # (another test module may have turned gradients off for the process)
        xt = torch.from_numpy(x).requires_grad_(True)
        y, flat = F.max_pool2d(xt, 2, return_indices=True)
        dx, = torch.autograd.grad(y, xt, torch.from_numpy(dy))
    W = x.shape[3]
    idx = (((flat // W) % 2) * 2 + (flat % W) % 2).numpy().astype(np.uint8)
    return y.detach().numpy(), idx, dx.numpy()


@pytest.mark.parametrize("shape", [(1, 1, 2, 2), (2, 3, 9, 7), (1, 2, 8, 16), (3, 2, 3, 17), (2, 1, 16, 65), (1, 3, 31, 30)])
@pytest.mark.parametrize("relu_like", [False, True])
def test_pooling_restatement_equals_torch(shape, relu_like):
    x, dy = RP.pool_case(7, *shape, relu_like=relu_like)
    y, idx = RP.pool_forward(x)
    dx = RP.pool_backward(idx, dy, shape)
    ty, tidx, tdx = torch_pool(x, dy)
    assert bits(y, ty) and bits(idx, tidx) and bits(dx, tdx)
    assert idx.dtype == np.uint8 and idx.max() <= 3 and dx.shape == shape


def test_pooling_special_windows():
    """all equal, the three tie positions, NaN first, two NaNs, NaN before a larger value, all -inf, -0 before +0: the recorded index is
    the tabulated one and PyTorch's, y has PyTorch's bits (the sign of a zero and the payload of a NaN included), dx routes to it"""
    assert len(RP.SPECIAL_WINDOWS) == 9
    x = np.stack([np.array(w, np.float32).reshape(1, 2, 2) for _, w, _ in RP.SPECIAL_WINDOWS])          # (9,1,2,2)
    dy = np.arange(1, 10, dtype=np.float32).reshape(9, 1, 1, 1)
    y, idx = RP.pool_forward(x)
    assert idx.reshape(-1).tolist() == [want for _, _, want in RP.SPECIAL_WINDOWS]
    ty, tidx, tdx = torch_pool(x, dy)
    assert bits(y, ty) and bits(idx, tidx)
    dx = RP.pool_backward(idx, dy, x.shape)
    assert bits(dx, tdx)
    assert np.signbit(y[8, 0, 0, 0]) and np.isnan(y[4:7]).all() and y[7, 0, 0, 0] == -np.inf
    # planted into a larger map: first window, last window, last partial row
    base, dyb = RP.pool_case(3, 3, 3, 9, 7)
    for where in (lambda H, W: (0, 0), lambda H, W: (H // 2 - 1, W // 2 - 1), lambda H, W: (H // 2 - 1, 0)):
        xs = RP.plant(base, where)
        y, idx = RP.pool_forward(xs)
        ty, tidx, tdx = torch_pool(xs, dyb)
        assert bits(y, ty) and bits(idx, tidx) and bits(RP.pool_backward(idx, dyb, xs.shape), tdx)


@pytest.mark.parametrize("shape", [(2, 3, 6), (1, 1, 5), (3, 64, 7), (2, 256, 12)])
def test_norm_restatement_equals_autograd(shape):
    x, dy = RP.l2_case(11, *shape)
    ours, theirs = RP.l2_reference(x, dy), RP.l2_autograd(x, dy)
    for k in ("y", "dx"):
        assert (np.abs(ours[k] - theirs[k]) <= TIGHT(theirs[k])).all(), k
    assert (np.abs(ours["norm"] - np.linalg.norm(x.astype(np.float64), axis=1)) <= TIGHT(ours["norm"])).all()
    assert np.allclose((ours["y"] ** 2).sum(1), 1.0, atol=1e-12)


def test_norm_restatement_equals_central_differences():
    x, dy = (a.astype(np.float64).reshape(2, 3, 6) for a in RP.l2_case(13, 2, 3, 2 * 3))
    dx = RP.l2_reference(x, dy)["dx"]
    f = lambda v: float((RP.l2_reference(v, dy)["y"] * dy).sum())
    h = 1e-6
    num = np.zeros_like(x)
    for i in np.ndindex(*x.shape):
        e = np.zeros_like(x)
        e[i] = h
        num[i] = (f(x + e) - f(x - e)) / (2 * h)
    assert (np.abs(num - dx) <= 1e-6 + 1e-6 * np.abs(dx)).all()


def test_norm_zero_vector_is_nan_in_its_own_pixel():
    x, dy = RP.l2_case(17, 2, 5, 4)
    x[1, :, 2] = 0
    r = RP.l2_reference(x, dy)
    bad = np.zeros((2, 4), bool)
    bad[1, 2] = True
    for k in ("y", "dx"):
        assert (np.isnan(r[k]) == bad[:, None, :]).all(), k


@pytest.mark.parametrize("name", list(RP.NET_CASES))
def test_fixtures_are_reproduced_by_the_restated_net(name):
    """sppool_ref.Net from the restated blocks, in float64, gives what the reference's blocks wrote: samples, sums, buffers, the eval
    outputs and the Adam losses, at 1e-9 + 1e-9 |ref|; the seed rule holds at the recorded seed"""
    g = util.golden(f"spmodel_{name}.npz")
    seed = int(g["seed"])
    assert len(g["refused"]) == len(g["refused_why"]) < 400
    make = lambda train=True: RP.load_net(RP.Net(RP.D_NET), seed, torch.float64).train(train)
    x, dy_s, dy_d, t_s, t_d = (torch.from_numpy(a).double() for a in RP.net_case(seed, name))
    assert tuple(x.shape) == RP.NET_CASES[name]
    assert RP.unsafe(make(), x) == (0, 0, 0)
    m = make()
    res = RP.net_grads(m, x, dy_s, dy_d)
    names = [str(n) for n in g["names"]]
    assert names == list(res) and len(names) == 51
    for i, key in enumerate(names):
        a = res[key].numpy()
        ref = g[f"{i}_g"]
        assert (np.abs(a.reshape(-1)[RP.net_positions(i, a.size)] - ref) <= TIGHT(ref)).all(), key
        assert abs(a.sum() - g[f"{i}_sum"][0]) <= 1e-9 + 1e-9 * np.abs(a).sum(), key
    for i, (n, b) in enumerate(RP.net_buffers(m).items()):
        assert str(g["buffer_names"][i]) == n
        assert (np.abs(b - g[f"buffer_{i}"]) <= TIGHT(b)).all(), n
    with torch.no_grad():
        ev = make(False)(x)
    for i, key in enumerate(("semi", "desc")):
        a, ref = ev[key].numpy(), g[f"eval_{key}_g"]
        assert (np.abs(a.reshape(-1)[RP.net_positions(i, a.size)] - ref) <= TIGHT(ref)).all(), key
    if name == "even":
        losses = np.array(RP.adam_losses(make(), x, t_s, t_d))
        assert losses.shape == (RP.ADAM_STEPS,) and (np.abs(losses - g["adam_g"]) <= TIGHT(losses)).all()
        assert (np.diff(g["adam_g"]) < 0).all(), "the float64 losses decrease"
    else:
        assert "adam_g" not in g


@pytest.mark.parametrize("d", [64, 128, 256])
def test_trainable_keys_and_shapes(d):
    """state_dict() has exactly the keys and shapes of synth.superpoint_bn_shapes(d), in its order; building needs no GPU; a state dict
    of the restated network (the reference's layout) loads, bare or wrapped as the reference's training script wraps it"""
    from image_matching_amd import synth
    from image_matching_amd.engine import ImxError
    from image_matching_amd.sptrain_model import SuperPointTrainable
    m = SuperPointTrainable(None, descriptor_length=d)
    shapes = synth.superpoint_bn_shapes(d)
    sd = m.state_dict()
    assert list(sd) == list(shapes)
    assert all(tuple(sd[k].shape) == tuple(shapes[k]) for k in shapes)
    assert len(list(m.parameters())) == 48 and all(p.requires_grad for p in m.parameters())
    ref = RP.load_net(RP.Net(d), 5)
    assert list(ref.state_dict()) == list(sd)
    m.load_state_dict(ref.state_dict())
    m.load_state_dict({"model_state_dict": ref.state_dict(), "n_iter": 3})
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), ref.state_dict().values()))
    with pytest.raises(ImxError, match="without an engine"):
        m(torch.zeros(1, 1, 16, 16))
    with pytest.raises(ImxError, match="form must be"):
        SuperPointTrainable(None, form="slabs")


def test_layout_errors_come_before_any_call():
    """down_pooled checks the block's whole layout, the double_conv inside included, before the pooling runs: with no engine at all the
    error is the layout's"""
    from image_matching_amd import sptrain_net
    from image_matching_amd.engine import ImxError
    x = torch.zeros(1, 4, 8, 8)
    good = R3.Down(4, 8)
    with pytest.raises(ImxError, match="down: expected"):
        sptrain_net.down_pooled(None, R3.DoubleConv(4, 8), x)
    bad_pool = R3.Down(4, 8)
    bad_pool.mpconv[0] = torch.nn.MaxPool2d(2, ceil_mode=True)
    with pytest.raises(ImxError, match="down: expected"):
        sptrain_net.down_pooled(None, bad_pool, x)
    bad_pool.mpconv[0] = torch.nn.MaxPool2d(3, stride=2)
    with pytest.raises(ImxError, match="down: expected"):
        sptrain_net.down_pooled(None, bad_pool, x)
    bad_conv = R3.Down(4, 8)
    bad_conv.mpconv[1].conv[3] = torch.nn.Conv2d(8, 8, 5, padding=2)
    with pytest.raises(ImxError, match="double_conv: expected"):
        sptrain_net.down_pooled(None, bad_conv, x)
    # a good layout gets as far as the tensor check: a CPU tensor is refused, nothing is copied
    with pytest.raises(ImxError, match="maxpool2: x must be a contiguous fp32 cuda tensor"):
        sptrain_net.down_pooled(None, good, x)
    with pytest.raises(ImxError, match="l2norm: x must be a contiguous fp32 cuda tensor"):
        sptrain_net.normalize_descriptors(None, x)
