"""BatchNorm1d + ReLU of SuperGlue's MLPs in their training form on the GPU (imx_bn_relu_forward_train, imx_bn_relu_backward,
Engine.bn_relu_forward_train, Engine.bn_relu_backward, image_matching_amd.sgtrain_grad.batchnorm_relu / mlp / keypoint_encoder /
gnn_layer) against the project's restatement in float64 (tests/bngrad_ref.py, itself held to the reference's autograd by
tests/test_bngrad_host.py) and against the samples and per-channel sums the reference's own MLP, KeypointEncoder and
AttentionalPropagation wrote under torch.autograd (tests/golden/make_golden_bngrad.py, make_golden_lingrad.py).  The default bar,
element-wise: |x - x64| <= max(1e-4 + 1e-4 |x64|, 2.5 |ref32 - x64|); where the reference's fp32 result is not at hand (full tensors, sums)
the first term alone, except at the long sums, whose second term is the fp32 restatement's.

The mask rule, for shapes whose seed was not selected: ReLU's derivative jumps at z = 0, so with K = {|z64| < 1e-5} the kernel's mask
y > 0 must equal float64's outside K, |K| <= 4 + 4e-5 elements (a condition on the inputs, about three times what they give), and the
gradients are compared with the restatement evaluated with the kernel's mask.  Every test prints the fractions of the bar it used.
Needs an MI355X; a few seconds per test."""
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import bngrad_ref as R
from tests import lingrad_ref as LR
from tests import util
from tests.golden.make_golden_bngrad import CASES, KENC, RAGGED_COUNTS, RAGGED_FRAME, TENSORS, channel_sums, kenc_positions, kenc_sums, sample_positions
from tests.golden.make_golden_lingrad import LAYER, layer_positions

pytestmark = pytest.mark.gpu
OUTPUTS = ("y", "mean", "rstd", "dx", "dgamma", "dbeta")


def new_engine():
    from image_matching_amd.engine import Engine
    return Engine(util.sp_config(128, 256), util.sg_config(128), "cuda")


@pytest.fixture(scope="module")
def eng():
    return new_engine()


def cuda(a, dtype=torch.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def call(eng, x, gamma, beta, dy, n=None, training=True, rm=None, rv=None, nbt=False, want=(True, True, True), eps=R.EPS, momentum=R.MOMENTUM):
    """forward, then backward with the forward's mean and rstd -> dict of numpy arrays: y, mean, rstd, those of dx, dgamma, dbeta that
    were wanted, and the running statistics / num_batches_tracked after the call where they were given"""
    x, gamma, beta, dy, n, rm, rv = cuda(x), cuda(gamma), cuda(beta), cuda(dy), cuda(None if n is None else np.asarray(n), torch.int32), cuda(rm), cuda(rv)
    count = torch.zeros(1, dtype=torch.int64, device="cuda") if nbt else None
    res = dict(eng.bn_relu_forward_train(x, gamma, beta, rm, rv, count, n=n, training=training, momentum=momentum, eps=eps))
    res.update(eng.bn_relu_backward(x, gamma, beta, res["mean"], res["rstd"], dy, n=n, training=training, want=want))
    for key, t in (("running_mean", rm), ("running_var", rv), ("nbt", count)):
        if t is not None:
            res[key] = t
    torch.cuda.synchronize()
    return {key: t.cpu().numpy() for key, t in res.items()}


@functools.lru_cache(maxsize=None)
def seeded(seed, B, C, N):
    """the inputs of a seeded case, computed once and shared (read only)"""
    return R.case(seed, B, C, N)


def bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def same_bits(a, b, keys=OUTPUTS):
    return all(bits(a[k], b[k]) for k in keys if k in a and k in b)


def frac64(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref) / (1e-5 + 1e-5 * np.abs(ref))))


def show(what, f):
    print(f"{what}: of the bar -- " + ", ".join(f"{t} {v:.3g}" for t, v in f.items()))


def held(what, res, inputs, n=None, training=True, rm=None, rv=None, with_fp32=False):
    """the mask rule and the fractions of the bar of y, mean, rstd, dx, dgamma, dbeta against the float64 restatement (the gradients with
    the kernel's mask; with_fp32: the second term from the fp32 restatement with the same mask)"""
    x, gamma, beta, dy = inputs
    ref = R.batch_reference(x, gamma, beta, dy, n, training, rm, rv)
    K = R.kink(ref["z"], n)
    mask = res["y"] > 0
    elements = x.shape[1] * sum(R._counts(n, x.shape[0], x.shape[2]))
    assert np.array_equal(mask[~K], (ref["z"] > 0)[~K]), f"{what}: the mask differs from float64's away from the kink"
    assert K.sum() <= 4 + 4e-5 * elements, f"{what}: {int(K.sum())} elements within 1e-5 of the kink"
    if not np.array_equal(mask, ref["z"] > 0):
        ref.update(zip(("dx", "dgamma", "dbeta"), R.backward(x, gamma, beta, ref["mean"], ref["rstd"], dy, n, training, mask)))
    ref32 = R.batch_reference(x, gamma, beta, dy, n, training, rm, rv, mask=mask, dtype=torch.float32) if with_fp32 else None
    f = {}
    for t in OUTPUTS:
        if t in res:
            d32 = None if ref32 is None or t == "y" else ref32[t] - ref[t]
            f[t] = float(np.max(np.abs(res[t].astype(np.float64) - ref[t]) / R.bar(ref[t], d32)))
    show(f"{what} ({int(K.sum())} of {elements} elements at the kink)", f)
    return f


# ---------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("name", list(CASES))
def test_reference_fixtures(eng, name):
    """samples (with the reference's fp32 term) and per-channel sums (first term) against the reference's float64 autograd, the running
    statistics after the step at 1e-5 + 1e-5 |ref|.  The ragged case runs as one NaN-padded batch of three in a frame of 64 and is
    compared with the reference's BatchNorm on the valid columns concatenated."""
    g = util.golden(f"bngrad_{name}.npz")
    seed, (B, C, N), training = int(g["seed"]), (int(v) for v in g["shape"]), CASES[name][2]
    x, gamma, beta, dy = R.case(seed, B, C, N)
    rm, rv = R.running(seed, C) if not training else (np.zeros(C, np.float32), np.ones(C, np.float32))
    n = None
    if name == "ragged":
        x, dy, n = R.ragged_pad(x, RAGGED_COUNTS, RAGGED_FRAME), R.ragged_pad(dy, RAGGED_COUNTS, RAGGED_FRAME), RAGGED_COUNTS
    res = call(eng, x, gamma, beta, dy, n, training, rm, rv, nbt=True)
    assert all(np.isfinite(a).all() for a in res.values()), "NaN padding leaked"
    if name == "ragged":
        for b, cnt in enumerate(RAGGED_COUNTS):
            assert not res["y"][b, :, cnt:].any() and not res["dx"][b, :, cnt:].any()
        res.update({t: R.ragged_cat(res[t], RAGGED_COUNTS) for t in ("y", "dx")})
    worst = {}
    for t in TENSORS:
        got = res[t].astype(np.float64)
        pos = sample_positions(name, t, got.size)
        worst[t] = (float(np.max(np.abs(got.reshape(-1)[pos] - g[f"{t}_g"]) / R.bar(g[f"{t}_g"], g[f"{t}_d32"]))),
                    float(np.max(np.abs(channel_sums(t, got) - g[f"{t}_sum"]) / R.bar(g[f"{t}_sum"]))))
    fr = max(frac64(res["running_mean"], g["running_mean"]), frac64(res["running_var"], g["running_var"]))
    print(f"{name}: of the bar -- " + ", ".join(f"{t} samples {w_[0]:.3g} sums {w_[1]:.3g}" for t, w_ in worst.items())
          + f"; running statistics {fr:.3g} of 1e-5 + 1e-5 |ref|")
    assert max(max(w_) for w_ in worst.values()) <= 1.0 and fr <= 1.0
    assert int(res["nbt"][0]) == int(g["nbt"])


# (B, C, N): every value at least twice; partial waves, partial 256-strides, one value per channel and pair (B N = 1 is an error)
EDGES = [(2, 1, 1), (3, 33, 1), (1, 3, 2), (2, 33, 2), (3, 1, 63), (1, 3, 63), (2, 3, 64), (1, 33, 64), (3, 3, 65), (1, 1, 65), (2, 33, 255),
         (3, 1, 255), (1, 1, 256), (2, 3, 256), (3, 33, 257), (1, 3, 257), (2, 1, 1025), (3, 33, 1025)]


def test_edge_list_covers_every_value_twice():
    for axis, values in enumerate(((1, 2, 3), (1, 3, 33), (1, 2, 63, 64, 65, 255, 256, 257, 1025))):
        assert all(sum(e[axis] == v for e in EDGES) >= 2 for v in values) and {e[axis] for e in EDGES} == set(values)


@pytest.mark.parametrize("B,C,N", EDGES)
def test_edges(eng, B, C, N):
    """training and evaluation mode in full against the float64 restatement at the first term alone, under the mask rule"""
    inputs = seeded(100 + B + 3 * C + 7 * N, B, C, N)
    rm, rv = R.running(N, C)
    for training in (True, False):
        res = call(eng, *inputs, None, training, rm, rv)
        f = held(f"B={B} C={C} N={N} {'training' if training else 'evaluation'}", res, inputs, None, training, rm, rv)
        assert len(f) == 6 and max(f.values()) <= 1.0
        ref = R.forward(*inputs[:3], None, training, rm, rv)
        assert frac64(res["running_mean"], ref["running_mean"]) <= 1.0 and frac64(res["running_var"], ref["running_var"]) <= 1.0


@pytest.mark.parametrize("shape", [(1, 256, 1024), (4, 256, 1024), (8, 64, 600)])
def test_long_sums(eng, shape):
    """the workload's own shapes (the register form) and one frame of 24 slots per thread (the form that reads x again): the default bar,
    its second term from the fp32 restatement on the CPU, under the mask rule"""
    inputs = seeded(7, *shape)
    res = call(eng, *inputs)
    f = held(f"long sums {shape}", res, inputs, with_fp32=True)
    assert len(f) == 6 and max(f.values()) <= 1.0


# ---------------------------------------------------------------------------------------------- ragged batches and bits
RAGGED = (300, 5, 0)


def ragged_batch(frame, counts=RAGGED, C=5, fill=np.nan):
    x, gamma, beta, dy = seeded(40, 1, C, sum(counts))
    return (R.ragged_pad(x, counts, frame, fill), gamma, beta, R.ragged_pad(dy, counts, frame, fill)), np.array(counts, np.int32)


def test_ragged_batch_and_the_two_forms(eng):
    """three pairs with counts (300, 5, 0), NaN on the padding of x and dy, in a frame of 300 (the register form) and of 4100 (the form
    that reads x again): finite, 0 past the counts, held to the restatement, equal bits between the two frames, with and without the
    empty pair, and with the valid columns concatenated as one pair only up to the bar (another order of the sum)"""
    inputs, n = ragged_batch(300)
    res = call(eng, *inputs, n, rm=np.zeros(5, np.float32), rv=np.ones(5, np.float32))
    assert all(np.isfinite(a).all() for a in res.values()), "NaN padding leaked"
    f = held("ragged (300, 5, 0)", res, inputs, n, rm=np.zeros(5, np.float32), rv=np.ones(5, np.float32))
    assert max(f.values()) <= 1.0
    for b, cnt in enumerate(RAGGED):
        assert not res["y"][b, :, cnt:].any() and not res["dx"][b, :, cnt:].any(), b
    wide_inputs, _ = ragged_batch(4100)
    wide = call(eng, *wide_inputs, n, rm=np.zeros(5, np.float32), rv=np.ones(5, np.float32))
    assert all(bits(res[t], wide[t]) for t in ("mean", "rstd", "dgamma", "dbeta", "running_mean", "running_var")), "the frame does not enter the order"
    assert all(bits(res[t], wide[t][:, :, :300]) and not wide[t][:, :, 300:].any() for t in ("y", "dx"))
    without = call(eng, *(a[:2] if a.ndim == 3 else a for a in inputs), n[:2], rm=np.zeros(5, np.float32), rv=np.ones(5, np.float32))
    assert all(bits(res[t], without[t]) for t in ("mean", "rstd", "dgamma", "dbeta", "running_mean", "running_var")), "the empty pair adds nothing"
    assert all(bits(res[t][:2], without[t]) for t in ("y", "dx"))
    full = seeded(45, 2, 33, 90)
    assert same_bits(call(eng, *full), call(eng, *full, np.array([90, 90], np.int32))), "NULL means all"
    assert same_bits(call(eng, *full), call(eng, *full, np.array([91, 1 << 30], np.int32))), "counts are clamped to the frame"
    rm, rv = R.running(1, 33)
    empty = call(eng, *full, np.array([0, -3], np.int32), rm=rm, rv=rv, nbt=True)
    assert all(not empty[t].any() for t in OUTPUTS), "no valid column anywhere: zeros"
    assert bits(empty["running_mean"], rm) and bits(empty["running_var"], rv) and int(empty["nbt"][0]) == 0, "M = 0 leaves the running statistics"
    one = call(eng, *full, np.array([0, 1], np.int32), rm=rm, rv=rv)
    assert bits(one["running_var"], rv) and not bits(one["running_mean"], rm), "M = 1 with counts: var = 0, running_var untouched"
    assert np.array_equal(one["mean"], full[0][1, :, 0]) and np.allclose(one["rstd"], R.EPS ** -0.5, rtol=1e-6) and not one["dx"].any()


def test_the_form_is_reported_per_launch_and_does_not_leak(eng):
    """one handle with timing on: BatchNorm at (1, 2, 8) (one slot per thread: the register form), a 1x1 convolution, BatchNorm at
    (1, 2, 4097) (17 slots, past kBnSlots = 16: the form that reads x again).  The report names the form of each BatchNorm launch, and
    the convolution between them, whose launcher has one form and reports none, shows an empty one.  This records how the one
    form slot behind the training entry points behaves (run() resets it per launch); separate slots per stage would pass it too"""
    z = lambda *shape: torch.zeros(*shape, device="cuda")
    eng.timing_reset()
    eng.set_timing(True)
    try:
        eng.bn_relu_forward_train(z(1, 2, 8), z(2), z(2))
        eng.conv1x1_forward_train(z(1, 4, 8), z(2, 4), None)
        eng.bn_relu_forward_train(z(1, 2, 4097), z(2), z(2))
        rows = [(name, launches, form) for name, launches, _, form in eng.timing_report(forms=True)]
    finally:
        eng.set_timing(False)
        eng.timing_reset()
    assert rows == [("bn_relu_fwd", 1, "regs"), ("lin_fwd", 1, ""), ("bn_relu_fwd", 1, "reread")], rows


def test_equal_bits_between_calls_and_handles(eng):
    inputs, n = ragged_batch(300)
    first = call(eng, *inputs, n)
    assert same_bits(first, call(eng, *inputs, n)), "the same call twice"
    call(eng, *seeded(47, 3, 200, 600))                                  # a larger call in between
    assert same_bits(first, call(eng, *inputs, n)), "after a larger call on the same handle"
    other = new_engine()                                                 # a fresh handle, workspaces poisoned with NaN
    other.set_option("debug_poison", "nan")
    try:
        assert same_bits(first, call(other, *inputs, n)), "a second handle, debug_poison = nan"
    finally:
        other.set_option("debug_poison", "off")


def test_null_outputs_keep_the_bits(eng):
    """every subset of (dx, dgamma, dbeta) has the bits of the full call, in both modes and both forms"""
    for shape, training in (((2, 7, 130), True), ((2, 7, 130), False), ((3, 5, 2100), True)):
        inputs = seeded(48, *shape)
        rm, rv = R.running(48, shape[1])
        full = call(eng, *inputs, None, training, rm, rv)
        for want in itertools.product((False, True), repeat=3):
            only = call(eng, *inputs, None, training, rm, rv, want=want)
            assert {k for k in ("dx", "dgamma", "dbeta") if k in only} == {k for k, w_ in zip(("dx", "dgamma", "dbeta"), want) if w_}
            assert same_bits(full, only), (shape, training, want)


def test_masked_cotangent_gives_exact_zeros(eng):
    """dy non-zero (and NaN) only where y == 0: the mask of the backward equals y > 0 bit for bit, so dx, dgamma and dbeta are exactly 0"""
    for shape in ((2, 9, 300), (3, 4, 2100)):
        x, gamma, beta, dy = seeded(49, *shape)
        y = call(eng, x, gamma, beta, dy)["y"]
        off = y == 0
        assert 0.2 < off.mean() < 0.8
        masked = np.where(off, np.where(dy > 0, np.float32(np.nan), dy), np.float32(0))
        res = call(eng, x, gamma, beta, masked)
        assert not res["dx"].any() and not res["dgamma"].any() and not res["dbeta"].any(), shape


@pytest.mark.parametrize("shape", [(2, 4, 300), (2, 4, 4100)])
def test_constant_channel(eng, shape):
    """every value 3.7, beta = +-0.5 (no kink): the mean is formed around the channel's first value and the variance around the mean, so
    mean = 3.7, var = 0 and z = beta exactly -- asserted as bits, in place of the bar 1e-4 + 4 ulp(3.7) eps^(-1/2) |gamma| that a mean a
    few ulp off would need.  Everything is finite."""
    B, C, N = shape
    _, gamma, _, dy = seeded(50, B, C, N)
    x = np.full(shape, 3.7, np.float32)
    beta = np.array([0.5, -0.5, 0.5, -0.5], np.float32)
    res = call(eng, x, gamma, beta, dy, rm=np.zeros(C, np.float32), rv=np.ones(C, np.float32))
    assert all(np.isfinite(a).all() for a in res.values())
    assert bits(res["mean"], np.full(C, 3.7, np.float32)) and np.allclose(res["rstd"], R.EPS ** -0.5, rtol=1e-6)
    assert bits(res["y"], np.broadcast_to(np.maximum(beta, 0)[None, :, None], shape).astype(np.float32))
    assert np.allclose(res["running_mean"], 0.37, rtol=1e-6) and np.allclose(res["running_var"], 0.9, rtol=1e-6)
    ref = R.batch_reference(x.astype(np.float64), gamma, beta, dy)
    assert np.max(np.abs(res["dbeta"] - ref["dbeta"]) / R.bar(ref["dbeta"])) <= 1.0 and not res["dgamma"].any()
    assert not res["dx"][:, 1::2].any(), "the channels whose beta is negative are off"


# ---------------------------------------------------------------------------------------------- errors
def test_errors_are_reported_and_the_handle_survives(eng):
    from image_matching_amd.engine import ImxError
    z = lambda *s: torch.zeros(*s, device="cuda")
    for shape in ((0, 4, 3), (1, 0, 3), (1, 4, 0), (1, 1025, 1), (1, 1, (1 << 20) + 1)):     # each bound, through both entry points
        x = z(*shape)
        with pytest.raises(ImxError, match="bad shape"):
            eng.bn_relu_forward_train(x, z(shape[1]), z(shape[1]))
        with pytest.raises(ImxError, match="bad shape"):
            eng.bn_relu_backward(x, z(shape[1]), z(shape[1]), z(shape[1]), z(shape[1]), z(*shape))
    lib, x, c, y = eng.train, z(2, 4, 8), z(4), z(2, 4, 8)
    p = lambda t: None if t is None else t.data_ptr()
    err = lambda: eng.lib.imx_last_error(eng.handle)
    fwd = lambda B=2, C=4, N=8, train=1, eps=1e-5, mom=0.1, xx=x, g=c, b=c, rm=None, rv=None, yy=y, m=c, r=c: lib.imx_bn_relu_forward_train(
        eng.handle, B, C, N, train, eps, mom, p(xx), p(g), p(b), None, p(rm), p(rv), None, p(yy), p(m), p(r), None)
    for kw in ({"B": 65536}, {"B": 0}, {"C": 0}, {"C": 1025}, {"N": 0}, {"N": (1 << 20) + 1}):
        assert fwd(**kw) != 0 and b"bad shape" in err(), kw
    for kw in ({"eps": 0.0}, {"eps": -1.0}, {"mom": -0.1}, {"mom": 1.5}, {"eps": float("nan")}):
        assert fwd(**kw) != 0 and b"bad eps" in err(), kw
    for kw in ({"xx": None}, {"g": None}, {"b": None}, {"yy": None}, {"m": None}, {"r": None}):
        assert fwd(**kw) != 0 and b"null argument" in err(), kw
    assert fwd(train=0) != 0 and b"running statistics are required" in err()
    assert fwd(yy=x) != 0 and b"aliases" in err()
    assert fwd(B=1, N=1) != 0 and b"B N = 1" in err()
    assert fwd(B=1, N=1, train=0, rm=c, rv=c) == 0, "one value per channel is fine in evaluation mode"
    with pytest.raises(ImxError, match="B N = 1"):
        eng.bn_relu_forward_train(z(1, 4, 1), c, c)
    bwd = lambda xx=x, g=c, b=c, m=c, r=c, dy=y, dx=None: lib.imx_bn_relu_backward(eng.handle, 2, 4, 8, 1, p(xx), p(g), p(b), p(m), p(r), p(dy), None,
                                                                                 p(dx), None, None, None)
    for kw in ({"xx": None}, {"g": None}, {"b": None}, {"m": None}, {"r": None}, {"dy": None}):
        assert bwd(**kw) != 0 and b"null argument" in err(), kw
    assert bwd(dx=x) != 0 and b"aliases" in err()
    assert bwd() == 0, "nothing wanted: nothing launched"
    with pytest.raises(ImxError, match="contiguous fp32 cuda"):
        eng.bn_relu_forward_train(z(1, 3, 4).transpose(1, 2), z(4), z(4))
    with pytest.raises(ImxError, match=r"gamma must be \(4,\)"):
        eng.bn_relu_forward_train(z(1, 4, 3), z(5), z(4))
    with pytest.raises(ImxError, match="num_batches_tracked"):
        eng.bn_relu_forward_train(z(1, 4, 3), z(4), z(4), num_batches_tracked=z(1))
    inputs = seeded(51, 2, 5, 7)
    f = held("a valid call after the errors", call(eng, *inputs), inputs)
    assert max(f.values()) <= 1.0


# ---------------------------------------------------------------------------------------------- the bridge to autograd
@pytest.mark.parametrize("training", [True, False])
def test_batchnorm_relu_bridge(eng, training):
    """(B, C, N) = (2, 64, 300): loss.backward() through sgtrain_grad.batchnorm_relu and through PyTorch's own F.relu(bn(x)), both on the
    device and both held to the float64 restatement under the mask rule (each with its own mask) at the first term; the module's
    buffers after the step agree to 1e-5"""
    from image_matching_amd import sgtrain_grad
    inputs = seeded(9, 2, 64, 300)
    x, gamma, beta, dy = inputs
    rm, rv = R.running(9, 64)

    def run(fn):
        bn = torch.nn.BatchNorm1d(64).cuda().train(training)
        bn.load_state_dict({"weight": cuda(gamma), "bias": cuda(beta), "running_mean": cuda(rm), "running_var": cuda(rv)}, strict=False)
        xt = cuda(x).requires_grad_(True)
        with torch.enable_grad():
            y = fn(bn, xt)
            y.backward(cuda(dy))
        res = {"y": y.detach(), "dx": xt.grad, "dgamma": bn.weight.grad, "dbeta": bn.bias.grad}
        return {k: v.cpu().numpy() for k, v in res.items()}, bn

    ours, bn0 = run(lambda bn, t: sgtrain_grad.batchnorm_relu(eng, bn, t))
    theirs, bn1 = run(lambda bn, t: torch.relu(bn(t)))
    fo = held("bridge, sgtrain_grad.batchnorm_relu", ours, inputs, None, training, rm, rv)
    ft = held("bridge, F.relu(bn(x)) on the device", theirs, inputs, None, training, rm, rv)
    assert len(fo) == 4 and max(fo.values()) <= 1.0 and max(ft.values()) <= 1.0
    assert int(bn0.num_batches_tracked) == int(bn1.num_batches_tracked) == (1 if training else 0)
    assert torch.allclose(bn0.running_mean, bn1.running_mean, rtol=1e-5, atol=1e-5) and torch.allclose(bn0.running_var, bn1.running_var, rtol=1e-5, atol=1e-5)
    xt = cuda(x).requires_grad_(True)                                    # needs_input_grad: only x asks
    bn0.requires_grad_(False)
    sgtrain_grad.batchnorm_relu(eng, bn0, xt).sum().backward()
    assert xt.grad is not None and xt.grad.shape == xt.shape


def graded(ours, theirs, g, names, positions, sums=lambda name, a: a.sum(keepdims=True).reshape(1)):
    """per tensor: the samples at the default bar (the reference's own fp32 term), the fixture's sums (sums(name, array): per tensor or
    per channel) with the second term of the all-PyTorch module on this device -> (fractions of ours, fractions of theirs with the sums
    at the first term alone)"""
    fo, ft = {}, {}
    for i, name in enumerate(names):
        ref, ref_sum = g[f"{name}_g"], g[f"{name}_sum"]
        a, t = (res[name].cpu().numpy().astype(np.float64) for res in (ours, theirs))
        pos = positions(i, a.size)
        fo[name] = max(float(np.max(np.abs(a.reshape(-1)[pos] - ref) / R.bar(ref, g[f"{name}_d32"]))),
                       float(np.max(np.abs(sums(name, a) - ref_sum) / R.bar(ref_sum, sums(name, t) - ref_sum))))
        ft[name] = max(float(np.max(np.abs(t.reshape(-1)[pos] - ref) / R.bar(ref, g[f"{name}_d32"]))),
                       float(np.max(np.abs(sums(name, t) - ref_sum) / R.bar(ref_sum))))
    return fo, ft


def test_keypoint_encoder_and_mlp(eng):
    """the restated KeypointEncoder(128, [32, 64, 128]) in train mode with the fixture's seeded parameters on 70 keypoints:
    keypoint_encoder's output, dkpts, dscores and all 14 parameter gradients against the samples and per-channel sums the reference's
    module wrote, at the default bar (the three biases in front of a BatchNorm get their exact gradient, 0, from mlp(): asserted as
    bits); the three BatchNorm modules' buffers after the step against the fixture at 1e-5 + 1e-5 |ref|; mlp() on the formed cat has the
    same bits; in evaluation mode those biases' gradients are formed by the library and held to float64 at the first term"""
    from image_matching_amd import sgtrain_grad
    g = util.golden("bngrad_kenc.npz")
    seed, (_, d, layers, N) = int(g["seed"]), KENC
    mods = []
    for _ in range(3):
        m = R.KeypointEncoder(d, list(layers)).train()
        m.load_state_dict({k: torch.from_numpy(v) for k, v in R.kenc_parameters(seed, m).items()}, strict=False)
        mods.append(m.cuda())
    kpts, scores, dy = (cuda(a) for a in R.kenc_case(seed, N, d))
    ours = R.kenc_grads(mods[0], lambda a, b: sgtrain_grad.keypoint_encoder(eng, mods[0], a, b), kpts, scores, dy)
    theirs = R.kenc_grads(mods[1], mods[1], kpts, scores, dy)
    names = [str(n) for n in g["names"]]
    assert len(names) == 17 and set(names) == set(ours)
    fo, ft = graded(ours, theirs, g, names, kenc_positions, kenc_sums)
    show("kenc, keypoint_encoder", fo)
    show("kenc, all PyTorch on the device (sums at the first term alone)", ft)
    assert max(fo.values()) <= 1.0
    fr = 0.0
    for i, bn in enumerate(mod for mod in mods[0].encoder if isinstance(mod, torch.nn.BatchNorm1d)):
        assert int(bn.num_batches_tracked) == int(g["nbt"][i]) == 1
        fr = max(fr, frac64(bn.running_mean.cpu().numpy(), g[f"running_mean_{i}"]), frac64(bn.running_var.cpu().numpy(), g[f"running_var_{i}"]))
    print(f"kenc: the buffers after the step use {fr:.3g} of 1e-5 + 1e-5 |ref|")
    assert fr <= 1.0
    assert all(not ours[f"encoder.{i}.bias"].any() for i in (0, 3, 6)), "a bias in front of a training-mode BatchNorm: exactly 0"
    with torch.no_grad():
        cat = torch.cat([kpts.transpose(1, 2), scores.unsqueeze(1)], 1).contiguous()
        assert torch.equal(sgtrain_grad.mlp(eng, mods[2].encoder, cat), ours["out"]), "one source or two: the same bits"
    # evaluation mode (the running statistics the step above left): nothing cancels, every bias gradient comes from the library
    m64 = R.KeypointEncoder(d, list(layers))
    m64.load_state_dict({k: v.cpu() for k, v in mods[0].state_dict().items()})
    m64.double().eval()
    args64 = [torch.from_numpy(a).double() for a in R.kenc_case(seed, N, d)]
    ref = {}
    zs = R.bn_outputs(m64, lambda: ref.update(R.kenc_grads(m64, m64, *args64)))
    assert len(zs) == 3 and not any(R.kink(z.numpy()).any() for z in zs), "the seed keeps the evaluation-mode activations off the kink"
    mods[0].eval()
    got = R.kenc_grads(mods[0], lambda a, b: sgtrain_grad.keypoint_encoder(eng, mods[0], a, b), kpts, scores, dy)
    fe = {name: float(np.max(np.abs(got[name].cpu().numpy().astype(np.float64) - ref[name].numpy()) / R.bar(ref[name].numpy()))) for name in names}
    show("kenc, keypoint_encoder in evaluation mode (first term)", fe)
    assert max(fe.values()) <= 1.0 and all(got[f"encoder.{i}.bias"].any() for i in (0, 3, 6))


def test_gnn_layer(eng):
    """the restated AttentionalPropagation(128, 4) in train mode with the seeded parameters of lingrad_layer.npz (its seed has no element
    at the kink: tests/test_bngrad_host.py), x (1,128,70), source (1,128,100): gnn_layer's output, dx, dsource and all 14 parameter
    gradients against the samples the reference's module wrote, and the buffers after the step against the all-PyTorch layer to 1e-5"""
    from image_matching_amd import sgtrain_grad
    g = util.golden("lingrad_layer.npz")
    seed, d, heads, N, M = LAYER
    layers = []
    for _ in range(2):
        m = LR.AttentionalPropagation(d, heads).train()
        m.load_state_dict({k: torch.from_numpy(v) for k, v in LR.layer_parameters(seed, m).items()}, strict=False)
        layers.append(m.cuda())
    x, source, dy = (cuda(a) for a in LR.layer_case(seed, d, N, M))
    ours = LR.layer_grads(layers[0], lambda a, b: sgtrain_grad.gnn_layer(eng, layers[0], a, b), x, source, dy)
    theirs = LR.layer_grads(layers[1], layers[1], x, source, dy)
    names = [str(n) for n in g["names"]]
    assert len(names) == 17 and set(names) == set(ours)
    fo, ft = graded(ours, theirs, g, names, lambda i, size: layer_positions(seed, i, size))
    show("layer, gnn_layer", fo)
    show("layer, all PyTorch on the device (sums at the first term alone)", ft)
    assert max(fo.values()) <= 1.0
    bn0, bn1 = layers[0].mlp[1], layers[1].mlp[1]
    assert int(bn0.num_batches_tracked) == 1
    assert torch.allclose(bn0.running_mean, bn1.running_mean, rtol=1e-5, atol=1e-5) and torch.allclose(bn0.running_var, bn1.running_var, rtol=1e-5, atol=1e-5)


RAGGED_LAYER = (13, 64, 4, ((40, 70), (23, 9)), (48, 80))      # seed, d, heads, (n, m) per pair, the frame (N, M)


def ragged_layer_reference(module, xs, sources, dys):
    """the layer on each pair's valid columns, the BatchNorm statistics over all pairs' columns concatenated: attention and convolutions
    per pair, mlp[1:] on the concatenation -> dict name -> tensor (out, dx, dsource per pair in lists, one gradient per parameter)"""
    module.zero_grad()
    xs, sources = [t.clone().requires_grad_(True) for t in xs], [t.clone().requires_grad_(True) for t in sources]
    with torch.enable_grad():
        hidden = torch.cat([module.mlp[0](torch.cat([x, module.attn(x, s, s)], 1)) for x, s in zip(xs, sources)], 2)
        z = module.mlp[1](hidden)
        out = module.mlp[3](module.mlp[2](z))
        (out * torch.cat(dys, 2)).sum().backward()
    res = {"out": list(out.detach().split([x.shape[2] for x in xs], 2)), "dx": [x.grad for x in xs], "dsource": [s.grad for s in sources], "z": z.detach()}
    res.update({name: p.grad.clone() for name, p in module.named_parameters()})
    return res


def test_gnn_layer_on_a_ragged_batch(eng):
    """two pairs of (40, 70) and (23, 9) valid columns in a NaN-padded frame of (48, 80), d = 64, train mode: gnn_layer with the counts
    against the restated layer in float64 on each pair's valid columns with the BatchNorm statistics of the concatenation -- output, dx,
    dsource (0 on the padding) and all 14 parameter gradients at the default bar, its second term from the same restated layer in
    fp32 on the CPU; no element of the hidden activation lies at the kink (asserted)"""
    from image_matching_amd import sgtrain_grad
    seed, d, heads, counts, (N, M) = RAGGED_LAYER
    ref, mods = {}, {}
    for dtype in (torch.float64, torch.float32):
        m = mods[dtype] = LR.AttentionalPropagation(d, heads).train()
        params = {k: torch.from_numpy(v) for k, v in LR.layer_parameters(seed, m).items()}
        m.load_state_dict(params, strict=False)
        m.to(dtype)
        cases = [LR.layer_case(seed + b, d, n_, m_) for b, (n_, m_) in enumerate(counts)]
        ref[dtype] = ragged_layer_reference(m, *([torch.from_numpy(c[i]).to(dtype) for c in cases] for i in range(3)))
    r64, r32 = ref[torch.float64], ref[torch.float32]
    assert not R.kink(r64["z"].numpy()).any(), "the seed keeps the hidden activation off the kink"
    layer = LR.AttentionalPropagation(d, heads).train()
    layer.load_state_dict(params, strict=False)
    layer = layer.cuda()
    pad = lambda arrays, frame: cuda(np.concatenate([R.ragged_pad(a, [a.shape[2]], frame) for a in arrays], 0))
    x, source, dy = pad([c[0] for c in cases], N), pad([c[1] for c in cases], M), pad([c[2] for c in cases], N)
    n, ns = cuda(np.array([c[0] for c in counts]), torch.int32), cuda(np.array([c[1] for c in counts]), torch.int32)
    layer.zero_grad()
    x.requires_grad_(True), source.requires_grad_(True)
    with torch.enable_grad():
        out = sgtrain_grad.gnn_layer(eng, layer, x, source, n=n, ns=ns)
        out.backward(dy)
    got = {"out": out.detach(), "dx": x.grad, "dsource": source.grad}
    assert all(torch.isfinite(t).all() for t in got.values()), "NaN padding leaked"
    f = {}
    for name, t in got.items():
        for b, (n_, m_) in enumerate(counts):
            cnt = m_ if name == "dsource" else n_
            assert not t[b, :, cnt:].any(), (name, b)
            a, r = t[b:b + 1, :, :cnt].cpu().numpy().astype(np.float64), r64[name][b].numpy()
            f[name] = max(f.get(name, 0.0), float(np.max(np.abs(a - r) / R.bar(r, r32[name][b].double().numpy() - r))))
    for name, p in layer.named_parameters():
        a, r = p.grad.cpu().numpy().astype(np.float64), r64[name].numpy()
        f[name] = float(np.max(np.abs(a - r) / R.bar(r, r32[name].double().numpy() - r)))
    show("ragged layer, gnn_layer", f)
    assert len(f) == 17 and max(f.values()) <= 1.0
    bn, bn64 = layer.mlp[1], mods[torch.float64].mlp[1]
    fr = max(frac64(bn.running_mean.cpu().numpy(), bn64.running_mean.numpy()), frac64(bn.running_var.cpu().numpy(), bn64.running_var.numpy()))
    print(f"ragged layer: the buffers after the step use {fr:.3g} of 1e-5 + 1e-5 |ref|")
    assert fr <= 1.0 and int(bn.num_batches_tracked) == 1
