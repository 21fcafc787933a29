"""BatchNorm2d [+ ReLU] of SuperPoint's network in its training form on the GPU (imx_bn2d_forward_train, imx_bn2d_backward,
Engine.bn2d_forward_train, Engine.bn2d_backward, image_matching_amd.sptrain_net.bn2d / batchnorm2d / conv_bn_relu_form / double_conv_form / head) against
the project's restatement in float64 (tests/bn2d_ref.py over tests/bngrad_ref.py, held to the reference's autograd by
tests/test_bn2d_host.py) and against the samples and per-channel sums the reference's own double_conv wrote under torch.autograd
(tests/golden/make_golden_bn2d.py).  The default bar, element-wise: |x - x64| <= max(1e-4 + 1e-4 |x64|, 2.5 |ref32 - x64|); where the
reference's fp32 result is not at hand (full tensors, sums) the first term alone, except at the long sum, whose second term is the fp32
restatement's.

The mask rule, for shapes whose seed was not selected: ReLU's derivative jumps at z = 0, so with K = {|z64| < 1e-5} the kernel's mask
y > 0 must equal float64's outside K, |K| <= 4 + 4e-5 elements (a condition on the inputs), and the gradients are compared with the
restatement evaluated with the kernel's mask.  Every test prints the fractions of the bar it used.  Needs an MI355X; a few seconds per
test."""
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import bn2d_ref as R2
from tests import bngrad_ref as R
from tests import conv3grad_ref as R3
from tests import util
from tests.golden.make_golden_bn2d import CASES, TENSORS, channel_sums, head_positions, sample_positions
from tests.golden.make_golden_conv3grad import block_positions

pytestmark = pytest.mark.gpu
OUTPUTS = ("y", "mean", "rstd", "dx", "dgamma", "dbeta")
SLAB = 4096


def new_engine():
    from image_matching_amd.engine import Engine
    return Engine(util.sp_config(128, 256), util.sg_config(128), "cuda")


@pytest.fixture(scope="module")
def eng():
    return new_engine()


def cuda(a, dtype=torch.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def call(eng, x, gamma, beta, dy, relu=True, training=True, rm=None, rv=None, nbt=False, want=(True, True, True), eps=R.EPS, momentum=R.MOMENTUM):
    """forward, then backward with the forward's mean and rstd -> dict of numpy arrays: y, mean, rstd, those of dx, dgamma, dbeta that
    were wanted, and the running statistics / num_batches_tracked after the call where they were given"""
    x, gamma, beta, dy, rm, rv = (t if isinstance(t, torch.Tensor) else cuda(t) for t in (x, gamma, beta, dy, rm, rv))
    count = torch.zeros(1, dtype=torch.int64, device="cuda") if nbt else None
    res = dict(eng.bn2d_forward_train(x, gamma, beta, rm, rv, count, relu=relu, training=training, momentum=momentum, eps=eps))
    res.update(eng.bn2d_backward(x, gamma, beta, res["mean"], res["rstd"], dy, relu=relu, training=training, want=want))
    for key, t in (("running_mean", rm), ("running_var", rv), ("nbt", count)):
        if t is not None:
            res[key] = t
    torch.cuda.synchronize()
    return {key: t.cpu().numpy() for key, t in res.items()}


@functools.lru_cache(maxsize=None)
def seeded(seed, B, C, H, W):
    """the inputs of a seeded case, computed once and shared (read only)"""
    return R2.case(seed, B, C, H, W)


def bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def same_bits(a, b, keys=OUTPUTS):
    return all(bits(a[k], b[k]) for k in keys if k in a and k in b)


def frac64(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref) / (1e-5 + 1e-5 * np.abs(ref))))


def show(what, f):
    print(f"{what}: of the bar -- " + ", ".join(f"{t} {v:.3g}" for t, v in f.items()))


def held(what, res, inputs, relu=True, training=True, rm=None, rv=None, with_fp32=False):
    """the mask rule (with ReLU) and the fractions of the bar of y, mean, rstd, dx, dgamma, dbeta against the float64 restatement (the
    gradients with the kernel's mask; with_fp32: the second term from the fp32 restatement with the same mask)"""
    x, gamma, beta, dy = inputs
    ref = R2.batch_reference(x, gamma, beta, dy, relu, training, rm, rv)
    mask, at_kink = None, 0
    if relu:
        K = R2.kink(ref["z"])
        mask, at_kink = res["y"] > 0, int(K.sum())
        assert np.array_equal(mask[~K], (ref["z"] > 0)[~K]), f"{what}: the mask differs from float64's away from the kink"
        assert at_kink <= 4 + 4e-5 * x.size, f"{what}: {at_kink} elements within 1e-5 of the kink"
        if not np.array_equal(mask, ref["z"] > 0):
            ref = R2.batch_reference(x, gamma, beta, dy, relu, training, rm, rv, mask=mask)
    ref32 = R2.batch_reference(x, gamma, beta, dy, relu, training, rm, rv, mask=mask, dtype=torch.float32) if with_fp32 else None
    f = {}
    for t in OUTPUTS:
        if t in res:
            d32 = None if ref32 is None else ref32[t] - ref[t]
            f[t] = float(np.max(np.abs(res[t].astype(np.float64) - ref[t]) / R2.bar(ref[t], d32)))
    show(f"{what} ({at_kink} of {x.size} elements at the kink)", f)
    return f


# ---------------------------------------------------------------------------------------------- 1. the fixtures
@pytest.mark.parametrize("name", list(CASES))
def test_reference_fixtures(eng, name):
    """samples (with the reference's fp32 term) and per-channel sums (first term) against the reference's float64 autograd, the running
    statistics after the step at 1e-5 + 1e-5 |ref|, num_batches_tracked"""
    g = util.golden(f"bn2d_{name}.npz")
    _, shape, training, relu = CASES[name]
    seed, C = int(g["seed"]), shape[1]
    x, gamma, beta, dy = R2.case(seed, *shape)
    rm, rv = R.running(seed, C) if not training else (np.zeros(C, np.float32), np.ones(C, np.float32))
    res = call(eng, x, gamma, beta, dy, relu, training, rm, rv, nbt=True)
    worst = {}
    for t in TENSORS:
        got = res[t].astype(np.float64)
        pos = sample_positions(name, t, got.size)
        worst[t] = (float(np.max(np.abs(got.reshape(-1)[pos] - g[f"{t}_g"]) / R2.bar(g[f"{t}_g"], g[f"{t}_d32"]))),
                    float(np.max(np.abs(channel_sums(t, got) - g[f"{t}_sum"]) / R2.bar(g[f"{t}_sum"]))))
    fr = max(frac64(res["running_mean"], g["running_mean"]), frac64(res["running_var"], g["running_var"]))
    print(f"{name}: of the bar -- " + ", ".join(f"{t} samples {w_[0]:.3g} sums {w_[1]:.3g}" for t, w_ in worst.items())
          + f"; running statistics {fr:.3g} of 1e-5 + 1e-5 |ref|")
    assert max(max(w_) for w_ in worst.values()) <= 1.0 and fr <= 1.0
    assert int(res["nbt"][0]) == int(g["nbt"])


# ---------------------------------------------------------------------------------------------- 2. edges
# (B, C, HW): H W on either side of a wave (256 = 64 quads), of a stride of quads (1024) and of a slab (4096), and past two and three slabs
EDGES = [(2, 1, 1), (3, 3, 2), (1, 65, 3), (2, 3, 255), (1, 1, 256), (3, 65, 257), (1, 3, 1023), (2, 65, 1024), (3, 1, 1025), (1, 65, 4095),
         (2, 3, 4096), (3, 65, 4097), (2, 1, 8193), (1, 3, 12289), (3, 3, 8193)]
HWS = (1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8193, 12289)


def test_edge_list_covers_every_value():
    assert {e[2] for e in EDGES} == set(HWS) and {e[0] for e in EDGES} == {1, 2, 3} and {e[1] for e in EDGES} == {1, 3, 65}
    assert all(sum(e[0] == v for e in EDGES) >= 2 for v in (1, 2, 3)) and all(sum(e[1] == v for e in EDGES) >= 2 for v in (1, 3, 65))
    assert {HW % 4 for HW in HWS} == {0, 1, 2, 3}, "aligned and unaligned runs"


@pytest.mark.parametrize("B,C,HW", EDGES)
def test_edges(eng, B, C, HW):
    """both modes, with and without ReLU, in full against the float64 restatement at the first term alone, under the mask rule"""
    inputs = seeded(31 + (B + C + HW) % 9, B, C, 1, HW)
    rm, rv = R.running(HW, C)
    for training, relu in itertools.product((True, False), (True, False)):
        res = call(eng, *inputs, relu, training, rm, rv, nbt=True)
        f = held(f"B={B} C={C} HW={HW} {'training' if training else 'evaluation'}{' relu' if relu else ''}", res, inputs, relu, training, rm, rv)
        assert len(f) == 6 and max(f.values()) <= 1.0
        ref = R2.batch_reference(*inputs, relu, training, rm, rv)
        assert frac64(res["running_mean"], ref["running_mean"]) <= 1.0 and frac64(res["running_var"], ref["running_var"]) <= 1.0
        assert int(res["nbt"][0]) == (1 if training else 0)


# ---------------------------------------------------------------------------------------------- 3. the long sum
def test_long_sum(eng):
    """(16, 2, 240, 320): 1.2e6 values per channel, the M of the training shape, 19 slabs per map and 16 images; train mode with ReLU
    against float64 at the default bar, its second term from the fp32 restatement on the CPU, under the mask rule"""
    inputs = seeded(33, 16, 2, 240, 320)
    res = call(eng, *inputs)
    f = held("long sum (16, 2, 240, 320)", res, inputs, with_fp32=True)
    assert len(f) == 6 and max(f.values()) <= 1.0


# ---------------------------------------------------------------------------------------------- 4. the mask
def test_masked_cotangent_gives_exact_zeros(eng):
    """dy non-zero (and NaN) only where y == 0: the mask of the backward equals y > 0 bit for bit, so dx, dgamma and dbeta are exactly 0;
    without ReLU the same dy reaches the gradients"""
    for shape in ((2, 9, 15, 20), (3, 4, 70, 61)):
        x, gamma, beta, dy = seeded(49, *shape)
        y = call(eng, x, gamma, beta, dy)["y"]
        off = y == 0
        assert 0.2 < off.mean() < 0.8
        masked = np.where(off, np.where(dy > 0, np.float32(np.nan), dy), np.float32(0))
        res = call(eng, x, gamma, beta, masked)
        assert not res["dx"].any() and not res["dgamma"].any() and not res["dbeta"].any(), shape
        plain = call(eng, x, gamma, beta, masked, relu=False)
        assert np.isnan(plain["dbeta"]).all() and np.isnan(plain["dgamma"]).all() and np.isnan(plain["dx"]).any(), "without ReLU nothing is masked"
        finite = np.where(off, dy, np.float32(0))
        plain = call(eng, x, gamma, beta, finite, relu=False)
        ref = R2.batch_reference(x, gamma, beta, finite, relu=False)
        assert plain["dbeta"].any() and np.max(np.abs(plain["dbeta"] - ref["dbeta"]) / R2.bar(ref["dbeta"])) <= 1.0


# ---------------------------------------------------------------------------------------------- 5. a constant channel
@pytest.mark.parametrize("shape", [(2, 4, 1, 5000), (3, 4, 70, 61)])
def test_constant_channel(eng, shape):
    """every value 3.7 over two slabs and two or three images, beta = +-0.5 (no kink): a slab's mean is formed around its first pixel and
    the combine sees d = 0, so mean = 3.7, var = 0 and z = beta exactly -- asserted as bits, with and without ReLU"""
    B, C, H, W = shape
    assert H * W > SLAB
    _, gamma, _, dy = seeded(50, B, C, H, W)
    x = np.full(shape, 3.7, np.float32)
    beta = np.array([0.5, -0.5, 0.5, -0.5], np.float32)
    for relu in (True, False):
        res = call(eng, x, gamma, beta, dy, relu, rm=np.zeros(C, np.float32), rv=np.ones(C, np.float32))
        assert all(np.isfinite(a).all() for a in res.values())
        assert bits(res["mean"], np.full(C, 3.7, np.float32)) and bits(res["rstd"], (np.float32(1) / np.sqrt(np.full(C, R.EPS, np.float32))))
        z = np.broadcast_to(beta[None, :, None, None], shape).astype(np.float32)
        assert bits(res["y"], np.maximum(z, 0) if relu else z)
        assert np.allclose(res["running_mean"], 0.37, rtol=1e-6) and np.allclose(res["running_var"], 0.9, rtol=1e-6)
        assert not res["dgamma"].any()
        if relu:
            assert not res["dx"][:, 1::2].any(), "the channels whose beta is negative are off"


# ---------------------------------------------------------------------------------------------- 6. bits
def test_equal_bits_between_calls_handles_and_histories(eng):
    inputs = seeded(40, 3, 5, 70, 61)
    first = call(eng, *inputs)
    assert same_bits(first, call(eng, *inputs)), "the same call twice"
    call(eng, *seeded(47, 2, 33, 120, 160))                              # a larger call in between: the workspace grows
    call(eng, *seeded(48, 1, 7, 3, 5))
    assert same_bits(first, call(eng, *inputs)), "after other shapes on the same handle"
    other = new_engine()                                                 # a fresh handle, workspaces poisoned with NaN
    other.set_option("debug_poison", "nan")
    try:
        assert same_bits(first, call(other, *inputs)), "a second handle, debug_poison = nan"
    finally:
        other.set_option("debug_poison", "off")


def test_null_outputs_keep_the_bits(eng):
    """every subset of (dx, dgamma, dbeta) has the bits of the full call, in both modes, with and without ReLU"""
    for shape, training, relu in (((2, 7, 10, 13), True, True), ((2, 7, 10, 13), False, False), ((3, 5, 70, 61), True, False), ((3, 5, 70, 61), False, True)):
        inputs = seeded(48, *shape)
        rm, rv = R.running(48, shape[1])
        full = call(eng, *inputs, relu, training, rm, rv)
        for want in itertools.product((False, True), repeat=3):
            only = call(eng, *inputs, relu, training, rm, rv, want=want)
            assert {k for k in ("dx", "dgamma", "dbeta") if k in only} == {k for k, w_ in zip(("dx", "dgamma", "dbeta"), want) if w_}
            assert same_bits(full, only), (shape, training, relu, want)


def test_an_image_has_the_same_bits_in_any_batch_in_evaluation_mode(eng):
    x, gamma, beta, dy = seeded(52, 3, 6, 70, 61)
    rm, rv = R.running(52, 6)
    batch = call(eng, x, gamma, beta, dy, True, False, rm, rv)
    for b in range(3):
        alone = call(eng, x[b:b + 1], gamma, beta, dy[b:b + 1], True, False, rm, rv)
        assert bits(alone["y"][0], batch["y"][b]) and bits(alone["dx"][0], batch["dx"][b]), b


def forms_of(eng, fn):
    """the (kernel, form) rows the library reports for the launches of fn()"""
    eng.timing_reset()
    eng.set_timing(True)
    try:
        fn()
        return {(name, form) for name, _, _, form in eng.timing_report(forms=True)}
    finally:
        eng.set_timing(False)
        eng.timing_reset()


def test_the_16_byte_and_the_dword_form_give_the_same_bits(eng):
    """x, dy, y and dx one float into a larger allocation (runs that start 4 bytes past a 16-byte boundary: the dword form) against the
    aligned tensors (H W % 4 == 0: the 16-byte form); the library reports the form of every streaming launch"""
    B, C, H, W = 2, 5, 72, 60                                           # H W = 4320: two slabs, the second partial
    x, gamma, beta, dy = (cuda(a) for a in seeded(53, B, C, H, W))
    n = x.numel()

    def shifted(t):
        big = torch.empty(n + 8, device="cuda")
        v = big[1:1 + n].view(B, C, H, W)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v

    for training, relu in ((True, True), (False, False)):
        rm, rv = R.running(53, C)
        aligned, rows = {}, set()
        rows |= forms_of(eng, lambda: aligned.update(call(eng, x, gamma, beta, dy, relu, training, rm, rv)))
        assert {f for _, f in rows if f} == {"x4"}, rows
        xs, dys = shifted(x), shifted(dy)
        got = {}

        def run():
            fwd = eng.bn2d_forward_train(xs, gamma, beta, cuda(rm), cuda(rv), None, relu=relu, training=training)
            got.update(fwd)
            got.update(eng.bn2d_backward(xs, gamma, beta, fwd["mean"], fwd["rstd"], dys, relu=relu, training=training))
        rows = forms_of(eng, run)
        assert {f for _, f in rows if f} >= {"x1"} and ("bn2d_bwd_sums", "x1") in rows, rows
        torch.cuda.synchronize()
        assert same_bits(aligned, {k: v.cpu().numpy() for k, v in got.items()}), (training, relu)
    # the outputs misaligned as well, through the C ABI
    lib, p = eng.spnorm, lambda t: t.data_ptr()
    fwd = eng.bn2d_forward_train(x, gamma, beta)
    ys, dxs = shifted(torch.zeros_like(x)), shifted(torch.zeros_like(x))
    mean, rstd = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    assert lib.imx_bn2d_forward_train(eng.handle, B, C, H * W, 1, 1, R.EPS, 0.1, p(x), p(gamma), p(beta), None, None, None, p(ys), p(mean), p(rstd), None) == 0
    assert lib.imx_bn2d_backward(eng.handle, B, C, H * W, 1, 1, p(x), p(gamma), p(beta), p(mean), p(rstd), p(dy), p(dxs), None, None, None) == 0
    dx = eng.bn2d_backward(x, gamma, beta, fwd["mean"], fwd["rstd"], dy, want=(True, False, False))["dx"]
    torch.cuda.synchronize()
    assert torch.equal(ys.view(torch.int32), fwd["y"].view(torch.int32)) and torch.equal(dxs.view(torch.int32), dx.view(torch.int32))


# ---------------------------------------------------------------------------------------------- 7. offsets beyond 2^32
def test_offsets_beyond_32_bits(eng):
    """C = 1, H W = 2^24, B = 65, evaluation mode: the last image starts 4.3e9 bytes into x and y.  y of the last image equals, bit for
    bit and on the device, the same image run as B = 1"""
    B, HW = 65, 1 << 24
    free = torch.cuda.mem_get_info()[0]
    if free < 16 * 2 ** 30:
        print(f"skipped: {free / 2 ** 30:.1f} GiB free on the device, the test asks for 16 GiB (its allocator peak is about 9 GiB)")
        pytest.skip("not enough free device memory")
    gen = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(B, 1, 4096, 4096, device="cuda", generator=gen)
    assert (B - 1) * HW * 4 >= 2 ** 32, "every byte offset into the last image is 2^32 or more"
    gamma, beta, rm, rv = (torch.full((1,), v, device="cuda") for v in (1.25, -0.125, 0.5, 2.0))
    y = eng.bn2d_forward_train(x, gamma, beta, rm, rv, relu=True, training=False)["y"]
    y1 = eng.bn2d_forward_train(x[B - 1:].contiguous(), gamma, beta, rm, rv, relu=True, training=False)["y"]
    same = torch.equal(y[B - 1].view(torch.int32), y1[0].view(torch.int32))
    spread = float(y1.std())
    del x, y, y1
    torch.cuda.empty_cache()
    print(f"offsets: y {'equal' if same else 'DIFFERENT'}; std of y {spread:.3g}")
    assert same and spread > 0.2


# ---------------------------------------------------------------------------------------------- 8. errors
def test_errors_are_reported_and_the_handle_survives(eng):
    from image_matching_amd.engine import ImxError
    z = lambda *s: torch.zeros(*s, device="cuda")
    for shape in ((0, 4, 3, 3), (1, 0, 3, 3), (1, 4, 0, 3), (1, 1025, 1, 2)):          # through both Python entry points
        x = z(*shape)
        with pytest.raises(ImxError, match="bad shape"):
            eng.bn2d_forward_train(x, z(shape[1]), z(shape[1]))
        with pytest.raises(ImxError, match="bad shape"):
            eng.bn2d_backward(x, z(shape[1]), z(shape[1]), z(shape[1]), z(shape[1]), z(*shape))
    lib, x, c, y, dy = eng.spnorm, z(2, 4, 2, 4), z(4), z(2, 4, 2, 4), z(2, 4, 2, 4)
    m, r, rm, rv, c2 = z(4), z(4), z(4), z(4), z(8)
    p = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
    err = lambda: eng.lib.imx_last_error(eng.handle)
    fwd = lambda B=2, C=4, HW=8, relu=1, train=1, eps=1e-5, mom=0.1, xx=x, g=c, b=c, rm=None, rv=None, nbt=None, yy=y, mm=m, rr=r: \
        lib.imx_bn2d_forward_train(eng.handle, B, C, HW, relu, train, eps, mom, p(xx), p(g), p(b), p(rm), p(rv), p(nbt), p(yy), p(mm), p(rr), None)
    for kw in ({"B": 65536}, {"B": 0}, {"C": 0}, {"C": 1025}, {"HW": 0}, {"HW": (1 << 24) + 1}, {"B": 129, "HW": 1 << 24}):
        assert fwd(**kw) != 0 and b"bad shape" in err(), kw
    for kw in ({"eps": 0.0}, {"eps": -1.0}, {"mom": -0.1}, {"mom": 1.5}, {"eps": float("nan")}):
        assert fwd(**kw) != 0 and b"bad eps" in err(), kw
    for kw in ({"xx": None}, {"g": None}, {"b": None}, {"yy": None}, {"mm": None}, {"rr": None}):
        assert fwd(**kw) != 0 and b"null argument" in err(), kw
    assert fwd(train=0) != 0 and b"running statistics are required" in err()
    assert fwd(train=0, rm=rm) != 0 and b"running statistics are required" in err()
    assert fwd(B=1, HW=1) != 0 and b"B HW = 1" in err()
    for kw, text in (({"yy": x}, b"y aliases x"), ({"yy": x.data_ptr() + 4 * 60}, b"y aliases x"), ({"mm": c2, "rr": c2.data_ptr() + 4}, b"mean aliases rstd"),
                     ({"rm": c, "rv": rv}, b"running_mean aliases gamma"), ({"rm": rm, "rv": rm}, b"running_mean aliases running_var"),
                     ({"mm": y}, b"y aliases mean"), ({"nbt": r}, b"rstd aliases num_batches_tracked")):
        assert fwd(**kw) != 0 and text in err(), (kw, err())
    bwd = lambda B=2, C=4, HW=8, train=1, xx=x, g=c, b=c, mm=m, rr=r, d=dy, dx=None, dg=None, db=None: \
        lib.imx_bn2d_backward(eng.handle, B, C, HW, 1, train, p(xx), p(g), p(b), p(mm), p(rr), p(d), p(dx), p(dg), p(db), None)
    for kw in ({"B": 65536}, {"C": 1025}, {"HW": (1 << 24) + 1}, {"B": 129, "HW": 1 << 24}):
        assert bwd(**kw) != 0 and b"bad shape" in err(), kw
    for kw in ({"xx": None}, {"g": None}, {"b": None}, {"mm": None}, {"rr": None}, {"d": None}):
        assert bwd(**kw) != 0 and b"null argument" in err(), kw
    assert bwd(B=1, HW=1, dx=y) != 0 and b"B HW = 1" in err()
    for kw, text in (({"dx": x}, b"dx aliases x"), ({"dx": dy}, b"dx aliases dy"), ({"dg": c2, "db": c2.data_ptr() + 4}, b"dgamma aliases dbeta"),
                     ({"dg": c}, b"dgamma aliases gamma"), ({"db": m}, b"dbeta aliases mean"), ({"dx": y, "dg": y}, b"dx aliases dgamma")):
        assert bwd(**kw) != 0 and text in err(), (kw, err())
    assert bwd() == 0, "nothing wanted: nothing launched"
    torch.cuda.synchronize()
    assert not any(t.any() for t in (x, c, y, dy, m, r, rm, rv, c2)), "a refused call writes nothing"
    assert fwd(B=1, HW=1, train=0, rm=rm, rv=rv) == 0, "one value per channel is fine in evaluation mode"
    with pytest.raises(ImxError, match="B HW = 1"):
        eng.bn2d_forward_train(z(1, 4, 1, 1), c, c)
    with pytest.raises(ImxError, match="contiguous fp32 cuda"):
        eng.bn2d_forward_train(z(1, 3, 4, 5).transpose(2, 3), z(3), z(3))
    with pytest.raises(ImxError, match=r"gamma must be \(4,\)"):
        eng.bn2d_forward_train(z(1, 4, 3, 2), z(5), z(4))
    with pytest.raises(ImxError, match=r"dy must be \(1,4,3,2\)"):
        eng.bn2d_backward(z(1, 4, 3, 2), z(4), z(4), z(4), z(4), z(1, 4, 2, 3))
    with pytest.raises(ImxError, match="num_batches_tracked"):
        eng.bn2d_forward_train(z(1, 4, 3, 2), z(4), z(4), num_batches_tracked=z(1))
    with pytest.raises(ImxError, match="three flags"):
        eng.bn2d_backward(z(1, 4, 3, 2), z(4), z(4), z(4), z(4), z(1, 4, 3, 2), want=(True,))
    inputs = seeded(51, 2, 5, 3, 7)
    f = held("a valid call after the errors", call(eng, *inputs), inputs)
    assert max(f.values()) <= 1.0


# ---------------------------------------------------------------------------------------------- 9. the bridge to autograd
@pytest.mark.parametrize("training,relu", [(True, True), (True, False), (False, True), (False, False)])
def test_batchnorm2d_bridge(eng, training, relu):
    """(B, C, H, W) = (2, 64, 15, 20): loss.backward() through sptrain_net.batchnorm2d and through PyTorch's own bn(x) [F.relu], both on
    the device and both held to the float64 restatement under the mask rule (each with its own mask) at the first term; the module's
    buffers after the step agree to 1e-5"""
    from image_matching_amd import sptrain_net
    inputs = seeded(35, 2, 64, 15, 20)
    x, gamma, beta, dy = inputs
    rm, rv = R.running(9, 64)

    def run(fn):
        bn = torch.nn.BatchNorm2d(64).cuda().train(training)
        bn.load_state_dict({"weight": cuda(gamma), "bias": cuda(beta), "running_mean": cuda(rm), "running_var": cuda(rv)}, strict=False)
        xt = cuda(x).requires_grad_(True)
        with torch.enable_grad():
            y = fn(bn, xt)
            y.backward(cuda(dy))
        res = {"y": y.detach(), "dx": xt.grad, "dgamma": bn.weight.grad, "dbeta": bn.bias.grad}
        return {k: v.cpu().numpy() for k, v in res.items()}, bn

    ours, bn0 = run(lambda bn, t: sptrain_net.batchnorm2d(eng, bn, t, relu=relu))
    theirs, bn1 = run(lambda bn, t: torch.relu(bn(t)) if relu else bn(t))
    fo = held("bridge, sptrain_net.batchnorm2d", ours, inputs, relu, training, rm, rv)
    ft = held("bridge, bn(x) on the device", theirs, inputs, relu, training, rm, rv)
    assert len(fo) == 4 and max(fo.values()) <= 1.0 and max(ft.values()) <= 1.0
    assert int(bn0.num_batches_tracked) == int(bn1.num_batches_tracked) == (1 if training else 0)
    assert torch.allclose(bn0.running_mean, bn1.running_mean, rtol=1e-5, atol=1e-5) and torch.allclose(bn0.running_var, bn1.running_var, rtol=1e-5, atol=1e-5)
    xt = cuda(x).requires_grad_(True)                                    # needs_input_grad: only x asks
    bn0.requires_grad_(False)
    sptrain_net.batchnorm2d(eng, bn0, xt, relu=relu).sum().backward()
    assert xt.grad is not None and xt.grad.shape == xt.shape
    from image_matching_amd.engine import ImxError
    with pytest.raises(ImxError, match="bn must be nn.BatchNorm2d"):
        sptrain_net.batchnorm2d(eng, torch.nn.BatchNorm1d(64).cuda(), xt)
    with pytest.raises(ImxError, match="not supported"):
        sptrain_net.batchnorm2d(eng, torch.nn.BatchNorm2d(64, momentum=None).cuda(), xt)


def test_double_conv_in_the_pixels_form(eng):
    """the restated double_conv(3, 16) in train mode with the seeded state of conv3grad_block_double_conv.npz through
    sptrain_net.double_conv_form(form="pixels"): the output, dx and the 8 parameter gradients against the samples the reference's module
    wrote, at the bars of that fixture's own test; conv_bn_relu_form(form="pixels") twice has the same bits; form="auto", and
    double_conv() itself, have the bits of form="channel" (B H W = 240 < 4096)"""
    from image_matching_amd import sptrain_net
    g = util.golden("conv3grad_block_double_conv.npz")
    seed = int(g["seed"])
    x, dy = (cuda(a) for a in R3.block_case(seed, "double_conv"))
    blocks = [R3.load_block(R3.DoubleConv(*R3.BLOCKS["double_conv"][0]), seed).train().cuda() for _ in range(5)]
    res = {form: R3.block_grads(b, lambda a, b=b, form=form: sptrain_net.double_conv_form(eng, b, a, form=form), x, dy)
           for form, b in zip(("pixels", "channel", "auto"), blocks)}
    twice = R3.block_grads(blocks[3], lambda a: sptrain_net.conv_bn_relu_form(eng, blocks[3].conv[3], blocks[3].conv[4],
                                                                               sptrain_net.conv_bn_relu_form(eng, blocks[3].conv[0], blocks[3].conv[1], a, form="pixels"),
                                                                               form="pixels"), x, dy)
    plain = R3.block_grads(blocks[4], lambda a: sptrain_net.double_conv(eng, blocks[4], a), x, dy)
    names = [str(n) for n in g["names"]]
    assert len(names) == 10 and set(names) == set(res["pixels"])
    f = {}
    for i, name in enumerate(names):
        ref, ref_sum = g[f"{name}_g"], g[f"{name}_sum"]
        a = res["pixels"][name].cpu().numpy().astype(np.float64)
        pos = block_positions(seed, i, a.size)
        f[name] = max(float(np.max(np.abs(a.reshape(-1)[pos] - ref) / R3.bar(ref, g[f"{name}_d32"]))), float(np.max(np.abs(a.sum() - ref_sum) / R3.bar(ref_sum))))
        assert torch.equal(res["auto"][name], res["channel"][name]) and torch.equal(plain[name], res["channel"][name]), f"auto is channel below B H W = 4096: {name}"
        assert torch.equal(twice[name], res["pixels"][name]), name
    show("double_conv(form='pixels')", f)
    assert max(f.values()) <= 1.0
    convs = [m for m in blocks[0].modules() if isinstance(m, torch.nn.Conv2d)]
    assert len(convs) == 2 and all(c.bias.grad is not None and not c.bias.grad.any() for c in convs), "a bias before a training BatchNorm: exactly 0"
    fb = {}
    for i, (n, b) in enumerate(R3.block_buffers(blocks[0]).items()):
        ref = g[f"buffer_{i}"]
        if n.endswith("num_batches_tracked"):
            assert int(b) == int(ref) == 1
        else:
            fb[n] = float(np.max(np.abs(b - ref) / (1e-5 + 1e-5 * np.abs(ref))))
    show("double_conv(form='pixels'), buffers (of 1e-5 + 1e-5 |ref|)", fb)
    assert len(fb) == 4 and max(fb.values()) <= 1.0
    from image_matching_amd.engine import ImxError
    with pytest.raises(ImxError, match="form must be"):
        sptrain_net.double_conv_form(eng, blocks[0], x, form="rows")


def test_head(eng):
    """the restated head (conv_a 16 -> 32, bn_a, ReLU, conv_b 32 -> 9, bn_b) in train mode with the fixture's seeded state through
    sptrain_net.head: output, dx and the 8 parameter gradients against the fixture's samples at the default bar and its totals at the
    first term; both convolution biases exactly 0; the buffers at 1e-5 + 1e-5 |ref|; the evaluation output"""
    from image_matching_amd import sptrain_net
    from image_matching_amd.engine import ImxError
    g = util.golden("bn2d_head.npz")
    seed = int(g["seed"])
    x, dy = (cuda(a) for a in R2.head_case(seed))
    mods = [R2.load_head(seed).train().cuda() for _ in range(2)]
    fn = lambda m: (lambda a: sptrain_net.head(eng, m.conv_a, m.bn_a, m.conv_b, m.bn_b, a))
    ours = R2.head_grads(mods[0], fn(mods[0]), x, dy)
    theirs = R2.head_grads(mods[1], mods[1], x, dy)
    names = [str(n) for n in g["names"]]
    assert len(names) == 10 and set(names) == set(ours)
    fo, ft = {}, {}
    for i, name in enumerate(names):
        ref, ref_sum = g[f"{name}_g"], g[f"{name}_sum"]
        for res, f in ((ours, fo), (theirs, ft)):
            a = res[name].cpu().numpy().astype(np.float64)
            pos = head_positions(i, a.size)
            f[name] = max(float(np.max(np.abs(a.reshape(-1)[pos] - ref) / R2.bar(ref, g[f"{name}_d32"]))),
                          float(np.max(np.abs(a.sum() - ref_sum) / R2.bar(ref_sum))))
    show("head, sptrain_net.head", fo)
    show("head, all PyTorch on the device (not asserted)", ft)
    assert max(fo.values()) <= 1.0
    assert not ours["conv_a.bias"].any() and not ours["conv_b.bias"].any(), "a bias before a training BatchNorm: exactly 0"
    fb = {}
    for i, (n, b) in enumerate(R2.head_buffers(mods[0]).items()):
        ref = g[f"buffer_{i}"]
        assert str(g["buffer_names"][i]) == n
        if n.endswith("num_batches_tracked"):
            assert int(b) == int(ref) == 1
        else:
            fb[n] = float(np.max(np.abs(b - ref) / (1e-5 + 1e-5 * np.abs(ref))))
    show("head, buffers (of 1e-5 + 1e-5 |ref|)", fb)
    assert len(fb) == 4 and max(fb.values()) <= 1.0
    e = R2.load_head(seed).eval().cuda()
    with torch.no_grad():
        out = fn(e)(x).cpu().numpy().astype(np.float64)
    pos = head_positions(0, out.size)
    fe = float(np.max(np.abs(out.reshape(-1)[pos] - g["eval_g"]) / R2.bar(g["eval_g"], g["eval_d32"])))
    print(f"head, eval mode: of the bar -- out {fe:.3g}")
    assert fe <= 1.0 and int(e.bn_a.num_batches_tracked) == 0 and int(e.bn_b.num_batches_tracked) == 0
    with pytest.raises(ImxError, match="head: expected"):
        sptrain_net.head(eng, e.conv_a, e.bn_a, e.conv_a, e.bn_b, x)
    with pytest.raises(ImxError, match="head: bn must be"):
        sptrain_net.head(eng, e.conv_a, e.bn_a, e.conv_b, e.bn_a, x)
