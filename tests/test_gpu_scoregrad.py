"""The score product of SuperGlue's training step on the GPU (imx_score_product_forward_train, imx_score_product_backward,
Engine.score_product_forward_train, Engine.score_product_backward, image_matching_amd.sgtrain_grad.scores) against the project's
restatement in numpy float64 (tests/scoregrad_ref.py, itself held to torch's einsum and autograd by tests/test_scoregrad_host.py).  The
default bar, element-wise: |x - x64| <= max(1e-4 + 1e-4 |x64|, 2.5 |ref32 - x64|), ref32 = torch.einsum + autograd in fp32 on the CPU.
Every output buffer is filled with NaN before the call that writes it (call()).  Every parity test prints the fractions of the bar it used.
Needs an MI355X; well under a second per test."""
import functools

import numpy as np
import pytest
import torch

from tests import scoregrad_ref as R
from tests import util

pytestmark = pytest.mark.gpu
OUTPUTS = ("scores", "da", "db")
# the smallest shapes at which a tile (64), a chunk (32) or a block (128) boundary can go wrong
SHAPES = [(1, 64, 70, 100),        # partial tiles
          (2, 160, 130, 150),      # every summation index crosses a block of 128 and ends mid-chunk
          (1, 1, 33, 1), (1, 3, 1, 65)]   # degenerate shapes, rows of odd alignment
RAGGED = ((3, 64, 48, 80), (40, 0, 48), (70, 9, 80))


def new_engine():
    from image_matching_amd.engine import Engine
    return Engine(util.sp_config(128, 256), util.sg_config(128), "cuda")


@pytest.fixture(autouse=True)
def grad_enabled():
    """(a test module that imports one of the inference scripts switches autograd off for the whole process)"""
    with torch.enable_grad():
        yield


@pytest.fixture(scope="module")
def eng():
    return new_engine()


def cuda(a, dtype=torch.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def call(eng, a, b, ds, n0=None, n1=None, scale=None, want=(True, True)):
    """both entry points of the library into buffers filled with NaN beforehand, so that an element the kernels never write shows ->
    dict of numpy arrays: scores and those of da, db that were wanted.  (The Engine's own methods, which allocate their outputs, are
    held to these bits by test_autograd_bridge.)"""
    a, b, ds, n0, n1 = cuda(a), cuda(b), cuda(ds), cuda(n0, torch.int32), cuda(n1, torch.int32)
    (B, D, N0), N1 = a.shape, b.shape[2]
    scale = float(D) ** -0.5 if scale is None else float(scale)
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    res = {"scores": nan(B, N0, N1)}
    res.update({k: nan(*t.shape) for k, t, w in (("da", a, want[0]), ("db", b, want[1])) if w})
    p = lambda t: None if t is None else t.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    eng._check(eng.sgtrain.imx_score_product_forward_train(eng.handle, B, D, N0, N1, p(a), p(b), p(n0), p(n1), scale, p(res["scores"]), stream))
    eng._check(eng.sgtrain.imx_score_product_backward(eng.handle, B, D, N0, N1, p(a), p(b), p(ds), p(n0), p(n1), scale, p(res.get("da")),
                                                      p(res.get("db")), stream))
    torch.cuda.synchronize()
    return {key: t.cpu().numpy() for key, t in res.items()}


@functools.lru_cache(maxsize=None)
def seeded(seed, B, D, N0, N1):
    """the inputs of a seeded case, its float64 restatement and the fp32 einsum + autograd on the CPU, computed once and shared (read only)"""
    inputs = R.case(seed, B, D, N0, N1)
    return inputs, R.batch_reference(*inputs), R.autograd(*inputs, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def ragged(frame=None, fill=np.nan):
    """the ragged case: (inputs in a `fill`-padded frame, n0, n1, float64 restatement, fp32 einsum + autograd per pair)"""
    (B, D, N0, N1), n0, n1 = RAGGED
    a, b, ds = R.case(21, B, D, N0, N1)
    F0, F1 = frame or (N0, N1)
    a, b, ds = R.ragged_pad(a, (n0,), (F0,), (2,), fill), R.ragged_pad(b, (n1,), (F1,), (2,), fill), R.ragged_pad(ds, (n0, n1), (F0, F1), (1, 2), fill)
    n0, n1 = np.array(n0, np.int32), np.array(n1, np.int32)
    return (a, b, ds), n0, n1, R.batch_reference(a, b, ds, n0, n1), R.ragged_autograd(a, b, ds, n0, n1, dtype=torch.float32)


def fractions(res, ref, ref32):
    """the worst fraction of the default bar per tensor"""
    return {t: float(np.max(np.abs(res[t].astype(np.float64) - ref[t]) / R.bar(ref[t], ref32[t] - ref[t]))) for t in OUTPUTS if t in res}


def show(what, f):
    print(f"{what}: of the bar -- " + ", ".join(f"{t} {v:.3g}" for t, v in f.items()))


def bits(x, y):
    return x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.int32), np.ascontiguousarray(y).view(np.int32))


def same_bits(x, y):
    return all(bits(x[k], y[k]) for k in OUTPUTS if k in x and k in y)


# ---------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("shape", SHAPES)
def test_parity(eng, shape):
    inputs, ref, ref32 = seeded(100 + sum(shape), *shape)
    res = call(eng, *inputs)
    assert all(np.isfinite(v).all() for v in res.values()), "an element was never written"
    f = fractions(res, ref, ref32)
    show(f"(B, D, N0, N1) = {shape}", f)
    assert len(f) == 3 and max(f.values()) <= 1.0


def test_scale_argument(eng):
    """scale = None is D ** -0.5; any finite scale, negative included, multiplies the finished sums"""
    shape = SHAPES[0]
    inputs, _, _ = seeded(100 + sum(shape), *shape)
    assert same_bits(call(eng, *inputs), call(eng, *inputs, scale=0.125))
    res = call(eng, *inputs, scale=-3.0)
    f = fractions(res, R.batch_reference(*inputs, scale=-3.0), R.autograd(*inputs, dtype=torch.float32, scale=-3.0))
    show("scale = -3", f)
    assert max(f.values()) <= 1.0


def test_ragged_batch(eng):
    """three pairs with counts n0 = (40, 0, 48), n1 = (70, 9, 80) in a frame (48, 80), NaN in every padded column of a, b and dscores:
    finite, exactly 0 past the counts, within the bar on the valid block; NULL counts equal full counts and counts are clamped"""
    inputs, n0, n1, ref, ref32 = ragged()
    res = call(eng, *inputs, n0, n1)
    assert all(np.isfinite(v).all() for v in res.values()), "NaN padding leaked, or an element was never written"
    for p, (c0, c1) in enumerate(zip(n0, n1)):
        assert not res["scores"][p, c0:].any() and not res["scores"][p, :, c1:].any(), p
        assert not res["da"][p, :, c0:].any() and not res["db"][p, :, c1:].any(), p
    assert not any(res[t][1].any() for t in OUTPUTS), "a pair with n0 = 0 gets zeros everywhere"
    f = fractions(res, ref, ref32)
    show("ragged", f)
    assert max(f.values()) <= 1.0
    shape = SHAPES[1]
    full, _, _ = seeded(100 + sum(shape), *shape)
    whole = call(eng, *full)
    assert same_bits(whole, call(eng, *full, np.array([130, 130], np.int32), np.array([150, 150], np.int32))), "NULL means all"
    assert same_bits(whole, call(eng, *full, np.array([131, 1 << 30], np.int32), np.array([1 << 30, 150], np.int32))), "counts are clamped to the frame"
    empty = call(eng, *full, np.array([0, -3], np.int32), np.array([150, 150], np.int32))
    assert all(np.isfinite(empty[t]).all() and not empty[t].any() for t in OUTPUTS), "no valid row anywhere: zeros"


# ---------------------------------------------------------------------------------------------- determinism
def test_equal_bits_between_calls_frames_and_batches(eng):
    """the same call twice; each pair alone in a frame of its own size against the same pair in a larger NaN-padded frame beside the
    others: the same bits on the valid block"""
    inputs, n0, n1, _, _ = ragged()
    first = call(eng, *inputs, n0, n1)
    assert same_bits(first, call(eng, *inputs, n0, n1)), "the same call twice"
    wide, _, _, _, _ = ragged(frame=(131, 200))
    larger = call(eng, *wide, n0, n1)
    assert all(np.isfinite(v).all() for v in larger.values())
    for p, (c0, c1) in enumerate(zip(n0, n1)):
        assert bits(first["scores"][p, :c0, :c1], larger["scores"][p, :c0, :c1]), "the frame does not enter the order"
        assert bits(first["da"][p, :, :c0], larger["da"][p, :, :c0]) and bits(first["db"][p, :, :c1], larger["db"][p, :, :c1])
        if c0 and c1:
            a, b, ds = inputs
            alone = call(eng, a[p:p + 1, :, :c0], b[p:p + 1, :, :c1], ds[p:p + 1, :c0, :c1])
            assert bits(alone["scores"][0], larger["scores"][p, :c0, :c1]), f"pair {p} alone in its own frame"
            assert bits(alone["da"][0], larger["da"][p, :, :c0]) and bits(alone["db"][0], larger["db"][p, :, :c1]), p


def test_one_gradient_has_the_bits_of_both(eng):
    shape = SHAPES[1]
    inputs, _, _ = seeded(100 + sum(shape), *shape)
    both = call(eng, *inputs)
    only_a, only_b = call(eng, *inputs, want=(True, False)), call(eng, *inputs, want=(False, True))
    assert "db" not in only_a and "da" not in only_b and "da" in only_a and "db" in only_b
    assert same_bits(both, only_a) and same_bits(both, only_b)
    assert set(call(eng, *inputs, want=(False, False))) == {"scores"}, "nothing wanted: nothing formed"


def test_equal_bits_on_used_and_poisoned_handles(eng):
    """the pattern of tests/test_gpu_history.py: a used handle, a handle whose workspaces are filled with NaN / 3.4e38 / zero bytes, and a
    handle that allocates under the hook from the start return the bits of the first call"""
    inputs, n0, n1, _, _ = ragged()
    want = call(eng, *inputs, n0, n1)
    shape = SHAPES[1]
    big, _, _ = seeded(100 + sum(shape), *shape)
    other = new_engine()
    assert same_bits(want, call(other, *inputs, n0, n1)), "a second fresh handle"
    call(other, *big)
    assert same_bits(want, call(other, *inputs, n0, n1)), "after a larger call on the same handle"
    try:
        for p in ("nan", "huge", "zero"):
            other.set_option("debug_poison", p)
            assert same_bits(want, call(other, *inputs, n0, n1)), f"after debug_poison = {p}"
    finally:
        other.set_option("debug_poison", "off")
    cold = new_engine()
    cold.set_option("debug_poison", "nan")
    try:
        assert same_bits(want, call(cold, *inputs, n0, n1)), "workspaces allocated under debug_poison = nan"
    finally:
        cold.set_option("debug_poison", "off")


# ---------------------------------------------------------------------------------------------- errors
def test_errors_are_reported_and_the_handle_survives(eng):
    from image_matching_amd.engine import ImxError
    z = lambda *s: torch.zeros(*s, device="cuda")
    with pytest.raises(ImxError, match="contiguous fp32 cuda"):
        eng.score_product_forward_train(z(1, 3, 4).transpose(1, 2), z(1, 4, 4))
    with pytest.raises(ImxError, match=r"a and b must be \(B,D,N0\) and \(B,D,N1\)"):
        eng.score_product_forward_train(z(1, 4, 3), z(1, 5, 3))
    with pytest.raises(ImxError, match=r"dscores must be \(1,3,5\)"):
        eng.score_product_backward(z(1, 4, 3), z(1, 4, 5), z(1, 5, 3))
    with pytest.raises(ImxError, match="want must be two flags"):
        eng.score_product_backward(z(1, 4, 3), z(1, 4, 5), z(1, 3, 5), want=(True,))
    with pytest.raises(ImxError, match="2 counts for a batch of 1"):
        eng.score_product_forward_train(z(1, 4, 3), z(1, 4, 5), n0=[1, 2])
    lib, h = eng.sgtrain, eng.handle
    a, b, s, da, db = z(1, 4, 8), z(1, 4, 8), z(1, 8, 8), z(1, 4, 8), z(1, 4, 8)
    p = lambda t: t.data_ptr()
    err = lambda: eng.lib.imx_last_error(eng.handle)
    fwd = lambda B=1, D=4, N0=8, N1=8, a_=p(a), b_=p(b), scale=0.5, s_=p(s): \
        lib.imx_score_product_forward_train(h, B, D, N0, N1, a_, b_, None, None, scale, s_, None)
    bwd = lambda B=1, D=4, N0=8, N1=8, a_=p(a), b_=p(b), ds_=p(s), scale=0.5, da_=p(da), db_=p(db): \
        lib.imx_score_product_backward(h, B, D, N0, N1, a_, b_, ds_, None, None, scale, da_, db_, None)
    # each bound once; nothing is launched, so the (small) buffers are never touched
    for kw in (dict(B=0), dict(B=65536), dict(D=0), dict(D=1025), dict(N0=0), dict(N0=(1 << 20) + 1), dict(N1=0), dict(N1=(1 << 20) + 1)):
        for fn, name in ((fwd, b"imx_score_product_forward_train"), (bwd, b"imx_score_product_backward")):
            assert fn(**kw) < 0 and name in err() and b"bad shape" in err(), kw
    for fn, name in ((fwd, b"imx_score_product_forward_train"), (bwd, b"imx_score_product_backward")):
        assert fn(B=65535, N0=1 << 20, N1=1 << 20) < 0 and name in err() and b"tiles" in err(), "the tile count must fit the grid"
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert fn(scale=bad) < 0 and name in err() and b"scale must be finite" in err()
        for kw in (dict(a_=None), dict(b_=None)):
            assert fn(**kw) < 0 and name in err() and b"null argument" in err(), kw
    assert fwd(s_=None) < 0 and b"imx_score_product_forward_train: null argument" in err()
    assert bwd(ds_=None) < 0 and b"imx_score_product_backward: null argument" in err()
    # aliasing: an output on top of an input, or overlapping it in part
    assert fwd(D=8, s_=p(a)) < 0 and b"imx_score_product_forward_train: scores aliases an input" in err()
    assert fwd(s_=p(b) + 16) < 0 and b"scores aliases an input" in err()
    assert bwd(da_=p(a)) < 0 and b"imx_score_product_backward: da aliases an input" in err()
    assert bwd(D=8, da_=p(s)) < 0 and b"da aliases an input" in err()
    assert bwd(db_=p(b)) < 0 and b"db aliases an input" in err()
    assert bwd(da_=p(da), db_=p(da) + 4) < 0 and b"da aliases db" in err()
    assert bwd(da_=None, db_=None) == 0, "nothing wanted: nothing launched"
    shape = SHAPES[0]
    inputs, ref, ref32 = seeded(100 + sum(shape), *shape)
    assert max(fractions(call(eng, *inputs), ref, ref32).values()) <= 1.0, "a valid call after the errors"


# ---------------------------------------------------------------------------------------------- the bridge to autograd
def test_autograd_bridge(eng):
    """sgtrain_grad.scores(...) and .backward(dS) against the restatement (gradcheck is of no use in fp32); needs_input_grad = (True,
    False) skips score_db, read from the timing rows"""
    from image_matching_amd import sgtrain_grad
    inputs, n0, n1, ref, ref32 = ragged()
    a, b = (cuda(t).requires_grad_(True) for t in inputs[:2])
    s = sgtrain_grad.scores(eng, a, b, cuda(n0, torch.int32), cuda(n1, torch.int32))
    s.backward(cuda(inputs[2])[:, :, :])
    res = {"scores": s.detach().cpu().numpy(), "da": a.grad.cpu().numpy(), "db": b.grad.cpu().numpy()}
    assert all(np.isfinite(v).all() for v in res.values())
    f = fractions(res, ref, ref32)
    show("bridge", f)
    assert max(f.values()) <= 1.0
    assert same_bits(res, call(eng, *inputs, n0, n1)), "the bridge runs the same kernels on the same tensors"
    # a non-contiguous cotangent: the bridge makes it contiguous
    shape = SHAPES[0]
    full, fref, fref32 = seeded(100 + sum(shape), *shape)
    a, b = (cuda(t).requires_grad_(True) for t in full[:2])
    sgtrain_grad.scores(eng, a, b).backward(cuda(np.ascontiguousarray(full[2].transpose(0, 2, 1))).transpose(1, 2))
    f = fractions({"da": a.grad.cpu().numpy(), "db": b.grad.cpu().numpy()}, fref, fref32)
    assert max(f.values()) <= 1.0

    def rows(need_b):
        a, b = cuda(full[0]).requires_grad_(True), cuda(full[1]).requires_grad_(need_b)
        eng.set_timing(True)
        eng.timing_reset()
        try:
            sgtrain_grad.scores(eng, a, b).backward(cuda(full[2]))
            torch.cuda.synchronize()
            names = {r[0]: r[1] for r in eng.timing_report()}
        finally:
            eng.set_timing(False)
        assert a.grad is not None and (b.grad is not None) == need_b
        return names

    assert rows(True) == {"score_fwd": 1, "score_da": 1, "score_db": 1}
    assert rows(False) == {"score_fwd": 1, "score_da": 1}, "needs_input_grad = (True, False) skips score_db"
