"""nn.MaxPool2d(2), the descriptor normalisation and the trainable SuperPoint network on the GPU (imx_maxpool2_forward_train,
imx_maxpool2_backward, imx_l2norm_forward_train, imx_l2norm_backward, the Engine methods of the same names,
image_matching_amd.sptrain_net.maxpool2 / max_pool2 / l2norm / normalize_descriptors / down_pooled and
image_matching_amd.sptrain_model.SuperPointTrainable) against the project's restatements (tests/sppool_ref.py, held to torch by
tests/test_sppool_host.py) and against the samples the reference's own blocks wrote under torch.autograd
(tests/golden/make_golden_sppool.py).  Pooling is compared bit for bit.  Everything else at the default bar, element-wise:
|x - x64| <= max(1e-4 + 1e-4 |x64|, 2.5 |ref32 - x64|), the first term alone where no reference fp32 value exists (sums).  Needs an
MI355X; a few seconds per test."""
import hashlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv3grad_ref as R3
from tests import sppool_ref as RP
from tests import util

pytestmark = pytest.mark.gpu
POOL_H = (2, 3, 9)
POOL_W = (2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 66, 67, 129, 514, 515)
POOL_BC = ((1, 1), (2, 3), (3, 65))
L2_C = (1, 3, 64, 65, 128, 256, 1024)
L2_HW = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1200, 4097)
GUARD = 16                     # floats (bytes for idx) of sentinel in front of and behind every output of a raw call
SENTINEL, SENTINEL_BYTE = 12345.0, 0xAB


def new_engine():
    from image_matching_amd.engine import Engine
    return Engine(util.sp_config(128, 256), util.sg_config(128), "cuda")


@pytest.fixture(scope="module")
def eng():
    return new_engine()


def cuda(a, dtype=torch.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


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


class Banded:
    """a tensor of `shape` inside a larger allocation filled with a sentinel: `shift` elements past the guard band (0: 16-byte aligned
    like the allocation; 1: one element further)"""

    def __init__(self, shape, dtype=torch.float32, shift=0, fill=None):
        n = int(np.prod(shape))
        self.sentinel = SENTINEL if dtype == torch.float32 else SENTINEL_BYTE
        self.big = torch.full((n + 2 * GUARD + 1,), self.sentinel, dtype=dtype, device="cuda")
        self.lo, self.hi = GUARD + shift, GUARD + shift + n
        self.t = self.big[self.lo:self.hi].view(shape)
        if fill is not None:
            self.t.copy_(fill)
        assert self.t.is_contiguous() and self.t.data_ptr() % (16 if dtype == torch.float32 else 4) == (shift * self.t.element_size())

    def untouched(self):
        return bool((self.big[:self.lo] == self.sentinel).all()) and bool((self.big[self.hi:] == self.sentinel).all())


def raw_pool(eng, x, dy, shift=0, want_idx=True):
    """both pooling calls through the C ABI, every tensor `shift` elements off its 16-byte boundary and every output between guard
    bands -> (y, idx or None, dx as numpy arrays, the guard bands were left alone)"""
    B, C, H, W = x.shape
    out = (B, C, H // 2, W // 2)
    xs, dys = Banded(x.shape, shift=shift, fill=cuda(x)), Banded(out, shift=shift, fill=cuda(dy))
    ys, dxs = Banded(out, shift=shift), Banded(x.shape, shift=shift)
    idxs = Banded(out, torch.uint8, shift=shift)
    lib, p = eng.sppool, lambda b: b.t.data_ptr()
    assert lib.imx_maxpool2_forward_train(eng.handle, B, C, H, W, p(xs), p(ys), p(idxs) if want_idx else None, None) == 0, eng.lib.imx_last_error(eng.handle)
    if not want_idx:
        torch.cuda.synchronize()
        return ys.t.cpu().numpy(), None, None, ys.untouched() and idxs.untouched() and not bool((idxs.t != SENTINEL_BYTE).any())
    assert lib.imx_maxpool2_backward(eng.handle, B, C, H, W, p(idxs), p(dys), p(dxs), None) == 0, eng.lib.imx_last_error(eng.handle)
    torch.cuda.synchronize()
    return ys.t.cpu().numpy(), idxs.t.cpu().numpy(), dxs.t.cpu().numpy(), ys.untouched() and idxs.untouched() and dxs.untouched()


# ---------------------------------------------------------------------------------------------- 1. pooling, bit for bit
@pytest.mark.parametrize("H", POOL_H)
def test_pooling_equals_the_restatement_bit_for_bit(eng, H):
    """every W of the list with (B, C) cycling, plain and ReLU-like inputs: y, idx and dx of the Engine methods and of the raw calls --
    aligned, one element off (the dword form), and with idx_dev = NULL -- equal the restatement's bits; the guard band around every
    output is untouched; the reported form is x4 exactly where W % 8 == 0 and the pointers are aligned"""
    bad = []
    for n, W in enumerate(POOL_W):
        B, C = POOL_BC[(n + POOL_H.index(H)) % 3]
        plain, dy = RP.pool_case(100 + n, B, C, H, W)
        for relu_like in (False, True):
            x = np.maximum(plain, np.float32(0)) if relu_like else plain          # (pool_case's own ReLU-like form)
            y, idx = RP.pool_forward(x)
            dx = RP.pool_backward(idx, dy, x.shape)
            if relu_like and x.size >= 1000:
                assert 0.45 < (x == 0).mean() < 0.55, "about half of a ReLU-like map is exact zeros"
            tag = (B, C, H, W, relu_like)
            fwd = eng.maxpool2_forward_train(cuda(x))
            bwd = eng.maxpool2_backward(fwd["idx"], cuda(dy), x.shape)
            assert fwd["idx"].dtype == torch.uint8
            if not (bits(fwd["y"].cpu().numpy(), y) and bits(fwd["idx"].cpu().numpy(), idx) and bits(bwd["dx"].cpu().numpy(), dx)):
                bad.append(("engine",) + tag)
            ev = eng.maxpool2_forward_train(cuda(x), want_idx=False)
            if ev["idx"] is not None or not bits(ev["y"].cpu().numpy(), y):
                bad.append(("want_idx=False",) + tag)
            for shift in (0, 1):
                got = {}
                rows = forms_of(eng, lambda: got.update(zip("abcd", raw_pool(eng, x, dy, shift))))
                want_form = "x4" if (W % 8 == 0 and shift == 0) else "x1"
                if rows != {("maxpool2_fwd", want_form), ("maxpool2_bwd", want_form)}:
                    bad.append(("form", shift, sorted(rows)) + tag)
                if not (bits(got["a"], y) and bits(got["b"], idx) and bits(got["c"], dx)):
                    bad.append(("raw", shift) + tag)
                if not got["d"]:
                    bad.append(("guard band", shift) + tag)
            ys, none, _, clean = raw_pool(eng, x, dy, 0, want_idx=False)
            if none is not None or not bits(ys, y) or not clean:
                bad.append(("idx_dev = NULL",) + tag)
    assert not bad, bad


@pytest.mark.parametrize("shape", [(3, 3, 2, 2), (3, 3, 9, 7), (3, 3, 3, 17), (3, 3, 9, 16), (3, 3, 8, 64), (3, 3, 9, 515)])
def test_pooling_special_windows(eng, shape):
    """the nine special windows (all equal, the three tie positions, NaN first, two NaNs, NaN before a larger value, all -inf, -0 before
    +0), one per plane, planted at a map's first window, its last window and its last partial row: bits of the restatement, which
    tests/test_sppool_host.py holds to PyTorch's"""
    base, dy = RP.pool_case(9, *shape)
    for where in (lambda H, W: (0, 0), lambda H, W: (H // 2 - 1, W // 2 - 1), lambda H, W: (H // 2 - 1, 0)):
        x = RP.plant(base, where)
        y, idx = RP.pool_forward(x)
        r, c = where(*shape[2:])
        assert [int(idx[(n // 3) % 3, n % 3, r, c]) for n in range(9)] == [w for _, _, w in RP.SPECIAL_WINDOWS]
        dx = RP.pool_backward(idx, dy, shape)
        for shift in (0, 1):
            gy, gi, gdx, clean = raw_pool(eng, x, dy, shift)
            assert bits(gy, y) and bits(gi, idx) and bits(gdx, dx) and clean, (shape, shift)


def test_pooling_offsets_beyond_32_bits(eng):
    """(65, 1, 4096, 4096): the last image starts 4.3e9 bytes into x and dx.  Its y, idx and dx equal, bit for bit and on the device,
    the same image run alone"""
    B, H, W = 65, 4096, 4096
    free = torch.cuda.mem_get_info()[0]
    if free < 20 * 2 ** 30:
        print(f"skipped: {free / 2 ** 30:.1f} GiB free on the device, the test asks for 20 GiB (its allocator peak is about 12 GiB)")
        pytest.skip("not enough free device memory")
    gen = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(B, 1, H, W, device="cuda", generator=gen)
    dy = torch.randn(B, 1, H // 2, W // 2, device="cuda", generator=gen)
    assert (B - 1) * H * W * 4 >= 2 ** 32, "every byte offset into the last image is 2^32 or more"
    fwd = eng.maxpool2_forward_train(x)
    dx = eng.maxpool2_backward(fwd["idx"], dy, x.shape)["dx"]
    one = eng.maxpool2_forward_train(x[B - 1:].contiguous())
    dx1 = eng.maxpool2_backward(one["idx"], dy[B - 1:].contiguous(), (1, 1, H, W))["dx"]
    same = (torch.equal(fwd["y"][B - 1].view(torch.int32), one["y"][0].view(torch.int32)) and torch.equal(fwd["idx"][B - 1], one["idx"][0])
            and torch.equal(dx[B - 1].view(torch.int32), dx1[0].view(torch.int32)))
    agrees = torch.equal(one["y"], F.max_pool2d(x[B - 1:], 2))
    routed = float((dx1 != 0).float().mean())
    del x, dy, fwd, dx, one, dx1
    torch.cuda.empty_cache()
    print(f"offsets: last image {'equal' if same else 'DIFFERENT'}; nonzero share of dx {routed:.3g}")
    assert same and agrees and abs(routed - 0.25) < 1e-3


# ---------------------------------------------------------------------------------------------- 2. the normalisation
def l2_call(eng, x, dy):
    x, dy = (t if isinstance(t, torch.Tensor) else cuda(t) for t in (x, dy))
    res = dict(eng.l2norm_forward_train(x))
    res.update(eng.l2norm_backward(res["y"], res["norm"], dy))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def same_bits(a, b):
    return all(bits(a[k], b[k]) for k in ("y", "norm", "dx"))


@pytest.mark.parametrize("C", L2_C)
def test_norm_values(eng, C):
    """y, norm and dx against the float64 closed forms at the default bar, the reference's two lines under PyTorch in fp32 as the second
    term (norm: the first term alone), over every HW of the list and B in {1, 3}"""
    worst = {"y": 0.0, "norm": 0.0, "dx": 0.0}
    gen = torch.Generator().manual_seed(1000 + C)
    for HW in L2_HW:
        for B in (1, 3):
            x = (torch.randn(B, C, HW, generator=gen) * torch.exp(0.5 * torch.randn(B, C, HW, generator=gen))).numpy()
            dy = torch.randn(B, C, HW, generator=gen).numpy()
            ref, ref32, got = RP.l2_reference(x, dy), RP.l2_autograd(x, dy, torch.float32), l2_call(eng, x, dy)
            assert got["norm"].shape == (B, HW) and got["y"].shape == got["dx"].shape == (B, C, HW)
            for k in worst:
                f = float(np.max(np.abs(got[k] - ref[k]) / RP.bar(ref[k], None if k == "norm" else ref32[k] - ref[k])))
                assert f <= 1.0, (k, B, C, HW, f)
                worst[k] = max(worst[k], f)
    print(f"l2norm C={C}: of the bar -- " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def test_norm_special_inputs(eng):
    """a zero vector gives NaN in exactly its own pixel, forward and backward; a one-hot vector gives y exactly"""
    x, dy = RP.l2_case(21, 2, 65, 130)
    x[1, :, 77] = 0
    got = l2_call(eng, x, dy)
    bad = np.zeros((2, 130), bool)
    bad[1, 77] = True
    assert (np.isnan(got["y"]) == bad[:, None, :]).all() and (np.isnan(got["dx"]) == bad[:, None, :]).all()
    assert (np.isnan(got["norm"]) == False).all() and got["norm"][1, 77] == 0       # noqa: E712
    hot = np.zeros((2, 65, 130), np.float32)
    vals = RP.heavy(22, "l2.hot", (2, 130))
    ch = (np.arange(2 * 130).reshape(2, 130) * 7) % 65
    np.put_along_axis(hot, ch[:, None, :], vals[:, None, :], 1)
    got = l2_call(eng, hot, dy)
    assert bits(got["y"], np.sign(hot).astype(np.float32) + np.float32(0)) and bits(got["norm"], np.abs(vals))


def test_norm_invariance(eng):
    """an image has the same bits alone and in any batch, between calls, on a second handle with debug_poison = nan, and in the dword
    form of a misaligned pointer; at 2^16 pixels and more the 16-byte form runs and gives the bits of each image run alone in the dword
    form"""
    for C, HW in ((65, 257), (256, 1200), (1024, 64)):
        x, dy = RP.l2_case(31, 3, C, HW)
        full = l2_call(eng, x, dy)
        assert same_bits(full, l2_call(eng, x, dy)), "between calls"
        for b in range(3):
            alone = l2_call(eng, x[b:b + 1], dy[b:b + 1])
            assert all(bits(alone[k][0], full[k][b]) for k in ("y", "norm", "dx")), (C, HW, b)
        pair = l2_call(eng, x[[2, 0]], dy[[2, 0]])
        assert all(bits(pair[k][0], full[k][2]) and bits(pair[k][1], full[k][0]) for k in ("y", "norm", "dx"))
    other = new_engine()
    other.set_option("debug_poison", "nan")
    try:
        assert same_bits(full, l2_call(other, x, dy)), "a second handle, debug_poison = nan"
    finally:
        other.set_option("debug_poison", "off")
    # the forms
    B, C, HW = 2, 3, 1 << 15
    x, dy = RP.l2_case(33, B, C, HW)
    got = {}
    rows = forms_of(eng, lambda: got.update(l2_call(eng, x, dy)))
    assert rows == {("l2norm_fwd", "x4"), ("l2norm_bwd", "x4")}, rows
    for b in range(B):
        alone = {}
        rows = forms_of(eng, lambda: alone.update(l2_call(eng, x[b:b + 1], dy[b:b + 1])))
        assert rows == {("l2norm_fwd", "x1"), ("l2norm_bwd", "x1")}, rows
        assert all(bits(alone[k][0], got[k][b]) for k in ("y", "norm", "dx")), b
    xs, dys = Banded(x.shape, shift=1, fill=cuda(x)), Banded(x.shape, shift=1, fill=cuda(dy))
    ys, dxs, ns = Banded(x.shape, shift=1), Banded(x.shape, shift=1), Banded((B, HW), shift=1)
    lib, p = eng.sppool, lambda b: b.t.data_ptr()

    def run():
        assert lib.imx_l2norm_forward_train(eng.handle, B, C, HW, p(xs), p(ys), p(ns), None) == 0
        assert lib.imx_l2norm_backward(eng.handle, B, C, HW, p(ys), p(ns), p(dys), p(dxs), None) == 0
    rows = forms_of(eng, run)
    torch.cuda.synchronize()
    assert rows == {("l2norm_fwd", "x1"), ("l2norm_bwd", "x1")}, rows
    assert bits(ys.t.cpu().numpy(), got["y"]) and bits(ns.t.cpu().numpy(), got["norm"]) and bits(dxs.t.cpu().numpy(), got["dx"])
    assert ys.untouched() and dxs.untouched() and ns.untouched()


# ---------------------------------------------------------------------------------------------- 3. errors
def test_errors_are_reported_and_the_handle_survives(eng):
    from image_matching_amd.engine import ImxError
    z = lambda *s: torch.zeros(*s, device="cuda")
    zb = lambda *s: torch.zeros(*s, dtype=torch.uint8, device="cuda")
    p = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
    err = lambda: eng.lib.imx_last_error(eng.handle)
    lib = eng.sppool
    x, y, idx, dy, dx = z(2, 3, 4, 6), z(2, 3, 2, 3), zb(2, 3, 2, 3), z(2, 3, 2, 3), z(2, 3, 4, 6)
    fwd = lambda B=2, C=3, H=4, W=6, xx=x, yy=y, ii=idx: lib.imx_maxpool2_forward_train(eng.handle, B, C, H, W, p(xx), p(yy), p(ii), None)
    bwd = lambda B=2, C=3, H=4, W=6, ii=idx, d=dy, xx=dx: lib.imx_maxpool2_backward(eng.handle, B, C, H, W, p(ii), p(d), p(xx), None)
    for call in (fwd, bwd):
        for kw in ({"B": 0}, {"B": 65536}, {"C": 0}, {"C": 1025}, {"H": 1}, {"H": 4097}, {"W": 1}, {"W": 4097}):
            assert call(**kw) != 0 and b"bad shape" in err(), kw
    for kw in ({"xx": None}, {"yy": None}):
        assert fwd(**kw) != 0 and b"null argument" in err(), kw
    for kw in ({"ii": None}, {"d": None}, {"xx": None}):
        assert bwd(**kw) != 0 and b"null argument" in err(), kw
    for kw, text in (({"yy": x}, b"y aliases x"), ({"yy": x.data_ptr() + 4 * 100}, b"y aliases x"), ({"ii": x.data_ptr() + 8}, b"idx aliases x"),
                     ({"ii": y.data_ptr() + 4}, b"y aliases idx")):
        assert fwd(**kw) != 0 and text in err(), (kw, err())
    for kw, text in (({"xx": dy.data_ptr() - 4 * 100}, b"dx aliases dy"), ({"xx": idx.data_ptr() - 8}, b"dx aliases idx")):
        assert bwd(**kw) != 0 and text in err(), (kw, err())
    v, w, n, dv, dw = z(2, 5, 7), z(2, 5, 7), z(2, 7), z(2, 5, 7), z(2, 5, 7)
    lf = lambda B=2, C=5, HW=7, xx=v, yy=w, nn=n: lib.imx_l2norm_forward_train(eng.handle, B, C, HW, p(xx), p(yy), p(nn), None)
    lb = lambda B=2, C=5, HW=7, yy=w, nn=n, d=dv, xx=dw: lib.imx_l2norm_backward(eng.handle, B, C, HW, p(yy), p(nn), p(d), p(xx), None)
    for call in (lf, lb):
        for kw in ({"B": 0}, {"C": 0}, {"C": 1025}, {"HW": 0}, {"HW": (1 << 24) + 1}, {"B": 129, "HW": 1 << 24}):
            assert call(**kw) != 0 and b"bad shape" in err(), kw
    for kw in ({"xx": None}, {"yy": None}, {"nn": None}):
        assert lf(**kw) != 0 and b"null argument" in err(), kw
    for kw in ({"xx": None}, {"yy": None}, {"nn": None}, {"d": None}):
        assert lb(**kw) != 0 and b"null argument" in err(), kw
    for kw, text in (({"yy": v}, b"y aliases x"), ({"nn": v.data_ptr() + 4 * 60}, b"norm aliases x"), ({"nn": w.data_ptr() + 4}, b"y aliases norm")):
        assert lf(**kw) != 0 and text in err(), (kw, err())
    for kw, text in (({"xx": w}, b"dx aliases y"), ({"xx": dv.data_ptr() + 4}, b"dx aliases dy"), ({"xx": n.data_ptr() - 4 * 50}, b"dx aliases norm")):
        assert lb(**kw) != 0 and text in err(), (kw, err())
    torch.cuda.synchronize()
    assert not any(t.any() for t in (x, y, idx, dy, dx, v, w, n, dv, dw)), "a refused call writes nothing"
    for bad in (z(2, 3, 4, 6).transpose(2, 3), z(2, 3, 4, 6).double(), torch.zeros(2, 3, 4, 6)):
        with pytest.raises(ImxError, match="x must be a contiguous float32 cuda tensor"):
            eng.maxpool2_forward_train(bad)
        with pytest.raises(ImxError, match="x must be a contiguous float32 cuda tensor"):
            eng.l2norm_forward_train(bad)
    with pytest.raises(ImxError, match="idx must be a contiguous uint8 cuda tensor"):
        eng.maxpool2_backward(z(2, 3, 2, 3), dy, (2, 3, 4, 6))
    with pytest.raises(ImxError, match=r"dy must be \(2,3,2,3\)"):
        eng.maxpool2_backward(idx, z(2, 3, 3, 2), (2, 3, 4, 6))
    with pytest.raises(ImxError, match="bad shape"):
        eng.maxpool2_forward_train(z(1, 1, 1, 8))
    with pytest.raises(ImxError, match="norm"):
        eng.l2norm_backward(w, z(2, 5), dv)
    with pytest.raises(ImxError, match="bad shape"):
        eng.l2norm_forward_train(z(1, 1025, 2))
    xs, dys = RP.pool_case(41, 2, 3, 5, 9)
    gy, gi, gdx, clean = raw_pool(eng, xs, dys)
    yr, ir = RP.pool_forward(xs)
    assert bits(gy, yr) and bits(gi, ir) and bits(gdx, RP.pool_backward(ir, dys, xs.shape)) and clean, "a valid call after the errors"


# ---------------------------------------------------------------------------------------------- 4. the bridge to autograd
@torch.enable_grad()                                     # (another test module may have turned gradients off for the process)
def test_bridge_to_autograd(eng):
    """max_pool2 and normalize_descriptors under loss.backward() against PyTorch's own operations on the device: pooling bit for bit
    (output and gradient), the normalisation at the default bar against float64 with PyTorch's fp32 as the second term; maxpool2 saves
    one byte per output and nothing else, l2norm saves y and norm"""
    from image_matching_amd import sptrain_net
    for shape in ((2, 5, 9, 16), (2, 16, 15, 21), (1, 64, 30, 40)):
        xn, dyn = RP.pool_case(51, *shape, relu_like=True)
        saved = []
        with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
            a = cuda(xn).requires_grad_(True)
            ya = sptrain_net.max_pool2(eng, a)
        assert [(t.dtype, tuple(t.shape)) for t in saved] == [(torch.uint8, tuple(ya.shape))], "nothing but idx is saved by maxpool2"
        (ya * cuda(dyn)).sum().backward()
        b = cuda(xn).requires_grad_(True)
        yb = F.max_pool2d(b, 2)
        (yb * cuda(dyn)).sum().backward()
        assert torch.equal(ya.view(torch.int32), yb.view(torch.int32)) and torch.equal(a.grad.view(torch.int32), b.grad.view(torch.int32)), shape
        with torch.no_grad():
            assert torch.equal(sptrain_net.max_pool2(eng, b.detach()), yb)
    for shape in ((2, 128, 2, 3), (3, 256, 15, 20)):
        xn, dyn = (t.reshape(shape) for t in RP.l2_case(53, shape[0], shape[1], shape[2] * shape[3]))
        saved = []
        with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
            a = cuda(xn).requires_grad_(True)
            ya = sptrain_net.normalize_descriptors(eng, a)
        assert [tuple(t.shape) for t in saved] == [shape, (shape[0],) + shape[2:]], "l2norm saves y and norm"
        (ya * cuda(dyn)).sum().backward()
        res = {}
        for dtype in (torch.float64, torch.float32):
            b = cuda(xn, dtype).requires_grad_(True)
            yb = b.div(torch.unsqueeze(torch.norm(b, p=2, dim=1), 1))
            (yb * cuda(dyn, dtype)).sum().backward()
            res[dtype] = (yb.detach().double().cpu().numpy(), b.grad.double().cpu().numpy())
        for got, r64, r32, k in ((ya, res[torch.float64][0], res[torch.float32][0], "y"), (a.grad, res[torch.float64][1], res[torch.float32][1], "dx")):
            f = float(np.max(np.abs(got.detach().double().cpu().numpy() - r64) / RP.bar(r64, r32 - r64)))
            print(f"normalize_descriptors {shape}: of the bar -- {k} {f:.3g}")
            assert f <= 1.0
    from image_matching_amd.engine import ImxError
    with pytest.raises(ImxError, match="contiguous fp32 cuda"):
        sptrain_net.max_pool2(eng, torch.zeros(1, 1, 4, 4))


def test_down_pooled_equals_down_form(eng):
    """the restated down(16, 32) in train mode with the seeded state of conv3grad_block_down.npz: down_pooled has the bits of down_form --
    output, dx, the 8 parameter gradients and the buffers -- in every BatchNorm form"""
    from image_matching_amd import sptrain_net
    seed = int(util.golden("conv3grad_block_down.npz")["seed"])
    x, dy = (cuda(a) for a in R3.block_case(seed, "down"))
    for form in ("auto", "pixels", "channel"):
        blocks = [R3.load_block(R3.Down(*R3.BLOCKS["down"][0]), seed).train().cuda() for _ in range(2)]
        ours = R3.block_grads(blocks[0], lambda a: sptrain_net.down_pooled(eng, blocks[0], a, form), x, dy)
        theirs = R3.block_grads(blocks[1], lambda a: sptrain_net.down_form(eng, blocks[1], a, form), x, dy)
        assert len(ours) == 10 and set(ours) == set(theirs)
        for name in ours:
            assert torch.equal(ours[name].view(torch.int32), theirs[name].view(torch.int32)), (form, name)
        for (n, a), (_, b) in zip(R3.block_buffers(blocks[0]).items(), R3.block_buffers(blocks[1]).items()):
            assert bits(a, b), (form, n)


# ---------------------------------------------------------------------------------------------- 5. the network
def fractions(res, g, names):
    """per tensor: the largest share of the bar used by the samples (with the reference's fp32 term) and by the sum (first term alone)"""
    f = {}
    for i, name in enumerate(names):
        a = res[name].detach().double().cpu().numpy()
        ref, ref_sum = g[f"{i}_g"], g[f"{i}_sum"]
        f[name] = max(float(np.max(np.abs(a.reshape(-1)[RP.net_positions(i, a.size)] - ref) / RP.bar(ref, g[f"{i}_d32"]))),
                      float(np.max(np.abs(a.sum() - ref_sum) / RP.bar(ref_sum))))
    return f


def show(what, f):
    worst = max(f, key=f.get)
    print(f"{what}: of the bar -- semi {f['semi']:.3g}, desc {f['desc']:.3g}, dx {f['dx']:.3g}, worst gradient "
          f"{max(v for k, v in f.items() if k not in ('semi', 'desc', 'dx')):.3g}, worst of all {worst} {f[worst]:.3g}")


def trainable(eng, seed, train=True):
    from image_matching_amd.sptrain_model import SuperPointTrainable
    m = SuperPointTrainable(eng, descriptor_length=RP.D_NET)
    m.load_state_dict(RP.load_net(RP.Net(RP.D_NET), seed).state_dict())
    return m.train(train)


@pytest.mark.parametrize("name", list(RP.NET_CASES))
def test_the_net(eng, name):
    """SuperPointTrainable with the fixture's seeded state, one training step: semi, desc, dx and the 48 parameter gradients against
    the samples the reference's blocks wrote (default bar with the reference's fp32 term) and the sums (first term), the buffers at
    1e-5 + 1e-5 |ref|, num_batches_tracked, and the eval-mode outputs; a second module with the same state gives the same bits in all 51
    tensors.  The restated all-PyTorch Net on the device goes through the same bar and both sets of fractions are printed, as the head
    test of tests/test_gpu_bn2d.py does: PyTorch's fractions are a record, not an assertion -- they depend on the convolution algorithm
    its library picks on the day (first use against a warm cache) and are not this project's to hold"""
    g = util.golden(f"spmodel_{name}.npz")
    seed = int(g["seed"])
    x, dy_s, dy_d, _, _ = (cuda(a) for a in RP.net_case(seed, name))
    names = [str(n) for n in g["names"]]
    m = trainable(eng, seed)
    ours = RP.net_grads(m, x, dy_s, dy_d)
    assert m.output is not None and set(m.output) == {"semi", "desc"}
    t = RP.load_net(RP.Net(RP.D_NET), seed).train().cuda()
    theirs = RP.net_grads(t, x, dy_s, dy_d)
    assert list(ours) == names == list(theirs) and len(names) == 51
    fo, ft = fractions(ours, g, names), fractions(theirs, g, names)
    show(f"net {name}, SuperPointTrainable", fo)
    show(f"net {name}, all PyTorch on the device (not asserted)", ft)
    assert max(fo.values()) <= 1.0, {k: v for k, v in fo.items() if v > 1.0}
    again = RP.net_grads(trainable(eng, seed), x, dy_s, dy_d)
    assert all(torch.equal(ours[k].view(torch.int32), again[k].view(torch.int32)) for k in names), [k for k in names if not torch.equal(ours[k], again[k])]
    print(f"net {name}, digest of the 51 tensors: " + hashlib.sha1(b"".join(ours[k].cpu().numpy().tobytes() for k in names)).hexdigest()[:16])
    fb = {}
    for i, (n, b) in enumerate(RP.net_buffers(m).items()):
        ref = g[f"buffer_{i}"]
        assert str(g["buffer_names"][i]) == n
        if n.endswith("num_batches_tracked"):
            assert int(b) == int(ref) == 1, n
        else:
            fb[n] = float(np.max(np.abs(b - ref) / (1e-5 + 1e-5 * np.abs(ref))))
    print(f"net {name}, buffers (of 1e-5 + 1e-5 |ref|): worst {max(fb, key=fb.get)} {max(fb.values()):.3g}")
    assert len(fb) == 24 and max(fb.values()) <= 1.0, {k: v for k, v in fb.items() if v > 1.0}
    e = trainable(eng, seed, train=False)
    with torch.no_grad():
        out = e(x)
    fe = {}
    for i, key in enumerate(("semi", "desc")):
        a, ref = out[key].double().cpu().numpy(), g[f"eval_{key}_g"]
        fe[key] = float(np.max(np.abs(a.reshape(-1)[RP.net_positions(i, a.size)] - ref) / RP.bar(ref, g[f"eval_{key}_d32"])))
    print(f"net {name}, eval mode: of the bar -- semi {fe['semi']:.3g}, desc {fe['desc']:.3g}")
    assert max(fe.values()) <= 1.0 and all(int(b) == 0 for n, b in e.named_buffers() if n.endswith("num_batches_tracked"))


def test_the_net_trains(eng):
    """4 Adam steps (lr 1e-3) of SuperPointTrainable on the `even` fixture's loss: the losses stay within the default bar of the
    reference's float64 losses (its fp32 run as the second term) and strictly decrease"""
    g = util.golden("spmodel_even.npz")
    seed = int(g["seed"])
    x, _, _, t_s, t_d = (cuda(a) for a in RP.net_case(seed, "even"))
    losses = np.array(RP.adam_losses(trainable(eng, seed), x, t_s, t_d))
    theirs = np.array(RP.adam_losses(RP.load_net(RP.Net(RP.D_NET), seed).train().cuda(), x, t_s, t_d))
    f = np.abs(losses - g["adam_g"]) / RP.bar(g["adam_g"], g["adam_d32"])
    ft = np.abs(theirs - g["adam_g"]) / RP.bar(g["adam_g"], g["adam_d32"])
    print("adam losses:", losses.tolist(), "float64:", g["adam_g"].tolist())
    print("adam: of the bar -- SuperPointTrainable " + ", ".join(f"{v:.3g}" for v in f) + "; all PyTorch on the device (not asserted) " + ", ".join(f"{v:.3g}" for v in ft))
    assert losses.shape == (RP.ADAM_STEPS,) and (f <= 1.0).all() and (np.diff(losses) < 0).all()


def test_state_dict_loads_into_the_inference_superpoint(eng):
    """state_dict() of the trainable net loads into the inference SuperPoint (superpoint/models/superpoint_train.py), whose dense
    outputs agree with the trainable net in .eval() at 1e-4 + 1e-4 |x|"""
    from image_matching_amd.superpoint.models.superpoint_train import SuperPoint as DenseSuperPoint
    seed = int(util.golden("spmodel_even.npz")["seed"])
    x = cuda(RP.net_case(seed, "even")[0])
    m = trainable(eng, seed, train=False)
    with torch.no_grad():
        out = m(x)
    net = DenseSuperPoint(descriptor_length=RP.D_NET).eval().to("cuda")
    net.load_state_dict(m.state_dict())
    dense = net(x)
    for key in ("semi", "desc"):
        assert dense[key].shape == out[key].shape
        util.assert_close(dense[key], out[key].cpu().numpy(), key)
