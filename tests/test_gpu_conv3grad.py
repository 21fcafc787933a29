"""The 3x3 convolutions of SuperPoint's network in their training form on the GPU (imx_conv3x3_forward_train, imx_conv3x3_backward,
Engine.conv3x3_forward_train, Engine.conv3x3_backward, image_matching_amd.sptrain_net) against the project's restatement in float64
(tests/conv3grad_ref.py, itself held to the reference's autograd by tests/test_conv3grad_host.py) and against the samples and sums the
reference's own double_conv and down wrote under torch.autograd (tests/golden/make_golden_conv3grad.py).  The default bar, element-wise:
|x - x64| <= max(1e-4 + 1e-4 |x64|, 2.5 |ref32 - x64|); where the reference's fp32 result is not at hand (full tensors, sums) the first
term alone, except at the long sums, whose second term is the fp32 restatement's.  Every test prints the fractions of the bar it used.
Needs an MI355X; a few seconds per test."""
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import conv3grad_ref as R
from tests import util
from tests.golden.make_golden_conv3grad import CASES, TENSORS, block_positions, channel_sums, sample_positions

gpu = pytest.mark.gpu
OUTPUTS = ("y", "dx", "dw", "db")


def new_engine():
    from image_matching_amd.engine import Engine
    return Engine(util.sp_config(128, 256), util.sg_config(128), "cuda")


@pytest.fixture(scope="module")
def eng():
    return new_engine()


def cuda(a, dtype=torch.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def call(eng, x, w, bias, dy, want=(True, True, True)):
    """forward, then backward -> dict of numpy arrays: y and those of dx, dw, db that were wanted"""
    x, w, bias, dy = cuda(x), cuda(w), cuda(bias), cuda(dy)
    res = dict(eng.conv3x3_forward_train(x, w, bias))
    res.update(eng.conv3x3_backward(x, w, dy, want=want))
    torch.cuda.synchronize()
    return {key: t.cpu().numpy() for key, t in res.items()}


@functools.lru_cache(maxsize=None)
def seeded(seed, B, Cout, Cin, H, W):
    """the inputs of a seeded case and its float64 restatement, computed once and shared (read only)"""
    inputs = R.case(seed, B, Cout, Cin, H, W)
    return inputs, R.batch_reference(*inputs)


def fractions(res, ref, ref32=None):
    """the worst fraction of the bar per tensor of y, dx, dw, db"""
    f = {}
    for t in TENSORS:
        if t in res:
            d32 = None if ref32 is None else ref32[t] - ref[t]
            f[t] = float(np.max(np.abs(res[t].astype(np.float64).reshape(ref[t].shape) - ref[t]) / R.bar(ref[t], d32)))
    return f


def show(what, f):
    print(f"{what}: of the bar -- " + ", ".join(f"{t} {v:.3g}" for t, v in f.items()))


def bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def same_bits(a, b, keys=OUTPUTS):
    return all(bits(a[k], b[k]) for k in keys if k in a and k in b)


# ---------------------------------------------------------------------------------------------- 1. the reference's fixtures
@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_reference_fixtures(eng, name):
    """samples (with the reference's fp32 term) and per-channel sums (first term) against the reference's float64 autograd.  Weights and
    images are asymmetric and not square: a transposed tap or an unflipped dx fails here."""
    g = util.golden(f"conv3grad_{name}.npz")
    seed, shape = int(g["seed"]), tuple(int(x) for x in g["shape"])
    assert (seed,) + shape == CASES[name]
    res = call(eng, *R.case(seed, *shape))
    assert all(np.isfinite(a).all() for a in res.values())
    worst = {}
    for t in TENSORS:
        got = res[t].astype(np.float64)
        pos = sample_positions(seed, t, got.size)
        worst[t] = (float(np.max(np.abs(got.reshape(-1)[pos] - g[f"{t}_g"]) / R.bar(g[f"{t}_g"], g[f"{t}_d32"]))),
                    float(np.max(np.abs(channel_sums(t, got) - g[f"{t}_sum"]) / R.bar(g[f"{t}_sum"]))))
    print(f"{name}: of the bar -- " + ", ".join(f"{t} samples {w_[0]:.3g} sums {w_[1]:.3g}" for t, w_ in worst.items()))
    assert max(max(w_) for w_ in worst.values()) <= 1.0


# ---------------------------------------------------------------------------------------------- 2. tile edges
# (Cout, Cin, H, W).  The first 24: every value of the four lists below at least twice.
EDGE_VALUES = ((1, 31, 33, 65, 129), (1, 3, 15, 33, 65), (1, 2, 7, 9, 15, 17, 33), (1, 2, 31, 33, 63, 65, 129))
EDGES = [(1, 1, 2, 1), (31, 3, 15, 2), (33, 15, 1, 31), (65, 33, 9, 33), (129, 65, 33, 63), (1, 3, 7, 65), (31, 15, 17, 129), (33, 33, 2, 1),
         (65, 65, 15, 2), (129, 1, 1, 31), (1, 15, 9, 33), (31, 33, 33, 63), (33, 65, 7, 65), (65, 1, 17, 129), (129, 3, 2, 1), (1, 33, 15, 2),
         (31, 65, 1, 31), (33, 1, 9, 33), (65, 3, 33, 63), (129, 15, 7, 65), (1, 65, 17, 129), (31, 1, 2, 1), (33, 3, 15, 2), (65, 15, 1, 31)]
# The widths the kernels use, each with a shape on either side (and on it): conv3_fwd / conv3_dx: 32 columns, 8 rows, 64 output channels in
# two blocks of 32, chunks of 8 and chains of 16 summation channels (Cin for y, Cout for dx); conv3_dw: slabs of 16 rows, 64 x 64 tiles of
# (Cout, 9 Cin + 1) -- Cin = 7 fills one tile exactly with the ones column, Cin = 64 puts the ones column alone in a tile of its own --
# chunks of 32 and chains of 128 pixels of a slab (1 x 31, 1 x 32, 1 x 33; 1 x 127, 16 x 8, 1 x 129).  Images of whole tiles on one axis and a partial tile on the
# other: 8 x 33, 16 x 31, 16 x 65, 9 x 32, 9 x 64, 17 x 32.
EXTRA = [(63, 7, 8, 33), (7, 9, 16, 31), (9, 17, 9, 64), (17, 31, 17, 32), (64, 64, 16, 65), (15, 63, 9, 32), (65, 64, 1, 127), (64, 8, 32, 5),
         (32, 16, 31, 3), (16, 32, 24, 34), (8, 14, 16, 8), (3, 5, 1, 129), (5, 2, 1, 33), (2, 5, 1, 32)]


def test_edge_list_covers_every_value_twice():
    for axis, values in enumerate(EDGE_VALUES):
        assert all(sum(e[axis] == v for e in EDGES) >= 2 for v in values) and {e[axis] for e in EDGES} == set(values)
    assert len(EDGES) == 24 and any(w % 4 for _, _, _, w in EDGES)
    shapes = EDGES + EXTRA
    for axis, widths in ((0, (8, 16, 32, 64)), (1, (8, 16, 32, 64)), (2, (8, 16)), (3, (32, 64))):
        for width in widths:
            assert all(any(e[axis] == width + d for e in shapes) for d in (-1, 0, 1)), (axis, width)
    assert any(h % 8 == 0 and w % 32 for _, _, h, w in shapes) and any(h % 8 and w % 32 == 0 for _, _, h, w in shapes)
    assert any(h % 16 == 0 and w % 32 for _, _, h, w in shapes) and any((9 * c + 1) % 64 == 0 for _, c, _, _ in shapes)
    assert any((9 * c) % 64 == 0 for _, c, _, _ in shapes) and {min(h, 16) * w for _, _, h, w in shapes} >= {31, 32, 33, 127, 128, 129}


@gpu
@pytest.mark.parametrize("Cout,Cin,H,W", EDGES + EXTRA)
def test_tile_edges(eng, Cout, Cin, H, W):
    """B = 2, full tensors against the float64 restatement at the first term alone"""
    inputs, ref = seeded(100 + Cout + 3 * Cin + 7 * H + 11 * W, 2, Cout, Cin, H, W)
    f = fractions(call(eng, *inputs), ref)
    show(f"Cout={Cout} Cin={Cin} H={H} W={W}", f)
    assert len(f) == 4 and max(f.values()) <= 1.0


# ---------------------------------------------------------------------------------------------- 3. long sums
@gpu
def test_long_sums(eng):
    """(4, 64, 64, 60, 80): dw and db sum 19 200 terms over four slabs and four images: the default bar, its second term from the fp32
    restatement on the CPU"""
    shape = (4, 64, 64, 60, 80)
    inputs, ref = seeded(7, *shape)
    res = call(eng, *inputs)
    f = fractions(res, ref, R.batch_reference(*inputs, dtype=torch.float32))
    show(f"long sums {shape} (with the fp32 restatement's term)", f)
    show(f"long sums {shape} (first term alone, not asserted)", fractions(res, ref))
    assert len(f) == 4 and max(f.values()) <= 1.0


# ---------------------------------------------------------------------------------------------- 4. bits
BITS_SHAPE = (3, 70, 33, 37, 45)                   # three slabs, two channel tiles, five chunks of summation channels


@gpu
def test_equal_bits_between_calls_histories_and_handles(eng):
    inputs, _ = seeded(46, *BITS_SHAPE)
    first = call(eng, *inputs)
    assert same_bits(first, call(eng, *inputs)), "the same call twice"
    big, _ = seeded(47, 4, 130, 70, 50, 70)
    call(eng, *big)                                                      # a larger call uses (and grows) the workspace
    assert same_bits(first, call(eng, *inputs)), "after a larger call on the same handle"
    other = new_engine()                                                 # a fresh handle: the workspace it allocates is poisoned
    other.set_option("debug_poison", "nan")
    try:
        assert same_bits(first, call(other, *inputs)), "a second handle, workspace poisoned with NaN"
        call(other, *big)
        assert same_bits(first, call(other, *inputs))
    finally:
        other.set_option("debug_poison", "off")


@gpu
def test_null_outputs_keep_the_bits(eng):
    """every subset of (dx, dw, db) has the bits of the full call; bias = NULL has the bits of a zero bias exactly"""
    inputs, _ = seeded(46, *BITS_SHAPE)
    full = call(eng, *inputs)
    for want in itertools.product((False, True), repeat=3):
        only = call(eng, *inputs, want=want)
        assert {k for k in ("dx", "dw", "db") if k in only} == {k for k, w_ in zip(("dx", "dw", "db"), want) if w_}
        assert same_bits(full, only), want
    x, w, bias, dy = inputs
    assert bits(call(eng, x, w, None, dy, want=(False,) * 3)["y"], call(eng, x, w, np.zeros_like(bias), dy, want=(False,) * 3)["y"])
    # 9 Cin a multiple of 64: db alone comes from a tile that holds nothing but the ones column
    inputs, _ = seeded(48, 2, 33, 64, 20, 21)
    assert same_bits(call(eng, *inputs), call(eng, *inputs, want=(False, False, True)))


@gpu
def test_an_image_has_the_same_bits_in_any_batch(eng):
    """y and dx of an image alone, and of the same image at positions 0 and 2 of a batch of three"""
    (x, w, bias, dy), _ = seeded(46, *BITS_SHAPE)
    alone = call(eng, x[1:2], w, bias, dy[1:2], want=(True, False, False))
    for at in (0, 2):
        order = [1, 0, 2] if at == 0 else [0, 2, 1]
        batch = call(eng, x[order], w, bias, dy[order], want=(True, False, False))
        assert bits(alone["y"][0], batch["y"][at]) and bits(alone["dx"][0], batch["dx"][at]), at


# ---------------------------------------------------------------------------------------------- 5. offsets beyond 2^32
@gpu
def test_offsets_beyond_32_bits(eng):
    """Cin = Cout = 8, H = W = 4096, B = 9: the last image starts 4.3e9 bytes into x, y, dy and dx.  y, then dx, of the last image equal
    bit for bit, on the device, the same image run as B = 1"""
    B, C, S = 9, 8, 4096
    free = torch.cuda.mem_get_info()[0]
    if free < 30 * 2 ** 30:
        print(f"skipped: {free / 2 ** 30:.1f} GiB free on the device, the test asks for 30 GiB (its allocator peak is about 10 GiB)")
        pytest.skip("not enough free device memory")
    gen = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(B, C, S, S, device="cuda", generator=gen)
    w = torch.randn(C, C, 3, 3, device="cuda", generator=gen) / 8.0
    bias = torch.randn(C, device="cuda", generator=gen)
    assert (B - 1) * C * S * S * 4 >= 2 ** 32, "every byte offset into the last image is 2^32 or more"
    last = x[B - 1:].contiguous()
    y = eng.conv3x3_forward_train(x, w, bias)["y"]
    y1 = eng.conv3x3_forward_train(last, w, bias)["y"]
    same_y = torch.equal(y[B - 1].view(torch.int32), y1[0].view(torch.int32))
    spread = float(y1.std())
    del y, y1
    dx = eng.conv3x3_backward(x, w, x, want=(True, False, False))["dx"]          # x stands for dy as well: Cin = Cout
    dx1 = eng.conv3x3_backward(last, w, last, want=(True, False, False))["dx"]
    same_dx = torch.equal(dx[B - 1].view(torch.int32), dx1[0].view(torch.int32))
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    del dx, dx1, x, last
    torch.cuda.empty_cache()
    print(f"offsets: y {'equal' if same_y else 'DIFFERENT'}, dx {'equal' if same_dx else 'DIFFERENT'}; std of y {spread:.3g}; allocator peak {peak:.1f} GiB")
    assert same_y and same_dx and spread > 0.5


# ---------------------------------------------------------------------------------------------- 6. errors
@gpu
def test_errors_are_reported_and_the_handle_survives(eng):
    from image_matching_amd.engine import ImxError
    z = lambda *s: torch.zeros(*s, device="cuda")
    for x, w_ in ((z(0, 4, 3, 3), z(2, 4, 3, 3)), (z(1, 4, 3, 3), z(1025, 4, 3, 3)), (z(1, 1025, 1, 1), z(2, 1025, 3, 3)), (z(1, 1, 4097, 1), z(1, 1, 3, 3)),
                  (z(1, 1, 1, 4097), z(1, 1, 3, 3))):
        with pytest.raises(ImxError, match="bad shape"):
            eng.conv3x3_forward_train(x, w_)
        with pytest.raises(ImxError, match="bad shape"):
            eng.conv3x3_backward(x, w_, z(x.shape[0], w_.shape[0], x.shape[2], x.shape[3]))
    with pytest.raises(ImxError, match="contiguous fp32 cuda"):
        eng.conv3x3_forward_train(z(1, 3, 4, 5).transpose(2, 3), z(2, 3, 3, 3))
    with pytest.raises(ImxError, match="contiguous fp32 cuda"):
        eng.conv3x3_forward_train(z(1, 3, 4, 5).double(), z(2, 3, 3, 3))
    with pytest.raises(ImxError, match="contiguous fp32 cuda"):
        eng.conv3x3_backward(z(1, 3, 4, 5), z(2, 3, 3, 3), z(1, 2, 4, 5).half())
    with pytest.raises(ImxError, match=r"w must be \(Cout,3,3,3\)"):
        eng.conv3x3_forward_train(z(1, 3, 4, 5), z(2, 4, 3, 3))
    with pytest.raises(ImxError, match=r"dy must be \(1,2,4,5\)"):
        eng.conv3x3_backward(z(1, 3, 4, 5), z(2, 3, 3, 3), z(1, 2, 5, 4))
    with pytest.raises(ImxError, match="three flags"):
        eng.conv3x3_backward(z(1, 3, 4, 5), z(2, 3, 3, 3), z(1, 2, 4, 5), want=(True, True))
    lib, x, w_, y, dw, db = eng.spnet, z(1, 4, 3, 8), z(2, 4, 3, 3), z(1, 2, 3, 8), z(2, 4, 3, 3), z(2)
    p = lambda t: t.data_ptr()
    err = lambda: eng.lib.imx_last_error(eng.handle)
    assert lib.imx_conv3x3_forward_train(eng.handle, 1, 2, 4, 3, 8, None, p(w_), None, p(y), None) != 0 and b"null argument" in err()
    assert lib.imx_conv3x3_forward_train(eng.handle, 1, 2, 4, 3, 8, p(x), p(w_), None, None, None) != 0 and b"null argument" in err()
    assert lib.imx_conv3x3_forward_train(eng.handle, 1, 2, 4, 3, 8, p(x), p(w_), None, p(x), None) != 0 and b"y aliases an input" in err()
    assert lib.imx_conv3x3_forward_train(eng.handle, 1, 2, 4, 3, 8, p(x), p(w_), None, p(x) + 4 * 90, None) != 0 and b"y aliases an input" in err()
    assert lib.imx_conv3x3_forward_train(eng.handle, 65535, 1024, 1024, 4096, 4096, p(x), p(w_), None, p(y), None) != 0 and b"more than a grid" in err()
    assert lib.imx_conv3x3_backward(eng.handle, 1, 2, 4, 3, 8, p(x), p(w_), None, p(x), None, None, None) != 0 and b"null argument" in err()
    assert lib.imx_conv3x3_backward(eng.handle, 1, 2, 4, 3, 8, p(x), p(w_), p(y), p(x), None, None, None) != 0 and b"dx aliases an input" in err()
    assert lib.imx_conv3x3_backward(eng.handle, 1, 2, 4, 3, 8, p(x), p(w_), p(y), None, p(w_), None, None) != 0 and b"dw aliases an input" in err()
    assert lib.imx_conv3x3_backward(eng.handle, 1, 2, 4, 3, 8, p(x), p(w_), p(y), None, p(dw), p(dw) + 4, None) != 0 and b"dw aliases db" in err()
    assert lib.imx_conv3x3_backward(eng.handle, 1, 2, 4, 3, 8, p(x), p(w_), p(y), None, None, p(y), None) != 0 and b"db aliases an input" in err()
    assert lib.imx_conv3x3_backward(eng.handle, 1, 2, 4, 3, 8, p(x), p(w_), p(y), None, None, None, None) == 0, "nothing wanted: nothing launched"
    torch.cuda.synchronize()
    assert not any(t.any() for t in (x, w_, y, dw, db)), "a refused call writes nothing"
    inputs, ref = seeded(49, 1, 5, 3, 4, 7)
    f = fractions(call(eng, *inputs), ref)
    assert max(f.values()) <= 1.0, "a valid call after the errors"


# ---------------------------------------------------------------------------------------------- 7. the bridge to autograd
@gpu
def test_autograd_bridge(eng):
    """(B, Cout, Cin, H, W) = (2, 33, 17, 19, 23): loss.backward() through sptrain_net.conv2d, and through F.conv2d, on cuda, against the
    float64 CPU autograd; y and three gradients at the first term alone"""
    from image_matching_amd import sptrain_net
    inputs = R.case(9, 2, 33, 17, 19, 23)
    ref = R.autograd(*inputs)

    def run(fn):
        leaves = [cuda(a).requires_grad_(True) for a in inputs[:3]]
        with torch.enable_grad():
            y = fn(*leaves)
            (y * cuda(inputs[3])).sum().backward()
        g = [t.grad.cpu().numpy().astype(np.float64) for t in leaves]
        return {"y": y.detach().cpu().numpy().astype(np.float64), "dx": g[0], "dw": g[1], "db": g[2]}

    ours = run(lambda x, w, b: sptrain_net.conv2d(eng, x, w, b))
    theirs = run(lambda x, w, b: torch.nn.functional.conv2d(x, w, b, padding=1))
    fo = fractions(ours, ref)
    show("bridge, sptrain_net.conv2d (first term alone)", fo)
    show("bridge, F.conv2d on the device (first term alone, not asserted)", fractions(theirs, ref))
    assert len(fo) == 4 and max(fo.values()) <= 1.0
    x = cuda(inputs[0])                                                  # needs_input_grad: the image asks for nothing, dx is not formed
    w = cuda(inputs[1]).requires_grad_(True)
    sptrain_net.conv2d(eng, x, w, None).sum().backward()
    assert w.grad is not None and x.grad is None


@gpu
@pytest.mark.parametrize("kind", list(R.BLOCKS))
def test_blocks(eng, kind):
    """the restated double_conv(3, 16) / down(16, 32) in train mode with the fixture's seeded state through sptrain_net: the output, dx and
    the 8 parameter gradients against the samples the reference's module wrote, at the default bar; the whole-tensor sums at its first
    term alone (the fixture holds them in float64 only); the buffers after the step at 1e-5 + 1e-5 |ref|; num_batches_tracked; the evaluation output;
    the convolutions' bias gradients are exactly 0 in train mode"""
    from image_matching_amd import sptrain_net
    g = util.golden(f"conv3grad_block_{kind}.npz")
    seed = int(g["seed"])
    ctor, fn = (R.DoubleConv, sptrain_net.double_conv) if kind == "double_conv" else (R.Down, sptrain_net.down)
    blocks = [R.load_block(ctor(*R.BLOCKS[kind][0]), seed).train().cuda() for _ in range(2)]
    x, dy = (cuda(a) for a in R.block_case(seed, kind))
    ours = R.block_grads(blocks[0], lambda a: fn(eng, blocks[0], a), x, dy)
    theirs = R.block_grads(blocks[1], blocks[1], x, dy)
    names = [str(n) for n in g["names"]]
    assert len(names) == 10 and set(names) == set(ours)
    fo, ft = {}, {}
    for i, name in enumerate(names):
        ref, ref_sum = g[f"{name}_g"], g[f"{name}_sum"]
        a, t = (res[name].cpu().numpy().astype(np.float64) for res in (ours, theirs))
        pos = block_positions(seed, i, a.size)
        fo[name] = max(float(np.max(np.abs(a.reshape(-1)[pos] - ref) / R.bar(ref, g[f"{name}_d32"]))),
                       float(np.max(np.abs(a.sum() - ref_sum) / R.bar(ref_sum))))
        ft[name] = max(float(np.max(np.abs(t.reshape(-1)[pos] - ref) / R.bar(ref, g[f"{name}_d32"]))),
                       float(np.max(np.abs(t.sum() - ref_sum) / R.bar(ref_sum))))
    show(f"{kind}, sptrain_net", fo)
    show(f"{kind}, all PyTorch on the device (not asserted)", ft)
    assert max(fo.values()) <= 1.0
    convs = [m for m in blocks[0].modules() if isinstance(m, torch.nn.Conv2d)]
    assert len(convs) == 2 and all(c.bias.grad is not None and not c.bias.grad.any() for c in convs), "a bias before a training BatchNorm: exactly 0"
    fb = {}
    for i, (n, b) in enumerate(R.block_buffers(blocks[0]).items()):
        ref = g[f"buffer_{i}"]
        assert str(g["buffer_names"][i]) == n
        if n.endswith("num_batches_tracked"):
            assert int(b) == int(ref) == 1
        else:
            fb[n] = float(np.max(np.abs(b - ref) / (1e-5 + 1e-5 * np.abs(ref))))
    show(f"{kind}, buffers (of 1e-5 + 1e-5 |ref|)", fb)
    assert len(fb) == 4 and max(fb.values()) <= 1.0
    e = R.load_block(ctor(*R.BLOCKS[kind][0]), seed).eval().cuda()
    with torch.no_grad():
        out = fn(eng, e, x).cpu().numpy().astype(np.float64)
    pos = block_positions(seed, 0, out.size)
    fe = float(np.max(np.abs(out.reshape(-1)[pos] - g["eval_g"]) / R.bar(g["eval_g"], g["eval_d32"])))
    print(f"{kind}, eval mode: of the bar -- out {fe:.3g}")
    assert fe <= 1.0 and int(e.conv[1].num_batches_tracked if kind == "double_conv" else e.mpconv[1].conv[1].num_batches_tracked) == 0


@gpu
def test_a_layout_that_is_not_the_reference_s_raises(eng):
    from image_matching_amd import sptrain_net
    from image_matching_amd.engine import ImxError
    x = torch.zeros(1, 3, 8, 8, device="cuda")
    bad = R.DoubleConv(3, 4).cuda()
    bad.conv[0] = torch.nn.Conv2d(3, 4, 3, padding=1, dilation=1, groups=1, stride=2).cuda()
    with pytest.raises(ImxError, match="double_conv: expected"):
        sptrain_net.double_conv(eng, bad, x)
    with pytest.raises(ImxError, match="down: expected"):
        sptrain_net.down(eng, R.DoubleConv(3, 4).cuda(), x)
    with pytest.raises(ImxError, match="contiguous fp32 cuda"):
        sptrain_net.conv2d(eng, x.transpose(2, 3), torch.zeros(4, 3, 3, 3, device="cuda"), None)
    assert sptrain_net.double_conv(eng, R.DoubleConv(3, 4).cuda(), x).shape == (1, 4, 8, 8)
