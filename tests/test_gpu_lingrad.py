"""The 1x1 convolutions of SuperGlue's GNN in their training form on the GPU (imx_conv1x1_forward_train, imx_conv1x1_backward,
Engine.conv1x1_forward_train, Engine.conv1x1_backward, image_matching_amd.sgtrain_grad.conv1d / attentional_propagation) against the
project's restatement in float64 (tests/lingrad_ref.py, itself held to the reference's autograd by tests/test_lingrad_host.py) and
against the samples and per-channel sums the reference's own MLP and AttentionalPropagation wrote under torch.autograd
(tests/golden/make_golden_lingrad.py).  The default bar, element-wise: |x - x64| <= max(1e-4 + 1e-4 |x64|, 2.5 |ref32 - x64|); where the
reference's fp32 result is not at hand (full tensors, sums) the first term alone, except at the two long sums, whose second term is the
fp32 restatement's.  Every test prints the fractions of the bar it used.  Needs an MI355X; a few seconds per test."""
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import lingrad_ref as R
from tests import util
from tests.golden.make_golden_lingrad import CASES, LAYER, RAGGED_FRAME, TENSORS, channel_sums, layer_positions, sample_positions

pytestmark = pytest.mark.gpu
OUTPUTS = ("y", "dx0", "dx1", "dw", "db")


def new_engine():
    from image_matching_amd.engine import Engine
    return Engine(util.sp_config(128, 256), util.sg_config(128), "cuda")


@pytest.fixture(scope="module")
def eng():
    return new_engine()


def cuda(a, dtype=torch.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def call(eng, x0, x1, w, bias, dy, n=None, want=(True, True, True, True)):
    """forward, then backward -> dict of numpy arrays: y, those of dx0, dx1, dw, db that were wanted, and dx (both, concatenated)"""
    x0, x1, w, bias, dy, n = cuda(x0), cuda(x1), cuda(w), cuda(bias), cuda(dy), cuda(n, torch.int32)
    res = dict(eng.conv1x1_forward_train(x0, w, bias, x1=x1, n=n))
    res.update(eng.conv1x1_backward(x0, w, dy, x1=x1, n=n, want=want))
    torch.cuda.synchronize()
    res = {key: t.cpu().numpy() for key, t in res.items()}
    if "dx0" in res and ("dx1" in res or x1 is None):
        res["dx"] = np.concatenate([res["dx0"], res["dx1"]], 1) if x1 is not None else res["dx0"]
    return res


@functools.lru_cache(maxsize=None)
def seeded(seed, B, Cout, C0, C1, N):
    """the inputs of a seeded case and its float64 restatement, computed once and shared (read only)"""
    inputs = R.case(seed, B, Cout, C0, C1, N)
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


def item(g, k):
    return {key[:-len(f"_{k}")]: v for key, v in g.items() if key.endswith(f"_{k}")}


# ---------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("name", list(CASES))
def test_reference_fixtures(eng, name):
    """samples (with the reference's fp32 term) and per-channel sums (first term) against the reference's float64 autograd.  The ragged
    case runs as one NaN-padded batch of three in a frame of 64: y and dx per pair, dw and db of the batch against the float64 sum of the
    items' values (the gradient is linear in the pairs) at the first term."""
    g = util.golden(f"lingrad_{name}.npz")
    items = CASES[name]
    seed0, Cout, C0, C1 = items[0][:4]
    N, B = (RAGGED_FRAME if name == "ragged" else items[0][4]), len(items)
    x0, x1, dy = (np.full(s, np.nan, np.float32) for s in ((B, C0, N), (B, max(C1, 1), N), (B, Cout, N)))
    for b, (seed, _, _, _, n) in enumerate(items):
        a0, a1, w, bias, ga = R.case(seed, 1, Cout, C0, C1, n, wseed=seed0)
        x0[b, :, :n], dy[b, :, :n] = a0[0], ga[0]
        if C1:
            x1[b, :, :n] = a1[0]
    res = call(eng, x0, x1 if C1 else None, w, bias, dy, np.array([it[4] for it in items], np.int32))
    assert all(np.isfinite(a).all() for a in res.values())
    worst = {t: [0.0, 0.0] for t in TENSORS}

    def hold(t, got, ref, d32, ref_sum):
        pos = sample_positions(seed0, t, got.size, B)
        worst[t][0] = max(worst[t][0], float(np.max(np.abs(got.reshape(-1)[pos] - ref) / R.bar(ref, d32))))
        worst[t][1] = max(worst[t][1], float(np.max(np.abs(channel_sums(t, got) - ref_sum) / R.bar(ref_sum))))

    for b, (_, _, _, _, n) in enumerate(items):
        it = item(g, b)
        for t in ("y", "dx"):
            hold(t, np.ascontiguousarray(res[t][b:b + 1, :, :n]).astype(np.float64), it[f"{t}_g"], it[f"{t}_d32"], it[f"{t}_sum"])
    for t in ("dw", "db"):
        total = lambda key: sum(item(g, b)[f"{t}_{key}"].astype(np.float64) for b in range(B))
        hold(t, res[t].astype(np.float64).reshape(Cout, -1) if t == "dw" else res[t].astype(np.float64), total("g"),
             item(g, 0)[f"{t}_d32"] if B == 1 else None, total("sum"))
    print(f"{name}: of the bar -- " + ", ".join(f"{t} samples {w_[0]:.3g} sums {w_[1]:.3g}" for t, w_ in worst.items()))
    assert max(max(w_) for w_ in worst.values()) <= 1.0


# (Cout, Cin, N): every value at least twice; N % 4 != 0 together with Cin % 4 != 0 in most
EDGES = [(1, 1, 1), (1, 3, 31), (31, 1, 33), (31, 33, 127), (33, 3, 129), (33, 129, 257), (127, 257, 513), (127, 33, 1), (129, 129, 31),
         (129, 257, 33), (1, 257, 127), (31, 129, 129), (33, 33, 257), (127, 3, 513), (129, 1, 1), (1, 33, 513), (31, 3, 257),
         (33, 257, 31), (127, 129, 33), (129, 33, 127), (1, 129, 129), (31, 257, 1), (33, 1, 513), (127, 1, 127)]


def test_edge_list_covers_every_value_twice():
    for axis, values in enumerate(((1, 31, 33, 127, 129), (1, 3, 33, 129, 257), (1, 31, 33, 127, 129, 257, 513))):
        assert all(sum(e[axis] == v for e in EDGES) >= 2 for v in values) and {e[axis] for e in EDGES} == set(values)
    assert len(EDGES) == 24 and any(n % 4 and c % 4 for _, c, n in EDGES)


@pytest.mark.parametrize("Cout,Cin,N", EDGES)
def test_tile_edges(eng, Cout, Cin, N):
    """B = 2, the input channels split in two sources (one source at Cin = 1), around the 32-wide chunks, the 64-wide tiles, the 128-wide
    blocks and the 256-wide slabs, against the float64 restatement in full at the first term alone"""
    C0 = (Cin + 1) // 2
    inputs, ref = seeded(100 + Cout + 3 * Cin + 7 * N, 2, Cout, C0, Cin - C0, N)
    f = fractions(call(eng, *inputs), ref)
    show(f"Cout={Cout} Cin={C0}+{Cin - C0} N={N}", f)
    assert len(f) == 4 and max(f.values()) <= 1.0


@pytest.mark.parametrize("shape", [(1, 512, 256, 256, 1024), (4, 128, 128, 128, 1024)])
def test_long_sums(eng, shape):
    """the only shapes near the workload's own size: the default bar, its second term from the fp32 restatement on the CPU"""
    inputs, ref = seeded(7, *shape)
    res = call(eng, *inputs)
    f = fractions(res, ref, R.batch_reference(*inputs, dtype=torch.float32))
    show(f"long sums {shape} (with the fp32 restatement's term)", f)
    show(f"long sums {shape} (first term alone, not asserted)", fractions(res, ref))
    assert len(f) == 4 and max(f.values()) <= 1.0


@pytest.mark.parametrize("C0", [1, 3, 127, 128, 130, 259])
def test_two_sources_have_the_bits_of_one(eng, C0):
    """Cin = 260 split at C0: y, dw, db have the bits of the single-source call on the concatenated tensor, dx0 / dx1 of its dx ranges"""
    (x, _, w, bias, dy), _ = seeded(60, 2, 70, 260, 0, 77)
    one = call(eng, x, None, w, bias, dy)
    two = call(eng, x[:, :C0], x[:, C0:], w, bias, dy)
    assert bits(one["y"], two["y"]) and bits(one["dw"], two["dw"]) and bits(one["db"], two["db"])
    assert bits(one["dx0"][:, :C0], two["dx0"]) and bits(one["dx0"][:, C0:], two["dx1"])


# ---------------------------------------------------------------------------------------------- ragged batches
RAGGED = (300, 5, 1, 0)
SHAPE = (70, 40, 30)                              # Cout, C0, C1


def ragged_batch(frame=300, counts=RAGGED, fill=np.nan):
    Cout, C0, C1 = SHAPE
    x0, x1, dy = (np.full(s, fill, np.float32) for s in ((len(counts), C0, frame), (len(counts), C1, frame), (len(counts), Cout, frame)))
    _, _, w, bias, _ = R.case(40, 1, Cout, C0, C1, 1)
    alone = []
    for b, n in enumerate(counts):
        a0, a1, _, _, ga = R.case(40 + b, 1, Cout, C0, C1, max(n, 1))
        x0[b, :, :n], x1[b, :, :n], dy[b, :, :n] = a0[0, :, :n], a1[0, :, :n], ga[0, :, :n]
        alone.append((a0, a1, w, bias, ga))
    return (x0, x1, w, bias, dy), np.array(counts, np.int32), alone


def test_ragged_batch(eng):
    """four pairs in one frame of 300 with counts (300, 5, 1, 0), NaN on the padding of x0, x1 and dy: finite, 0 past the counts, y and
    dx of each pair equal the pair alone at its own frame bit for bit; dw and db equal the batch without the empty pair and the batch in
    a larger frame; NULL counts equal full counts and counts are clamped"""
    inputs, n, alone = ragged_batch()
    res = call(eng, *inputs, n)
    assert all(np.isfinite(a).all() for a in res.values()), "NaN padding leaked"
    f = fractions(res, R.batch_reference(*inputs, n))
    show("ragged", f)
    assert max(f.values()) <= 1.0
    for b, cnt in enumerate(RAGGED):
        for t in ("y", "dx0", "dx1"):
            assert not res[t][b, :, cnt:].any(), (b, t)
        if cnt:
            one = call(eng, *alone[b])
            assert all(bits(res[t][b, :, :cnt], one[t][0]) for t in ("y", "dx0", "dx1")), b
    without = call(eng, *(a[:3] if a.ndim == 3 else a for a in inputs), n[:3])
    assert bits(res["dw"], without["dw"]) and bits(res["db"], without["db"]), "the empty pair adds nothing"
    wide, n_wide, _ = ragged_batch(frame=337)
    larger = call(eng, *wide, n_wide)
    assert bits(res["dw"], larger["dw"]) and bits(res["db"], larger["db"]), "the frame does not enter the order"
    assert all(bits(res[t], larger[t][:, :, :300]) for t in ("y", "dx0", "dx1"))
    full, _ = seeded(45, 2, 33, 20, 13, 90)
    assert same_bits(call(eng, *full), call(eng, *full, np.array([90, 90], np.int32))), "NULL means all"
    assert same_bits(call(eng, *full), call(eng, *full, np.array([91, 1 << 30], np.int32))), "counts are clamped to the frame"
    empty = call(eng, *full, np.array([0, -3], np.int32))
    assert all(not empty[t].any() for t in OUTPUTS), "no valid column anywhere: zeros, dw and db included"


# ---------------------------------------------------------------------------------------------- determinism
def test_equal_bits_between_calls_histories_and_handles(eng):
    inputs, n, _ = ragged_batch()
    first = call(eng, *inputs, n)
    assert same_bits(first, call(eng, *inputs, n)), "the same call twice"
    big, _ = seeded(47, 3, 200, 150, 150, 600)
    call(eng, *big)                                                      # a larger call uses (and grows) the workspace
    assert same_bits(first, call(eng, *inputs, n)), "after a larger call on the same handle"
    other = new_engine()                                                 # a fresh handle: the workspace it allocates is poisoned
    other.set_option("debug_poison", "nan")
    try:
        assert same_bits(first, call(other, *inputs, n)), "a second handle, workspace poisoned with NaN"
        call(other, *big)
        assert same_bits(first, call(other, *inputs, n))
    finally:
        other.set_option("debug_poison", "off")


def test_null_outputs_keep_the_bits(eng):
    """every subset of (dx0, dx1, dw, db) has the bits of the full call; bias = NULL has the bits of a zero bias exactly (the running sum
    is never -0, so the last add of +0 changes nothing)"""
    inputs, _ = seeded(48, 2, 70, 65, 64, 130)
    full = call(eng, *inputs)
    for want in itertools.product((False, True), repeat=4):
        only = call(eng, *inputs, want=want)
        assert {k for k in ("dx0", "dx1", "dw", "db") if k in only} == {k for k, w_ in zip(("dx0", "dx1", "dw", "db"), want) if w_}
        assert same_bits(full, only), want
    x0, x1, w, bias, dy = inputs
    assert bits(call(eng, x0, x1, w, None, dy)["y"], call(eng, x0, x1, w, np.zeros_like(bias), dy)["y"])
    single = call(eng, x0, None, np.ascontiguousarray(w[:, :65]), bias, dy, want=(True, True, False, False))
    assert "dx1" not in single and "dx0" in single, "want[1] is ignored without x1"


def test_errors_are_reported_and_the_handle_survives(eng):
    from image_matching_amd.engine import ImxError
    z = lambda *s: torch.zeros(*s, device="cuda")
    for x, w_ in ((z(0, 4, 3), z(2, 4)), (z(1, 4, 3), z(1025, 4)), (z(1, 1025, 1), z(2, 1025)), (z(1, 1, (1 << 20) + 1), z(1, 1))):
        with pytest.raises(ImxError, match="bad shape"):
            eng.conv1x1_forward_train(x, w_)
        with pytest.raises(ImxError, match="bad shape"):
            eng.conv1x1_backward(x, w_, z(x.shape[0], w_.shape[0], x.shape[2]))
    with pytest.raises(ImxError, match="contiguous fp32 cuda"):
        eng.conv1x1_forward_train(z(1, 3, 4).transpose(1, 2), z(2, 4))
    with pytest.raises(ImxError, match=r"w must be \(Cout,4\)"):
        eng.conv1x1_forward_train(z(1, 4, 3), z(2, 5))
    lib, x, w_, y = eng.train, z(1, 4, 8), z(2, 4), z(1, 2, 8)
    p = lambda t: t.data_ptr()
    err = lambda: eng.lib.imx_last_error(eng.handle)
    assert lib.imx_conv1x1_forward_train(eng.handle, 1, 2, 4, 0, 8, p(x), p(x), p(w_), None, None, p(y), None) != 0 and b"x1 given with C1 = 0" in err()
    assert lib.imx_conv1x1_forward_train(eng.handle, 1, 2, 2, 2, 8, p(x), None, p(w_), None, None, p(y), None) != 0 and b"x1 is null with C1 = 2" in err()
    assert lib.imx_conv1x1_forward_train(eng.handle, 1, 2, 4, 0, 8, None, None, p(w_), None, None, p(y), None) != 0 and b"null argument" in err()
    assert lib.imx_conv1x1_forward_train(eng.handle, 1, 2, 4, 0, 8, p(x), None, p(w_), None, None, None, None) != 0 and b"null argument" in err()
    assert lib.imx_conv1x1_backward(eng.handle, 1, 2, 4, 0, 8, p(x), None, p(w_), None, None, p(x), None, None, None, None) != 0 and b"null argument" in err()
    assert lib.imx_conv1x1_backward(eng.handle, 1, 2, 4, 0, 8, p(x), None, p(w_), p(y), None, None, p(x), None, None, None) != 0 and b"dx1 given with C1 = 0" in err()
    assert lib.imx_conv1x1_backward(eng.handle, 1, 2, 4, 0, 8, p(x), p(x), p(w_), p(y), None, p(x), None, None, None, None) != 0 and b"x1 given with C1 = 0" in err()
    assert lib.imx_conv1x1_backward(eng.handle, 1, 2, 4, 0, 8, p(x), None, p(w_), p(y), None, None, None, None, None, None) == 0, "nothing wanted: nothing launched"
    inputs, ref = seeded(49, 1, 5, 3, 2, 7)
    f = fractions(call(eng, *inputs), ref)
    assert max(f.values()) <= 1.0, "a valid call after the errors"


# ---------------------------------------------------------------------------------------------- the bridge to autograd
def test_autograd_bridge(eng):
    """(B, Cout, C0, C1, N) = (2, 256, 128, 128, 100): loss.backward() through sgtrain_grad.conv1d, and through F.conv1d(torch.cat(...)), on
    cuda, against the float64 CPU autograd; y and four gradients at the default bar, its second term from PyTorch's result on the device"""
    from image_matching_amd import sgtrain_grad
    inputs = R.case(9, 2, 256, 128, 128, 100)
    ref = R.autograd(*inputs)

    def run(fn):
        leaves = [cuda(a).requires_grad_(True) for a in inputs[:4]]
        leaves[2] = cuda(inputs[2][:, :, None]).requires_grad_(True)     # the (Cout, Cin, 1) parameter itself
        with torch.enable_grad():
            y = fn(*leaves)
            (y * cuda(inputs[4])).sum().backward()
        g = [t.grad.cpu().numpy().astype(np.float64) for t in leaves]
        return {"y": y.detach().cpu().numpy().astype(np.float64), "dx": np.concatenate(g[:2], 1), "dw": g[2][:, :, 0], "db": g[3]}

    ours = run(lambda x0, x1, w, b: sgtrain_grad.conv1d(eng, x0, w, b, x1=x1))
    theirs = run(lambda x0, x1, w, b: torch.nn.functional.conv1d(torch.cat([x0, x1], 1), w, b))
    fo, ft = fractions(ours, ref, theirs), fractions(theirs, ref)
    show("bridge, sgtrain_grad.conv1d (default bar)", fo)
    show("bridge, sgtrain_grad.conv1d (first term alone, not asserted)", fractions(ours, ref))
    show("bridge, F.conv1d on torch.cat (first term alone, not asserted)", ft)
    assert len(fo) == 4 and max(fo.values()) <= 1.0
    x = cuda(inputs[0]).requires_grad_(True)                             # needs_input_grad: only x asks, dw and db are not formed
    sgtrain_grad.conv1d(eng, x, cuda(inputs[2][:, :128].copy()), None).sum().backward()
    assert x.grad is not None and x.grad.shape == x.shape


def test_attentional_propagation_layer(eng):
    """the restated AttentionalPropagation(128, 4) in train mode with the fixture's seeded parameters, x (1,128,70), source (1,128,100):
    attentional_propagation's output, dx, dsource and every parameter gradient (14: six convolutions and the BatchNorm, weight and
    bias) against the samples the reference's module wrote, at the default bar, and the whole-tensor sums at the default bar
    with the all-PyTorch layer's term; running_mean /
    running_var after the step equal those of the all-PyTorch layer on the same device to 1e-5"""
    from image_matching_amd import sgtrain_grad
    g = util.golden("lingrad_layer.npz")
    seed, d, heads, N, M = LAYER
    layers = []
    for _ in range(2):
        m = R.AttentionalPropagation(d, heads).train()
        m.load_state_dict({k: torch.from_numpy(v) for k, v in R.layer_parameters(seed, m).items()}, strict=False)
        layers.append(m.cuda())
    x, source, dy = (cuda(a) for a in R.layer_case(seed, d, N, M))
    ours = R.layer_grads(layers[0], lambda a, b: sgtrain_grad.attentional_propagation(eng, layers[0], a, b), x, source, dy)
    theirs = R.layer_grads(layers[1], layers[1], x, source, dy)
    names = [str(n) for n in g["names"]]
    assert len(names) == 17 and set(names) == set(ours)
    fo, ft = {}, {}
    for i, name in enumerate(names):
        ref, ref_sum = g[f"{name}_g"], g[f"{name}_sum"]
        a, t = (res[name].cpu().numpy().astype(np.float64) for res in (ours, theirs))
        pos = layer_positions(seed, i, a.size)
        # the samples at the default bar (the reference's own fp32 term); the whole-tensor sum, thousands of rounded terms, with
        # the second term of the all-PyTorch layer on this device
        fo[name] = max(float(np.max(np.abs(a.reshape(-1)[pos] - ref) / R.bar(ref, g[f"{name}_d32"]))),
                       float(np.max(np.abs(a.sum() - ref_sum) / R.bar(ref_sum, t.sum() - ref_sum))))
        ft[name] = max(float(np.max(np.abs(t.reshape(-1)[pos] - ref) / R.bar(ref, g[f"{name}_d32"]))),
                       float(np.max(np.abs(t.sum() - ref_sum) / R.bar(ref_sum))))
    show("layer, attentional_propagation", fo)
    show("layer, all PyTorch on the device (sums at the first term alone)", ft)
    assert max(fo.values()) <= 1.0
    bn0, bn1 = layers[0].mlp[1], layers[1].mlp[1]
    assert int(bn0.num_batches_tracked) == 1
    assert torch.allclose(bn0.running_mean, bn1.running_mean, rtol=1e-5, atol=1e-5) and torch.allclose(bn0.running_var, bn1.running_var, rtol=1e-5, atol=1e-5)
