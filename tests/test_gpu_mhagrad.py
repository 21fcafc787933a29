"""The attention of SuperGlue's GNN in its training form on the GPU (imx_mha_forward_train, imx_mha_backward, Engine.mha_forward_train,
Engine.mha_backward, image_matching_amd.sgtrain_grad.attention) against the project's restatement in float64 (tests/mhagrad_ref.py,
itself held to the reference's autograd by tests/test_mhagrad_host.py) and against the samples and per-head sums the reference's own
attention wrote under torch.autograd (tests/golden/make_golden_mhagrad.py).  The default bar, element-wise:
|x - x64| <= max(1e-4 + 1e-4 |x64|, 2.5 |ref32 - x64|); where the reference's fp32 result is not at hand (full tensors, sums) the first
term alone, except at logit gain 4, whose second term is the fp32 restatement's.  Every test prints the fractions of the bar it used.
Needs an MI355X; a few seconds per test."""
import functools

import numpy as np
import pytest
import torch

from tests import mhagrad_ref as R
from tests import util
from tests.golden.make_golden_mhagrad import CASES, RAGGED_FRAME, TENSORS, sample_positions

pytestmark = pytest.mark.gpu
OUTPUTS = ("out", "lse", "dq", "dk", "dv")


def new_engine():
    from image_matching_amd.engine import Engine
    return Engine(util.sp_config(128, 256), util.sg_config(128), "cuda")


@pytest.fixture(scope="module")
def eng():
    return new_engine()


def cuda(a, dtype=torch.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def call(eng, q, k, v, dout, nq=None, nk=None, want=(True, True, True), want_lse=True):
    """forward, then backward from the forward's own out and lse -> dict of numpy arrays"""
    q, k, v, dout, nq, nk = cuda(q), cuda(k), cuda(v), cuda(dout), cuda(nq, torch.int32), cuda(nk, torch.int32)
    fwd = eng.mha_forward_train(q, k, v, nq, nk)
    res = dict(fwd)
    if not want_lse:
        res = eng.mha_forward_train(q, k, v, nq, nk, want_lse=False)
        assert set(res) == {"out"}
    res.update(eng.mha_backward(q, k, v, fwd["out"], fwd["lse"], dout, nq, nk, want=want))
    torch.cuda.synchronize()
    return {key: t.cpu().numpy() for key, t in res.items()}


@functools.lru_cache(maxsize=None)
def seeded(seed, B, D, H, N, M, gain=1.0):
    """the inputs of a seeded case and its float64 restatement, computed once and shared (read only)"""
    inputs = R.case(seed, B, D, H, N, M, gain)
    return inputs, R.batch_reference(*inputs)


def fractions(res, ref, ref32=None):
    """the worst fraction of the bar per tensor; lse against 1e-4 + 1e-4 |ref|"""
    f = {}
    for t in OUTPUTS:
        if t in res:
            d32 = None if ref32 is None or t == "lse" else ref32[t] - ref[t]
            f[t] = float(np.max(np.abs(res[t].astype(np.float64) - ref[t]) / R.bar(ref[t], d32))) if res[t].size else 0.0
    return f


def show(what, f):
    print(f"{what}: of the bar -- " + ", ".join(f"{t} {v:.3g}" for t, v in f.items()))


def same_bits(a, b, keys=OUTPUTS):
    return all(np.array_equal(a[k].view(np.int32), b[k].view(np.int32)) for k in keys if k in a and k in b)


def item(g, k):
    return {key[:-len(f"_{k}")]: v for key, v in g.items() if key.endswith(f"_{k}")}


# ---------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("name", list(CASES))
def test_reference_fixtures(eng, name):
    """samples (with the reference's fp32 term) and per-head sums (first term) against the reference's float64 autograd; on the
    single-frame cases the RMS error over the reference's own fp32 RMS error at most 2 per tensor (tests/util.py: assert_fp64_anchored's
    limit).  The ragged case runs as one NaN-padded batch."""
    g = util.golden(f"mhagrad_{name}.npz")
    items = CASES[name]
    D, H = items[0][1], items[0][2]
    N, M = RAGGED_FRAME if name == "ragged" else items[0][3:]
    B = len(items)
    q, k, v, dout = (np.full(s, np.nan, np.float32) for s in ((B, D, H, N), (B, D, H, M), (B, D, H, M), (B, D, H, N)))
    for b, (seed, _, _, n, m) in enumerate(items):
        qa, ka, va, ga = R.case(seed, 1, D, H, n, m)
        q[b, :, :, :n], k[b, :, :, :m], v[b, :, :, :m], dout[b, :, :, :n] = qa[0], ka[0], va[0], ga[0]
    nq, nk = np.array([it[3] for it in items], np.int32), np.array([it[4] for it in items], np.int32)
    res = call(eng, q, k, v, dout, nq, nk)
    assert all(np.isfinite(a).all() for a in res.values())
    worst, rms = {t: [0.0, 0.0] for t in TENSORS}, {t: 0.0 for t in TENSORS}
    for b, (seed, _, _, n, m) in enumerate(items):
        it = item(g, b)
        for t in TENSORS:
            got = np.ascontiguousarray(res[t][b, :, :, :(n if t in ("out", "dq") else m)]).astype(np.float64)
            pos = sample_positions(seed, t, got.size, B)
            err = got.reshape(-1)[pos] - it[f"{t}_g"]
            worst[t][0] = max(worst[t][0], float(np.max(np.abs(err) / R.bar(it[f"{t}_g"], it[f"{t}_d32"]))))
            worst[t][1] = max(worst[t][1], float(np.max(np.abs(got.sum(axis=(0, 2)) - it[f"{t}_sum"]) / R.bar(it[f"{t}_sum"]))))
            rms[t] = max(rms[t], float(np.sqrt(np.mean(err ** 2)) / np.sqrt(np.mean(it[f"{t}_d32"].astype(np.float64) ** 2))))
    print(f"{name}: of the bar -- " + ", ".join(f"{t} samples {w[0]:.3g} sums {w[1]:.3g}" for t, w in worst.items()))
    print(f"{name}: RMS error over the reference's fp32 RMS error -- " + ", ".join(f"{t} {r:.3g}" for t, r in rms.items()))
    assert max(max(w) for w in worst.values()) <= 1.0
    if name != "ragged":
        assert max(rms.values()) <= 2.0


SQUARE = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257]
CROSS = [(1, 129), (129, 1), (33, 257), (257, 33), (64, 1)]
EDGES = ([(32, n, n) for n in SQUARE] + [(32, n, m) for n, m in CROSS] + [(d, n, n) for d in (64, 16) for n in (33, 65, 129)])


@pytest.mark.parametrize("D,N,M", EDGES)
def test_tile_edges(eng, D, N, M):
    """B = 2, H = 2 around the 32-wide tiles and the 128-wide workgroup blocks, against the float64 restatement in full"""
    inputs, ref = seeded(100 + N + 3 * M + D, 2, D, 2, N, M)
    f = fractions(call(eng, *inputs), ref)
    show(f"D={D} {N}x{M}", f)
    assert max(f.values()) <= 1.0


@pytest.mark.parametrize("N,M", [(1024, 1024), (1, 1024)])
def test_long_sums(eng, N, M):
    """(B, D, H) = (1, 32, 1): the only shapes near the workload's own size"""
    inputs, ref = seeded(7, 1, 32, 1, N, M)
    f = fractions(call(eng, *inputs), ref)
    show(f"long sums {N}x{M}", f)
    assert max(f.values()) <= 1.0


def test_logit_gain(eng):
    """130 x 130, D = 32, H = 2: gain 2 on q and k (logits 4 times as large) at the first term alone; gain 4 (16 times) with the second
    term, taken from the fp32 restatement on the CPU"""
    inputs, ref = seeded(8, 1, 32, 2, 130, 130, 2.0)
    f2 = fractions(call(eng, *inputs), ref)
    show("gain 2", f2)
    inputs, ref = seeded(8, 1, 32, 2, 130, 130, 4.0)
    res = call(eng, *inputs)
    f4 = fractions(res, ref, R.batch_reference(*inputs, dtype=torch.float32))
    show("gain 4 (with the fp32 restatement's term)", f4)
    show("gain 4 (first term alone, not asserted)", fractions(res, ref))
    assert max(f2.values()) <= 1.0 and max(f4.values()) <= 1.0


# ---------------------------------------------------------------------------------------------- ragged batches
RAGGED = [(130, 140), (77, 3), (1, 140), (0, 50)]


def ragged_batch(D=32, H=2, N=130, M=140, fill=np.nan):
    q, k, v, dout = (np.full(s, fill, np.float32) for s in ((4, D, H, N), (4, D, H, M), (4, D, H, M), (4, D, H, N)))
    alone = []
    for b, (n, m) in enumerate(RAGGED):
        qa, ka, va, ga = R.case(40 + b, 1, D, H, max(n, 1), m)
        q[b, :, :, :n], k[b, :, :, :m], v[b, :, :, :m], dout[b, :, :, :n] = qa[0, :, :, :n], ka[0], va[0], ga[0, :, :, :n]
        alone.append((qa, ka, va, ga))
    return (q, k, v, dout), np.array([c[0] for c in RAGGED], np.int32), np.array([c[1] for c in RAGGED], np.int32), alone


def test_ragged_batch(eng):
    """four pairs in one (130, 140) frame, NaN on the padding of every input: the valid region equals the pair alone bit for bit, the
    rest is 0; NULL counts equal full counts"""
    inputs, nq, nk, alone = ragged_batch()
    res = call(eng, *inputs, nq, nk)
    assert all(np.isfinite(a).all() for a in res.values()), "NaN padding leaked"
    f = fractions(res, R.batch_reference(*inputs, nq, nk))
    show("ragged", f)
    assert max(f.values()) <= 1.0
    for b, (n, m) in enumerate(RAGGED):
        for t, cnt in (("out", n), ("dq", n), ("dk", m), ("dv", m)):
            assert not res[t][b, :, :, cnt:].any(), (b, t)
        assert not res["lse"][b, :, n:].any()
        if n == 0:
            assert all(not res[t][b].any() for t in OUTPUTS)
            continue
        one = call(eng, *alone[b])
        for t, cnt in (("out", n), ("dq", n), ("dk", m), ("dv", m)):
            assert np.array_equal(res[t][b, :, :, :cnt].view(np.int32), one[t][0].view(np.int32)), (b, t)
        assert np.array_equal(res["lse"][b, :, :n].view(np.int32), one["lse"][0].view(np.int32))
    full, _ = seeded(45, 2, 32, 2, 70, 90)
    assert same_bits(call(eng, *full), call(eng, *full, np.array([70, 70], np.int32), np.array([90, 90], np.int32))), "NULL means all"
    assert same_bits(call(eng, *full), call(eng, *full, np.array([99, 1 << 30], np.int32), np.array([90, 91], np.int32))), "counts are clamped to the frame"


# ---------------------------------------------------------------------------------------------- determinism
def test_equal_bits_between_calls_batches_histories_and_handles(eng):
    inputs, nq, nk, _ = ragged_batch()
    first = call(eng, *inputs, nq, nk)
    assert same_bits(first, call(eng, *inputs, nq, nk)), "the same call twice"
    five, _ = seeded(46, 5, 32, 2, 100, 70)
    batch, one = call(eng, *five), call(eng, *(a[3:4] for a in five))
    assert all(np.array_equal(batch[t][3:4].view(np.int32), one[t].view(np.int32)) for t in OUTPUTS), "a pair alone against the same pair in a batch of 5"
    big, _ = seeded(47, 3, 64, 4, 300, 200)
    call(eng, *big)                                                      # another shape uses (and grows) the workspace
    assert same_bits(first, call(eng, *inputs, nq, nk)), "after a call at another shape"
    other = new_engine()                                                 # a fresh handle: the workspace it allocates is poisoned
    other.set_option("debug_poison", "nan")
    try:
        assert same_bits(first, call(other, *inputs, nq, nk)), "a second handle, workspace poisoned with NaN"
        call(other, *big)
        assert same_bits(first, call(other, *inputs, nq, nk))
    finally:
        other.set_option("debug_poison", "off")


def test_null_outputs_keep_the_bits(eng):
    inputs, ref = seeded(48, 2, 32, 2, 130, 97)
    full = call(eng, *inputs)
    for i, t in enumerate(("dq", "dk", "dv")):
        want = tuple(j == i for j in range(3))
        only = call(eng, *inputs, want=want)
        assert {"dq", "dk", "dv"} & set(only) == {t} and same_bits(full, only), t
    value = call(eng, *inputs, want_lse=False)
    assert "lse" not in value and same_bits(full, value), "lse = NULL gives the same out"


def test_errors_are_reported_and_the_handle_survives(eng):
    from image_matching_amd.engine import ImxError
    z = lambda *s: torch.zeros(*s, device="cuda")
    with pytest.raises(ImxError, match="head dimension 48"):
        eng.mha_forward_train(z(1, 48, 1, 4), z(1, 48, 1, 4), z(1, 48, 1, 4))
    with pytest.raises(ImxError, match="bad shape"):
        eng.mha_forward_train(z(0, 32, 4, 8), z(0, 32, 4, 8), z(0, 32, 4, 8))
    with pytest.raises(ImxError, match="bad shape"):
        eng.mha_backward(z(0, 32, 4, 8), z(0, 32, 4, 8), z(0, 32, 4, 8), z(0, 32, 4, 8), z(0, 4, 8), z(0, 32, 4, 8))
    lib, t = eng.train, z(1, 32, 1, 8)
    p = lambda x: x.data_ptr()
    assert lib.imx_mha_forward_train(eng.handle, 1, 1, 32, 8, 8, None, p(t), p(t), None, None, p(t), None, None) != 0
    assert b"null argument" in eng.lib.imx_last_error(eng.handle)
    assert lib.imx_mha_backward(eng.handle, 1, 1, 32, 8, 8, None, p(t), p(t), p(t), p(t), p(t), None, None, p(t), None, None, None) != 0
    assert b"null argument" in eng.lib.imx_last_error(eng.handle)
    inputs, ref = seeded(49, 1, 16, 1, 5, 7)
    f = fractions(call(eng, *inputs), ref)
    assert max(f.values()) <= 1.0, "a valid call after the errors"


# ---------------------------------------------------------------------------------------------- the bridge to autograd
class MultiHeadedAttention(torch.nn.Module):
    """superglue_train.py:89-104 restated, with the attention function as an argument"""

    def __init__(self, num_heads, d_model):
        super().__init__()
        self.dim, self.num_heads = d_model // num_heads, num_heads
        self.merge = torch.nn.Conv1d(d_model, d_model, kernel_size=1)
        self.proj = torch.nn.ModuleList([torch.nn.Conv1d(d_model, d_model, kernel_size=1) for _ in range(3)])

    def forward(self, attention, query, key, value):
        b = query.size(0)
        query, key, value = [l(x).view(b, self.dim, self.num_heads, -1) for l, x in zip(self.proj, (query, key, value))]
        x, _ = attention(query, key, value)
        return self.merge(x.contiguous().view(b, self.dim * self.num_heads, -1))


def bridge_grads(module, attention, x, src, dy):
    """the gradients of sum(module(x, src, src) * dy): the two input features, then the eight weight and bias tensors"""
    module.zero_grad()
    x, src = x.clone().requires_grad_(True), src.clone().requires_grad_(True)
    with torch.enable_grad():
        y = module(attention, x, src, src)
        (y * dy).sum().backward()
    return [x.grad, src.grad] + [p.grad.clone() for p in module.parameters()]


def test_autograd_bridge(eng):
    """d_model = 128, 4 heads, N = 70, M = 100: loss.backward() through sgtrain_grad.attention, and through the einsum form, on cuda,
    against the float64 CPU autograd of the einsum form; ten gradients, each at the default bar on its own values"""
    from image_matching_amd import sgtrain_grad
    from image_matching_amd.engine import ImxError
    torch.manual_seed(3)
    m64 = MultiHeadedAttention(4, 128).double()
    x, src, dy = (torch.from_numpy(R.heavy(9, n, s)) for n, s in (("x", (1, 128, 70)), ("src", (1, 128, 100)), ("dy", (1, 128, 70))))
    ref = [g.numpy() for g in bridge_grads(m64, R.attention_einsum, x.double(), src.double(), dy.double())]
    mc = MultiHeadedAttention(4, 128).cuda()
    mc.load_state_dict({k_: v_.float() for k_, v_ in m64.state_dict().items()})
    ours = bridge_grads(mc, lambda q, k, v: sgtrain_grad.attention(eng, q, k, v), x.cuda(), src.cuda(), dy.cuda())
    eins = bridge_grads(mc, R.attention_einsum, x.cuda(), src.cuda(), dy.cuda())
    names = ["x", "source"] + [n for n, _ in mc.named_parameters()]
    fo = {n: float(np.max(np.abs(g.cpu().numpy() - r) / R.bar(r))) for n, g, r in zip(names, ours, ref)}
    fe = {n: float(np.max(np.abs(g.cpu().numpy() - r) / R.bar(r))) for n, g, r in zip(names, eins, ref)}
    show("bridge, sgtrain_grad.attention", fo)
    show("bridge, einsum form", fe)
    assert len(fo) == 10 and max(fo.values()) <= 1.0 and max(fe.values()) <= 1.0
    with pytest.raises(ImxError, match="contiguous fp32 cuda"):
        q = torch.zeros(1, 32, 4, 8, device="cuda")
        sgtrain_grad.attention(eng, q.transpose(2, 3), q, q)


def test_memory_stays_below_one_probability_matrix(eng):
    """(B, D, H, N, M) = (1, 32, 4, 1024, 1024): torch's allocator peak over the bridge's forward plus backward(), above what was
    allocated before, stays below B H N M 4 bytes (16 MiB, one probability matrix); the einsum form cannot meet that"""
    from image_matching_amd import sgtrain_grad
    B, D, H, N, M = 1, 32, 4, 1024, 1024
    q, k, v, dout = (cuda(a) for a in R.case(10, B, D, H, N, M))

    def peak(attention):
        leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        with torch.enable_grad():
            out = attention(*leaves)[0]
            out.backward(dout)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    ours, eins = peak(lambda a, b, c: sgtrain_grad.attention(eng, a, b, c)), peak(R.attention_einsum)
    print(f"allocator peak above the baseline: sgtrain_grad.attention {ours / 2**20:.2f} MiB, einsum form {eins / 2**20:.2f} MiB, one matrix {B * H * N * M * 4 / 2**20:.0f} MiB")
    assert ours < B * H * N * M * 4 <= eins
