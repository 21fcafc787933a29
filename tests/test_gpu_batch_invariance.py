"""Batch-size invariance under "latency_forms" = off (include/imx.h): a pair's results do not depend on the batch it
is matched in, bit for bit -- the premise of the multi-GPU record gather, which compares pairs matched in shards with the same pairs
matched as one batch.  Several kernel choices depend on the batch size: the Sinkhorn slab group G (sg_misc.hip, launch_sinkhorn),
the two-query-block attention (attention_x3.hip, "attention_qblocks" = auto) and the pair / tile form of the Winograd layers.  Here
every pair is compared bitwise across batch sizes on both sides of each threshold, and the results are anchored to the oracle's
float64 evaluation at 1e-4 + 1e-4|ref| in every batch-size regime.  Also the A/B switch "qkv_amax" on a layer whose attention the
weights-derived guard moves to bf16x3 while the linear layers stay on the fp16 planes.  Needs an MI355X."""
import numpy as np
import pytest
import torch

from tests import util
from tests.test_gpu_strict import _matching_t, _strict_inputs

pytestmark = pytest.mark.gpu
HEADS = 4


def _sinkhorn_group(N0p, N1p, B):
    """The auto rule of the Sinkhorn slab group (sg_misc.hip: sinkhorn_auto_group; sinkhorn_slab_rows for R)."""
    R = 8 if N1p <= 2048 else 4
    nsl = N0p // R + 1
    slots = 1024 if N1p <= 1024 else 512
    return 4 if (nsl + 3) // 4 * B >= slots else 2 if (nsl + 1) // 2 * B >= slots else 1


def _attention_qblocks(Np, d, B):
    """The auto rule of the two-query-block attention (attention_x3.hip, launch_attention_x3): head dim 32, whole 256-query blocks."""
    return 2 if d // HEADS == 32 and Np % 256 == 0 and (Np + 127) // 128 * HEADS * 2 * B >= 1024 else 1


# fixture -> batch sizes: each side of every G threshold (and, at C3, of the qblocks threshold at B = 16)
BATCHES = {"strict_c3.npz": (1, 15, 16, 31, 32, 64), "strict_c5.npz": (1, 3, 4, 7, 8)}
ANCHOR = {"strict_c3.npz": (1, 16, 32), "strict_c5.npz": (1, 4, 8)}      # one batch per G regime: float64-anchored pair by pair
CHOSEN = 5                                                                  # the fixture seed index placed at the first, middle and last slot


def _slots(B, n):
    idx = [b % n for b in range(B)]
    for b in (0, B // 2, B - 1):
        idx[b] = CHOSEN
    return idx


def _run(eng, per_seed, idx, H, W):
    """One imx_superglue_forward over the fixture seeds idx (one pair per slot); per slot: matches, scores and the pair's taps."""
    cat = lambda k: torch.cat([per_seed[s][0][k] for s in idx]).cuda()
    out = eng.superglue(cat("keypoints0"), cat("scores0"), cat("descriptors0"), (1, 1, H, W),
                        cat("keypoints1"), cat("scores1"), cat("descriptors1"), (1, 1, H, W))
    torch.cuda.synchronize()
    m0, m1, ms0, ms1 = (o.cpu().numpy() for o in out)
    X, S, U, V = eng.fetch("x"), eng.fetch("scores_in"), eng.fetch("u"), eng.fetch("v")
    B, N0p, N1p = S.shape
    res = []
    for b in range(B):
        res.append({"matches0": m0[b], "matches1": m1[b], "matching_scores0": ms0[b], "matching_scores1": ms1[b],
                    "x0": X[b * N0p:(b + 1) * N0p], "x1": X[B * N0p + b * N1p:B * N0p + (b + 1) * N1p],
                    "scores_in": S[b], "u": U[b], "v": V[b]})
    return res, (N0p, N1p)


def _anchor(g, s, r, ref, K, alpha, thr, tag):
    """gnn17 / scores_in / Z against the oracle's float64 values, every element; match indices under the strict rule."""
    Z = util.transport_Z(r["scores_in"], r["u"], r["v"], K, K, alpha)
    gnn = np.stack([r["x0"][:K].T, r["x1"][:K].T])
    for key, mine, full in (("gnn17", gnn, np.stack([ref["gnn0"], ref["gnn1"]])), ("scores_in", r["scores_in"][:K, :K], ref["scores_in"]), ("Z", Z, ref["Z"])):
        util.assert_close(mine, full, f"{tag}: {key} vs the oracle, every element")
    util.strict_index_check(g, s, r["matches0"], r["matches1"], thr, tag)


@pytest.mark.parametrize("name", ["strict_c3.npz", "strict_c5.npz"])
def test_superglue_bitwise_across_batch_sizes(name):
    """SuperGlue alone on the strict fixture's inputs: every pair of batches of B = 1 .. 64 (C3) / 1 .. 8 (C5) -- both sides of every
    threshold of the Sinkhorn group rule and of the qblocks rule -- bitwise equal to the same pair at B = 1 (matches, matching scores,
    gnn17, scores_in, u, v), the chosen seed at the first, middle and last slot; the distinct pairs of one batch per regime anchored
    to the float64 oracle; and a control that the comparison sees a change of G at all."""
    g, per_seed = _strict_inputs(name)
    H, W, d, K = (int(g[k]) for k in ("H", "W", "d", "K"))
    n = len(g["seeds"])
    from image_matching_amd import _lib as L
    from image_matching_amd.engine import Engine
    eng = Engine(util.sp_config(d, K), util.sg_config(d), "cuda")
    sd = util.sg_sd(d, variant="t")
    eng.load_state_dict(L.NET_SUPERGLUE, sd)
    eng.set_option("latency_forms", "off")
    eng.set_debug(True)
    alpha, thr = float(sd["bin_score"]), float(util.sg_config(d)["match_threshold"])
    Bs = BATCHES[name]
    Np = (K + 127) // 128 * 128
    # the batch sizes must straddle the rules as they stand: if a threshold moves, this says the set is stale
    assert {_sinkhorn_group(Np, Np, B) for B in Bs} == {1, 2, 4}, f"{name}: batch sizes {Bs} no longer reach G = 1, 2 and 4"
    assert {_sinkhorn_group(Np, Np, B) for B in ANCHOR[name]} == {1, 2, 4}, ANCHOR[name]
    if d == 128:
        assert {_attention_qblocks(Np, d, B) for B in Bs} == {1, 2}, f"{name}: batch sizes {Bs} no longer straddle the qblocks rule"

    single = {}
    for s in range(n):
        single[s] = _run(eng, per_seed, [s], H, W)[0][0]
    anchored = {}
    for B in Bs[1:]:
        idx = _slots(B, n)
        res, _ = _run(eng, per_seed, idx, H, W)
        for b, s in enumerate(idx):
            for key, val in res[b].items():
                assert np.array_equal(val, single[s][key]), (f"{name}: seed {int(g['seeds'][s])} at slot {b} of a {B}-pair batch (G = {_sinkhorn_group(Np, Np, B)} "
                                                             f"under the auto rule): {key} differs from the same pair at B = 1")
        if B in ANCHOR[name]:
            for s in sorted(set(idx)):
                _anchor(g, s, res[idx.index(s)], per_seed[s][1], K, alpha, thr, f"{name} seed {int(g['seeds'][s])} in a {B}-pair batch")
            anchored[B] = sorted(int(g["seeds"][s]) for s in set(idx))
    _anchor(g, CHOSEN, single[CHOSEN], per_seed[CHOSEN][1], K, alpha, thr, f"{name} seed {int(g['seeds'][CHOSEN])} alone")
    anchored[1] = [int(g["seeds"][CHOSEN])]

    # control: forcing the group the auto rule would pick at other batch sizes changes the potentials' low bits
    seen = []
    for s in (CHOSEN, 0, 1):
        got = {}
        for G in ("1", "4"):
            eng.set_option("sinkhorn_group", G)
            got[G] = _run(eng, per_seed, [s], H, W)[0][0]
        seen.append(not (np.array_equal(got["1"]["u"], got["4"]["u"]) and np.array_equal(got["1"]["v"], got["4"]["v"])))
    eng.set_option("sinkhorn_group", "auto")
    assert any(seen), f"{name}: u and v are bitwise equal under sinkhorn_group 1 and 4 on seed indices {(CHOSEN, 0, 1)}: the test cannot see a change of G"
    print(f"[batch invariance] {name}: B = {Bs} bitwise equal to B = 1 on every slot; float64-anchored: "
          + "; ".join(f"B = {B} (G = {_sinkhorn_group(Np, Np, B)} under auto): seeds {v}" for B, v in sorted(anchored.items()))
          + f"; G control differs on {sum(seen)} of 3 seeds")


def test_records_of_shards_straddling_the_group_rule_equal_one_batch():
    """Images in (C3, 640x480, "t" weights): the records of 40 pairs matched as one batch, as two round-robin shards of 20 and as five
    shards of 8 -- G = 4, 2 and 1 under the auto rule -- equal byte for byte after sorting by pair id (the sharding premise of
    tests/multi_gpu_worker.py); and a pair at B = 1 equals the same pair inside the 40-pair batch (keypoints, descriptors, scores)."""
    from image_matching_amd import shard
    d, K, H, W = 128, 1024, 480, 640
    m = _matching_t(d, K)
    m._shared.get_engine([0, 1]).set_option("latency_forms", "off")
    n_pairs, distinct = 40, 8
    ims = [util.pair(4100 + i, H, W) for i in range(distinct)]
    assert [_sinkhorn_group(K, K, b) for b in (40, 20, 8)] == [4, 2, 1]

    def run(ids, want_desc=False):
        i0 = torch.cat([ims[i % distinct][0] for i in ids]).cuda()
        i1 = torch.cat([ims[i % distinct][1] for i in ids]).cuda()
        out = m.match_batch(i0, i1, want_desc=want_desc)
        torch.cuda.synchronize()
        return out

    whole_out = run(list(range(n_pairs)), want_desc=True)
    whole = shard.sort_by_pair_id(shard.pack_records(list(range(n_pairs)), whole_out)).cpu()
    for world in (2, 5):
        parts = torch.cat([shard.pack_records(ids, run(ids)) for ids in (shard.shard_indices(n_pairs, r, world) for r in range(world))])
        mine = shard.sort_by_pair_id(parts).cpu()
        assert mine.shape == whole.shape
        rows = [int(i) for i in torch.nonzero((mine != whole).any(1)).flatten()]
        assert not rows, f"{world} shards of {n_pairs // world}: the records of pairs {rows[:8]} differ from the {n_pairs}-pair batch ({len(rows)} in all)"
    one = run([3], want_desc=True)
    for k in ("keypoints0", "keypoints1", "scores0", "scores1", "descriptors0", "descriptors1", "matches0", "matches1", "matching_scores0", "matching_scores1"):
        for b in (3, 3 + distinct, 3 + 4 * distinct):
            assert torch.equal(one[k][0], whole_out[k][b]), f"pair 3 alone vs slot {b} of the {n_pairs}-pair batch: {k} differs"
    print(f"[batch invariance] records of {n_pairs} pairs: one batch == 2 x 20 == 5 x 8, byte for byte; pair 3 alone == its slots in the batch")


# ---------------------------------------------------------------------------------------------- qkv_amax on a guarded layer
GUARD_LAYER, FLAT_CH, FLAT_A, V_GAIN = 5, 17, 2.0 ** 8, 2.0 ** 4


def _guards(sd, l, d):
    """Host restatement of the two weights-derived guards on layer l's q|k|v (imx_host.h: attn_f16x2_ok, gemm_h2_weights_ok): the attention's -- per projection,
    largest / median column L2 norm -- and the linear layers' (split_f16x2) -- largest |w| / median column maximum over q|k|v."""
    Ws = [np.asarray(sd[f"gnn.layers.{l}.attn.proj.{w}.weight"], np.float64) for w in range(3)]
    att = max(np.sqrt((w ** 2).sum(1)).max() / np.sort(np.sqrt((w ** 2).sum(1)))[d // 2] for w in Ws)
    cm = np.concatenate([np.abs(w).max(1) for w in Ws])
    return att, np.abs(np.concatenate(Ws)).max() / np.sort(cm)[cm.size // 2]


def _guarded_superglue(d):
    """A "t" SuperGlue weight set on which layer GUARD_LAYER's attention runs bf16x3 while every linear layer stays on fp16 planes:
    q channel FLAT_CH made flat (every weight +-FLAT_A: its L2 norm is sqrt(d) times its maximum, so the attention guard trips while
    the linear guard, which reads maxima, does not), the matching k channel scaled down to keep the q.k logits of that channel at
    their size; the whole v projection scaled up by V_GAIN and attn.merge scaled down by the same power of two (exact for the
    network), so max |v| sits above max |x| and the maxima table's v word decides gnn_mlp1's scale."""
    from image_matching_amd import synth
    sd = synth.make_superglue_state_dict(d, variant="t")
    p = f"gnn.layers.{GUARD_LAYER}.attn"
    q = sd[f"{p}.proj.0.weight"]
    f = np.float32(2.0 ** -np.round(np.log2(np.sqrt(d) * FLAT_A / np.linalg.norm(q[FLAT_CH].astype(np.float64)))))
    q[FLAT_CH] = np.where(q[FLAT_CH] < 0, -FLAT_A, FLAT_A).astype(np.float32)
    sd[f"{p}.proj.1.weight"][FLAT_CH] *= f
    sd[f"{p}.proj.1.bias"][FLAT_CH] *= f
    sd[f"{p}.proj.2.weight"] *= np.float32(V_GAIN)
    sd[f"{p}.proj.2.bias"] *= np.float32(V_GAIN)
    sd[f"{p}.merge.weight"] *= np.float32(1.0 / V_GAIN)
    att, lin = _guards(sd, GUARD_LAYER, d)
    assert att > 4096 and lin <= 4096, f"construction: attention spread {att:.0f} (must exceed 2^12), linear spread {lin:.0f} (must not)"
    return sd


def test_qkv_amax_switch_agrees_on_a_guarded_layer_with_the_linear_layers_on_fp16():
    """descriptor_dim 256 (the layer tail unfused), K = 512: with lin_h2 on, gnn_mlp1 scales [x | att] by the (side, pair) maxima
    of x and v.  On a layer whose attention the guard sends to bf16x3, "qkv_amax" = kernel must still produce those maxima: the two
    switch settings agree bit for bit, every output is finite, and both sit inside 1e-4 + 1e-4|ref| of the float64 oracle on the
    same weights with the oracle's match indices (except on a row whose float64 score is within the tolerance of the threshold)."""
    from image_matching_amd import _lib as L
    from image_matching_amd.engine import Engine
    from tests import oracle_jobs
    d, K = 256, 512
    g, per_seed = _strict_inputs("strict_c5.npz")
    H, W = int(g["H"]), int(g["W"])
    data = {k: v[..., :K] if k.startswith("descriptors") else v[:, :K] for k, v in per_seed[0][0].items()}
    sd = _guarded_superglue(d)
    eng = Engine(util.sp_config(d, K), util.sg_config(d), "cuda")
    eng.load_state_dict(L.NET_SUPERGLUE, util.to_torch(sd))
    eng.set_option("latency_forms", "off")
    guard = eng.get_option("arith_guard")
    assert guard.split("attention bf16x3 layers:")[1].split("(")[0].split() == [str(GUARD_LAYER)], guard
    assert "-> f16x2" in guard.split("linear:")[1], guard
    eng.set_debug(True)
    res = {}
    for mode in ("epilogue", "kernel"):
        eng.set_option("qkv_amax", mode)
        eng.timing_reset()
        eng.set_timing(True)
        out = eng.superglue(data["keypoints0"].cuda(), data["scores0"].cuda(), data["descriptors0"].cuda(), (1, 1, H, W),
                            data["keypoints1"].cuda(), data["scores1"].cuda(), data["descriptors1"].cuda(), (1, 1, H, W))
        torch.cuda.synchronize()
        forms = {r[0]: r[3] for r in eng.timing_report(forms=True)}
        eng.set_timing(False)
        assert forms["gnn_mlp1"] == forms["qkv_proj"] == "gemm_h2:f16x2", forms
        r = dict(zip(("matches0", "matches1", "matching_scores0", "matching_scores1"), (o.cpu().numpy()[0] for o in out)))
        r.update({k: eng.fetch(k) for k in ("x", "scores_in", "u", "v")})
        for k in ("x", "scores_in", "u", "v", "matching_scores0", "matching_scores1"):
            assert np.isfinite(r[k]).all(), f"qkv_amax = {mode}: {k} has non-finite values"
        res[mode] = r
    for k in res["epilogue"]:
        assert np.array_equal(res["epilogue"][k], res["kernel"][k]), f"qkv_amax epilogue vs kernel: {k} differs"
    ref = oracle_jobs.pool_map(oracle_jobs.superglue_f64_job, [(sd, dict({k: v.numpy() for k, v in data.items()}, image_shape0=(1, 1, H, W),
                                                                        image_shape1=(1, 1, H, W)), d)])[0]
    alpha, thr = float(sd["bin_score"]), float(util.sg_config(d)["match_threshold"])
    r = res["kernel"]
    S = r["scores_in"][0, :K, :K]
    Z = util.transport_Z(r["scores_in"][0], r["u"][0], r["v"][0], K, K, alpha)
    gnn = np.stack([r["x"][:K].T, r["x"][K:2 * K].T])
    for key, mine, full in (("gnn17", gnn, np.stack([ref["gnn0"], ref["gnn1"]])), ("scores_in", S, ref["scores_in"]), ("Z", Z, ref["Z"])):
        util.assert_close(mine, full, f"guarded layer {GUARD_LAYER}: {key} vs the float64 oracle, every element")
    # match indices: the oracle's, except where the float64 candidate score is within the tolerance of the threshold
    band = (util.ATOL + util.RTOL * thr) / thr
    for side, mine, want in ((0, r["matches0"], ref["matches0"]), (1, r["matches1"], ref["matches1"])):
        Zs = ref["Z"][:-1, :-1] if side == 0 else ref["Z"][:-1, :-1].T
        cand = Zs.argmax(1)
        near = np.abs(Zs[np.arange(K), cand] - np.log(thr)) < band
        diff = np.nonzero(mine != want)[0]
        bad = [int(i) for i in diff if not (near[i] and {int(mine[i]), int(want[i])} == {-1, int(cand[i])})]
        assert not bad, f"guarded layer: matches{side} differ from the float64 oracle's on {bad[:8]} ({len(diff)} differ in all)"
    print(f"[batch invariance] qkv_amax epilogue == kernel bitwise on the guarded weights ({guard}); float64 oracle: "
          + ", ".join(f"{k} {util.tolerance_used(a, b):.3f}" for k, a, b in (("gnn17", gnn, np.stack([ref['gnn0'], ref['gnn1']])), ("scores_in", S, ref["scores_in"]), ("Z", Z, ref["Z"]))))
