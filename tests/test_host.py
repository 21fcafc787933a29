"""Host-side checks that need no GPU: the C-ABI library loads and exports what include/imx.h
declares, config plumbing, state-dict key contracts, portable synthetic data, sharding/records."""
import ctypes
import os
import re
import zlib

import numpy as np
import pytest
import torch

from image_matching_amd import _lib, shard, synth
from tests import util

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_library_exports_every_declared_symbol():
    lib = _lib.load_library()
    header = open(os.path.join(ROOT, "include", "imx.h")).read()
    declared = set(re.findall(r"\b(imx_[a-z0-9_]+)\s*\(", header))
    assert declared, "no declarations parsed"
    for name in declared:
        assert hasattr(lib, name), f"libimx.so does not export {name}"
    assert set(_lib.EXPORTS) == declared
    assert b"gfx950" in lib.imx_version()


def test_library_exports_nothing_but_the_declared_symbols():
    """the library is built with -fvisibility=hidden and a linker version script (csrc/imx.map), so its dynamic
    symbol table is exactly the C ABI of include/imx.h -- none of the ~60 mangled imx::launch_* symbols of round 5, no vague-linkage
    C++ symbols."""
    import shutil
    import subprocess
    if not shutil.which("nm"):
        pytest.skip("nm not present")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    defined = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    header = open(os.path.join(ROOT, "include", "imx.h")).read()
    declared = set(re.findall(r"\b(imx_[a-z0-9_]+)\s*\(", header))
    assert defined == declared, f"extra: {sorted(defined - declared)[:8]} missing: {sorted(declared - defined)[:8]}"
    assert all(re.search(r"^IMX_API [^\n]*\b" + n + r"\(", header, re.M) for n in declared), "an entry point lacks IMX_API"


def test_header_is_plain_c_and_the_c_example_links(tmp_path):
    """include/imx.h must be consumable from C (it is the drop-in boundary, not a C++/torch header): the plain-C
    example compiles as C99, links against libimx.so + the HIP runtime only, and -- with no GPU here -- exits through
    imx_create's clean "no HIP device" error rather than any CPU fallback."""
    import shutil
    import subprocess
    if not shutil.which("gcc") or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("gcc / ROCm headers not present")
    exe = str(tmp_path / "abi_example")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                    "-D__HIP_PLATFORM_AMD__", os.path.join(ROOT, "examples", "abi_example.c"), "-L" + libdir, "-limx",
                    "-L/opt/rocm/lib", "-lamdhip64", "-o", exe], check=True)
    env = dict(os.environ, LD_LIBRARY_PATH=libdir + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert "gfx950" in r.stdout
    if not torch.cuda.is_available():
        assert r.returncode == 2 and "no CPU path" in r.stderr


def test_config_struct_matches_header_layout():
    # 7 SuperPoint words + 1 + 64 + 1 + 8 + 2 = 83 32-bit words
    assert ctypes.sizeof(_lib.ImxConfig) == 4 * (7 + 1 + _lib.IMX_MAX_GNN_LAYERS + 1 + _lib.IMX_MAX_KENC + 2)


def test_no_gpu_fails_loudly():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from image_matching_amd.engine import Engine, ImxError
    with pytest.raises(ImxError, match="no CPU fallback"):
        Engine({}, {}, "cuda")
    lib = _lib.load_library()
    h = ctypes.c_void_p()
    cfg = _lib.ImxConfig()
    cfg.descriptor_dim, cfg.kenc_n, cfg.num_gnn_layers = 128, 3, 18
    assert lib.imx_create(0, ctypes.byref(cfg), ctypes.byref(h)) != 0
    assert b"no HIP device" in lib.imx_last_error(None)


def test_create_rejects_bad_config():
    lib = _lib.load_library()
    h = ctypes.c_void_p()
    cfg = _lib.ImxConfig()
    cfg.descriptor_dim, cfg.kenc_n, cfg.num_gnn_layers = 102, 3, 18      # not a multiple of 4
    assert lib.imx_create(0, ctypes.byref(cfg), ctypes.byref(h)) != 0
    assert b"descriptor_dim" in lib.imx_last_error(None)


def test_dropin_classes_config_and_state_dict_contract():
    from image_matching_amd.superglue.models.matching_test import Matching
    cfg = {"superpoint": util.sp_config(128, 1024), "superglue": util.sg_config(128)}
    m = Matching(cfg).eval().to("cuda")                      # chainable like superpoint_glue_test.py:69
    assert m.superpoint.config["keypoint_threshold"] == 0.005 and m.superglue.config["match_threshold"] == 0.1
    assert m.superpoint.config["remove_borders"] == 4        # default merged in
    assert m.superglue.config["GNN_layers"] == ["self", "cross"] * 9
    sp_keys, sg_keys = set(m.superpoint.state_dict()), set(m.superglue.state_dict())
    assert "inc.conv.conv.0.weight" in sp_keys and "down3.mpconv.1.conv.4.running_var" in sp_keys and "bnDb.bias" in sp_keys
    assert "bin_score" in sg_keys and "gnn.layers.17.attn.proj.2.weight" in sg_keys and "kenc.encoder.9.bias" in sg_keys
    n_sp = sum(v.numel() for k, v in m.superpoint.state_dict().items() if "running" not in k and "tracked" not in k)
    n_sg = sum(v.numel() for k, v in m.superglue.state_dict().items() if "running" not in k and "tracked" not in k)
    assert (n_sp, n_sg) == (1270915, 3018497)                # SURVEY §8b parameter counts at d=128
    with pytest.raises(RuntimeError, match="Missing key"):
        m.superpoint.load_state_dict({"convPa.weight": torch.zeros(256, 128, 3, 3)})
    with pytest.raises(RuntimeError, match="size mismatch"):
        sd = m.superglue.state_dict()
        sd["final_proj.weight"] = torch.zeros(64, 128, 1)
        m.superglue.load_state_dict(sd)
    with pytest.raises(KeyError):                            # reference quirk: no 'weights' default (superpoint_test.py:87)
        from image_matching_amd.superpoint.models.superpoint_test import SuperPoint
        SuperPoint({})
    with pytest.raises(RuntimeError, match="inference-only"):
        m.train()


def test_module_prefix_checkpoint_loading(tmp_path):
    """superpoint_test.py:87-99: {'model_state_dict': ...} with 'module.' prefixes from DataParallel."""
    from image_matching_amd.superpoint.models.superpoint_test import SuperPoint
    sd = util.sp_sd(128)
    path = tmp_path / "ckpt.pth.tar"
    torch.save({"n_iter": 1, "model_state_dict": {"module." + k: v for k, v in sd.items()}}, path)
    sp = SuperPoint(util.sp_config(128, 10, weights=str(path)))
    got = sp.state_dict()
    assert all(torch.equal(got[k], sd[k]) for k in sd)


def test_synth_is_portable_and_stable():
    """Bit-identical synthetic data on any machine: CRCs recorded in the build container."""
    im0, im1 = synth.synth_pair(59, 480, 640)
    sd = synth.make_superpoint_state_dict(128)
    sg = synth.make_superglue_state_dict(128)
    crcs = (zlib.crc32(im0.tobytes()), zlib.crc32(im1.tobytes()),
            zlib.crc32(sd["down2.mpconv.1.conv.3.weight"].tobytes()), zlib.crc32(sd["bnPb.running_var"].tobytes()),
            zlib.crc32(sg["gnn.layers.7.mlp.0.weight"].tobytes()))
    assert crcs == EXPECTED_CRCS, crcs
    assert im0.dtype == np.float32 and 0.0 <= im0.min() and im0.max() <= 1.0


EXPECTED_CRCS = (3817531681, 2015118848, 543481260, 1157619473, 3903334769)


def test_shard_and_records_roundtrip():
    assert shard.shard_indices(10, 1, 4) == [1, 5, 9]
    assert sorted(sum((shard.shard_indices(512, r, 8) for r in range(8)), [])) == list(range(512))
    B, K = 3, 16
    g = torch.Generator().manual_seed(0)
    out = {"keypoints0": torch.rand(B, K, 2, generator=g) * 600, "keypoints1": torch.rand(B, K, 2, generator=g) * 600,
           "counts0": torch.tensor([16, 12, 0], dtype=torch.int32), "counts1": torch.tensor([16, 16, 5], dtype=torch.int32),
           "matches0": torch.randint(-1, K, (B, K), generator=g), "matches1": torch.randint(-1, K, (B, K), generator=g),
           "matching_scores0": torch.rand(B, K, generator=g), "matching_scores1": torch.rand(B, K, generator=g)}
    rec = shard.pack_records([7, 8, 9], out)
    assert rec.shape == (B, shard.record_width(K))
    back = shard.unpack_records(rec)
    assert back["pair_id"].tolist() == [7, 8, 9]
    for k in out:
        assert torch.equal(back[k], out[k]), k
    assert shard.gather_records(rec) is rec                   # world_size 1: no process group needed


def test_cli_flags_match_reference_and_kenc_string_parsing():
    """superpoint_glue_test.py:17-35: every reference flag exists with the same default."""
    import superpoint_glue_test as cli
    opt = cli.build_parser().parse_args([])
    ref_defaults = {"exper_name": "superpoint_glue_descriptor", "img_dir": "datasets/Amazon/", "Result_dir": "Results/Amazon/",
                    "resize_scale": 0.125, "match_viz": True, "show_keypoints": True, "descriptor_dim": 128,
                    "superpoint_weights": "superpoint/models/weights/superPointNet_allss_descriptor_128.pth.tar",
                    "keypoint_threshold": 0.005, "nms_radius": 4, "max_keypoints": -1,
                    "superglue_weights": "superglue/models/weights/SuperGlue_allss_descriptor_128.pth",
                    "keypoint_encoder": [32, 64, 128], "sinkhorn_iterations": 30, "match_threshold": 0.1}
    for k, v in ref_defaults.items():
        assert getattr(opt, k) == v, k
    opt = cli.build_parser().parse_args(["--keypoint_encoder", "[32, 64]", "--max_keypoints", "100"])
    cfg = cli.make_config(opt)
    assert cfg["superglue"]["keypoint_encoder"] == [32, 64] and cfg["superpoint"]["max_keypoints"] == 100
    assert cfg["superpoint"]["weights"] is None            # LFS-pointer / absent checkpoint -> synthetic weights


def test_official_cli_flags_match_reference():
    """superpoint_glue_official_test.py:16-33: every reference flag exists with the same default (typo included)."""
    import superpoint_glue_official_test as cli
    opt = cli.build_parser().parse_args([])
    ref_defaults = {"exper_name": "superpoint_glue_official", "img_dir": "datasets/Camera/", "Result_dir": "Results/Camera/",
                    "resize_scale": 0.125, "match_viz": True, "show_keypoints": True, "descriptor_dim": 256,
                    "superpoint_weights": "supeeglue/models/weights/superpoint_v1.pth",
                    "superglue_weights": "superglue/models/weights/superglue_indoor.pth",
                    "sinkhorn_iterations": 30, "match_threshold": 0.1, "keypoint_threshold": 0.005, "nms_radius": 4,
                    "max_keypoints": -1}
    for k, v in ref_defaults.items():
        assert getattr(opt, k) == v, k
    cfg = cli.make_config(opt)
    assert cfg["superpoint"]["weights_path"] is None and cfg["superglue"]["weights"] is None
    assert "keypoint_encoder" not in cfg["superglue"]          # the official CLI leaves the d=256 default encoder


def test_flann_cli_flags_match_reference():
    """superpoint_flann_test.py:16-26: every reference flag exists with the same default."""
    import superpoint_flann_test as cli
    opt = cli.build_parser().parse_args([])
    ref_defaults = {"img_dir": "datasets/Amazon/", "Result_dir": "Results/Camera/superpoint_allss_descriptor_128",
                    "resize_scale": 0.25, "match_viz": True,
                    "weights_path": "superpoint/models/weights/superPointNet_allss_descriptor_128.pth.tar",
                    "descriptor_dim": 128, "max_keypoints": 1200, "keypoint_threshold": 0.005, "nms_radius": 4}
    for k, v in ref_defaults.items():
        assert getattr(opt, k) == v, k
    assert cli.MIN_MATCH_COUNT == 4 and cli.RATIO == 0.7
    c = cli.match_colors(np.array([0.0, 0.5, 1.0], np.float32), 128)       # dist <= 1 -> worst = 1
    assert c.shape == (3, 4) and np.all((c >= 0) & (c <= 1))


def test_hostops_similarity_ransac_and_warp():
    from image_matching_amd import hostops
    rng = np.random.RandomState(1)
    src = rng.rand(60, 2) * 400
    th, s = 0.1, 1.1
    R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]) * s
    dst = src @ R.T + [5, -3]
    dst[:12] += rng.rand(12, 2) * 200 + 20                  # outliers
    M, mask = hostops.estimate_affine_partial_2d(src, dst, ransac_thresh=7)
    np.testing.assert_allclose(M, np.concatenate([R, [[5], [-3]]], 1), atol=1e-6)
    assert mask.sum() == 48 and not mask[:12].any()
    img = rng.rand(40, 60) * 255
    w = hostops.warp_affine(img, np.array([[1, 0, 3], [0, 1, 2.0]]), (60, 40))
    np.testing.assert_allclose(w[5, 10], img[3, 7])


def test_superglue_checkpoint_formats(tmp_path):
    """superglue_test.py:221-227: {'net': state_dict} for self-trained checkpoints, a bare state dict when
    the path contains 'indoor'/'outdoor'; the user's (not the merged) config is indexed for the path."""
    from image_matching_amd.superglue.models.superglue_test import SuperGlue
    sd = util.sg_sd(128)
    p_net, p_ind = tmp_path / "SuperGlue_allss.pth", tmp_path / "superglue_indoor.pth"
    torch.save({"epoch": 3, "net": sd}, p_net)
    torch.save(sd, p_ind)
    for path in (p_net, p_ind):
        sg = SuperGlue(util.sg_config(128, weights=str(path)))
        got = sg.state_dict()
        assert all(torch.equal(got[k], sd[k]) for k in sd)
    with pytest.raises(KeyError):       # default 'weights': 'indoor' is truthy but the user's dict has no key (:222)
        SuperGlue({"descriptor_dim": 128, "keypoint_encoder": [32, 64, 128]})


def test_winograd_f2x4_matrices_reproduce_the_direct_convolution():
    """The 3x3 layers run as Winograd F(2x4,3x3) (conv1ab_wino24.hip, conv3x3_wino24.hip; U = G2 g G4^T is built in
    wino24_pack.h).  The transform matrices those files use must satisfy  Y = A2^T [(G2 g G4^T) (.) (B2^T d B4)] A4  ==  the
    direct 3x3 correlation of a 4x6 patch, exactly in float64 (F.conv2d semantics: no kernel flip)."""
    rng = np.random.default_rng(0)
    BT2 = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float64)
    G2 = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=np.float64)
    AT2 = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float64)
    BT4 = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                    [0, 4, 0, -5, 0, 1]], dtype=np.float64)
    G4 = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6],
                   [0, 0, 1]], dtype=np.float64)
    AT4 = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=np.float64)
    for _ in range(8):
        g, d = rng.standard_normal((3, 3)), rng.standard_normal((4, 6))
        U = G2 @ g @ G4.T                       # 4 x 6
        V = BT2 @ d @ BT4.T                     # 4 x 6
        Y = AT2 @ (U * V) @ AT4.T               # 2 x 4
        ref = np.array([[(g * d[y:y + 3, x:x + 3]).sum() for x in range(4)] for y in range(2)])
        np.testing.assert_allclose(Y, ref, rtol=0, atol=1e-12)


def test_traditional_plumbing_flags_and_skip_line(capsys):
    """BASELINE configs[0] (traditional.py:8-57): the reference's flags and defaults; without OpenCV the script prints one
    skip line and returns instead of failing (the arithmetic is OpenCV's: no GPU path, no parity claim)."""
    import traditional
    from Traditional import registration
    opt = traditional.build_parser().parse_args([])
    assert (opt.Method, opt.img_dir, opt.Result_dir, opt.resize_scale, opt.match_viz) == \
        ('SIFT', 'datasets/Amazon/', 'Results/Amazon/', 0.5, True)
    assert registration.MIN_MATCH_COUNT == 10 and registration.RATIO == 0.7
    if registration.cv2 is None:
        assert traditional.main([]) == []
        assert "skipped" in capsys.readouterr().out


def test_bench_plans_the_c4_job_without_a_gpu():
    """VERDICT r3 task 5: bench.py's own argument / environment handling for an 8-rank launch, far enough to see who gets which
    pairs: `--plan-only` under WORLD_SIZE=8, RANK=r prints this rank's pair ids and the padded record rows.  The eight shards must
    partition the 512 pairs of BASELINE configs[3] (pair i -> rank i mod 8, 64 per rank), and a --gpus / WORLD_SIZE disagreement
    must be refused."""
    import json
    import subprocess
    import sys
    bench = os.path.join(ROOT, "bench.py")
    seen = []
    for r in range(8):
        env = dict(os.environ, WORLD_SIZE="8", RANK=str(r), LOCAL_RANK=str(r))
        out = subprocess.run([sys.executable, bench, "--gpus", "8", "--steps", "20", "--warmup", "2", "--plan-only"], env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        pl = json.loads(out.stdout.strip().splitlines()[-1])
        assert pl["world"] == 8 and pl["rank"] == r and pl["global_pairs"] == 512 and pl["rows_per_rank"] == 64
        assert pl["pair_ids"] == list(range(r, 512, 8))
        seen += pl["pair_ids"]
    assert sorted(seen) == list(range(512))
    bad = subprocess.run([sys.executable, bench, "--gpus", "4", "--plan-only"], env=dict(os.environ, WORLD_SIZE="8", RANK="0"), capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "WORLD_SIZE=8" in (bad.stderr + bad.stdout)


def test_bench_dump_outputs_float_arrays_within_the_byte_budget(tmp_path, monkeypatch):
    """bench.py --dump-outputs writes through dump_outputs(): floating arrays as float32, integer arrays as float64 (exact); over
    the byte budget an array larger than its share is replaced by a sample at fixed, seeded positions (the same in every run),
    the smaller arrays stay whole and the files together fit the budget."""
    import importlib
    # bench.py sets a default for this variable at import: keep the test process's environment as it was
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    bench = importlib.import_module("bench")
    rng = np.random.RandomState(0)
    arrays = {"keypoints0": torch.from_numpy(rng.rand(4, 50, 2).astype(np.float32)), "matches0": torch.arange(200).reshape(4, 50) - 1,
              "counts0": np.array([50, 50, 49, 50], np.int32), "descriptors0": rng.rand(100000)}
    limit = 200000
    metas = [bench.dump_outputs(arrays, str(tmp_path / run), limit=limit) for run in ("a", "b")]
    assert metas[0] == metas[1]
    files = {run: {k: np.load(tmp_path / run / (k + ".npy")) for k in arrays} for run in ("a", "b")}
    a = files["a"]
    assert sum(os.path.getsize(tmp_path / "a" / (k + ".npy")) for k in arrays) <= limit
    assert a["keypoints0"].dtype == np.float32 and np.array_equal(a["keypoints0"], arrays["keypoints0"].numpy())
    assert a["matches0"].dtype == np.float64 and np.array_equal(a["matches0"], arrays["matches0"].numpy())
    assert a["counts0"].dtype == np.float64 and np.array_equal(a["counts0"], arrays["counts0"])
    d = a["descriptors0"]
    assert d.dtype == np.float32 and d.ndim == 1 and 0 < d.size < 100000 and metas[0]["descriptors0"] == {"shape": [100000], "sampled": d.size}
    assert np.isin(d, arrays["descriptors0"].astype(np.float32)).all()
    for k in arrays:                  # a second run writes the same files, sample positions included
        assert np.array_equal(files["b"][k], a[k]), k
    whole = bench.dump_outputs(arrays, str(tmp_path / "c"))          # the default budget (64 MB) holds these whole
    assert all(m["sampled"] is None for m in whole.values())


def test_package_and_library_versions_agree():
    import image_matching_amd
    from image_matching_amd import _lib
    major_minor = ".".join(image_matching_amd.__version__.split(".")[:2])
    assert f"imx {major_minor} ".encode() in _lib.load_library().imx_version()


def test_heavy_weight_sets_are_function_preserving():
    """Round 5: the "heavy" weight sets (synth.heavy_superpoint / heavy_superglue) rescale channels by powers of two and undo it in the
    next layer -- exact in fp32, so the reference gives bit-identical outputs on them (tests/golden/make_golden.py --heavy-check ran
    the reference's own modules on strict seeds of both sizes: tests/golden/heavy_check.npz records 48 bit-identical tensors) and every
    committed golden vector also pins the heavy sets.  Here the same statement for the oracle, on small shapes, without the reference."""
    from oracle import superglue_ref, superpoint_ref
    g = util.golden("heavy_check.npz")
    assert float(g["max_abs_diff"].max()) == 0.0 and int(g["tensors"]) == 48
    assert [list(map(int, r)) for r in g["heavy_sg_layers"]] == [[l, c, e] for l, (c, e) in synth.HEAVY_SG_LAYERS.items()]
    d, K = 128, 96
    x = util.pair(77, 72, 104)[0]
    outs = [superpoint_ref.superpoint_forward(x, to, util.sp_config(d, K), return_dense=True)
            for to in (util.to_torch(synth.make_superpoint_state_dict(d)), util.to_torch(synth.make_superpoint_state_dict(d, heavy=True)))]
    for k in ("semi", "desc"):
        assert torch.equal(outs[0][k], outs[1][k]), k
    assert torch.equal(outs[0]["keypoints"][0], outs[1]["keypoints"][0]) and torch.equal(outs[0]["descriptors"][0], outs[1]["descriptors"][0])
    o = outs[0]
    data = {"image0": x, "image1": x, "keypoints0": o["keypoints"][0][None], "keypoints1": o["keypoints"][0][None].flip(1),
            "scores0": o["scores"][0][None], "scores1": o["scores"][0][None].flip(1), "descriptors0": o["descriptors"][0][None],
            "descriptors1": o["descriptors"][0][None].flip(2)}
    sg = [superglue_ref.superglue_forward(data, util.to_torch(synth.make_superglue_state_dict(d, variant="t", heavy=hv)), util.sg_config(d), return_dense=True)
          for hv in (False, True)]
    for k in ("gnn0", "gnn1", "scores_in", "Z"):
        assert torch.equal(sg[0]["dense"][k], sg[1]["dense"][k]), k
    assert torch.equal(sg[0]["matches0"], sg[1]["matches0"])
    # ... while the weights an implementation folds ARE heavy-tailed: a BatchNorm scale 2^10 above its neighbours
    w = synth.make_superglue_state_dict(d, variant="t", heavy=True)["gnn.layers.3.mlp.1.weight"]
    assert abs(w[9]) > 200 * np.median(np.abs(w))


def test_every_handle_option_is_documented():
    """Every key imx_set_option accepts (the rows of kOptionTable in imx_options.cpp, the one place a key is spelled) and the read-only
    ones appear in include/imx.h's option documentation and in INTEGRATION.md -- a switch that changes which kernels run must not be
    findable only in the source (undocumented behaviour changes).  The key set itself is pinned: adding or dropping an
    option is a change of the interface."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "image-matching_amd", "csrc", "imx_options.cpp")).read()
    body = src[src.index("const OptionRow kOptionTable[] = {"):]
    body = body[:body.index("\n};\n")]
    keys = re.findall(r'^  \{"([a-z_0-9]+)", ', body, re.M)
    assert len(keys) == len(set(keys)), keys
    assert sorted(keys) == sorted(["mfma", "latency_forms", "gnn_tail", "attention", "conv", "attention_qblocks", "linear", "ha_masks",
                                   "conv_swizzle", "qkv_amax", "sinkhorn_group", "sinkhorn_merge", "keypoints", "sinkhorn_prefetch",
                                   "debug_poison"]), keys
    header = open(os.path.join(root, "include", "imx.h")).read()
    integ = open(os.path.join(root, "INTEGRATION.md")).read()
    for k in keys + ["arith_guard"]:
        assert f'"{k}"' in header, f"option '{k}' is not documented in include/imx.h"
        assert f"`{k}`" in integ, f"option '{k}' is not mentioned in INTEGRATION.md"
