"""The code paths of SuperPoint's training-data kernels that only a workload-size call takes (480x640, a batch of 8 to 32), each at the
smallest shape that crosses its threshold: the second and third row segment of shade_rows_kernel, the second and third chunk of 64 images
of imx_photo_shade, the second trip of the fill loops of imx_warp_labels and imx_warp_labels_bi, the second workgroup of
wl_points_kernel, the strided loop of det_loss_finish_kernel (whose sum det_grad_kernel divides by), and one batch of the dataset at the
shipped size.  Every bound is one the project already derives: the shade bound (2 (ksize + 2) + 8) 2^-24 of tests/test_gpu_photometric.py,
bit equality for both label kernels, 1 ulp of the coordinate for residuals, check_det's rule and the default bar of
tests/test_gpu_spgrad.py.  The thresholds stated here are pinned to the sources by tests/test_sp_workload_paths_host.py, which also checks
on the restatements alone what these tests take for granted about their cases.  Needs an MI355X.
Wall time on an MI355X: 11 s alone (no test above 1.4 s); the whole GPU suite with it 587 s and 602 s in two runs, of a limit of 1200 s:
half of it.  The parent commit's suite was not timed again on that machine: the same runs less this file are about 576 s and 591 s, so
the spread between two runs is larger than the file.
Against libraries built with one of these paths cut short -- either fill loop or the finishing sum left after its first trip, the row
pass's halo taken from x0 = 0, ksize read without b0, one workgroup of points -- the tests that cross that path fail, the others pass."""
import numpy as np
import pytest
import torch

from tests import photometric_ref as P
from tests import spgrad_ref as G
from tests import sploop_ref as S
from tests import sptrain_ref as R
from tests import util
from tests.test_gpu_history import POISONS
from tests.test_gpu_photometric import SHIPPED_PHOTO, allss_sets, pick, shade
from tests.test_gpu_sppool import Banded
from tests.test_gpu_sptrain import check_det, check_labels, cuda

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------- the thresholds and the shapes that cross them
ROW_OUT = 256                         # kRowOut (csrc/photo_aug.h): outputs of a row segment of shade_rows_kernel
WIDE_SHADE_CASES = ((3, 6, 257), (101, 6, 300), (351, 5, 513), (151, 9, 640))     # (ksize, H, W): two or three segments
SHADE_CHUNK = 64                      # kShadeChunk (csrc/photo_aug.h): images per launch of a blur pass
CHUNK_B, CHUNK_H, CHUNK_W = 130, 24, 40                                           # three chunks, the last of two images
CHUNK_EDGES = (63, 64, 65, 127, 128, 129)
CHUNK_OFF, CHUNK_EMPTY, CHUNK_SPLIT = 64, 65, 50
WL_FILL_BLOCKS = 2048                 # the cap of wl_fill_kernel's grid (csrc/sptrain.hip), 256 threads each
POINTS_PER_BLOCK = 256                # points per workgroup of wl_points_kernel
WL_B, WL_H, WL_W, WL_COUNTS = 2, 600, 600, (300, 257)                             # 720 000 elements; Kcap = 303
WL_TAIL_ROW = 274                     # the second trip of the fill loop: image 1 from this row down
LB_FILL_BLOCKS = 4096                 # the cap of lb_fill_kernel's grid (csrc/sploop.hip), 256 threads each
LB_B, LB_H, LB_W, LB_COUNTS = 2, 800, 800, (300, 300)                             # 1 280 000 elements
LB_TAIL_ROW = 511
DET_FINISH_THREADS = 256              # det_loss_finish_kernel: one partial pair per 256 cells, summed by 256 threads
DET_SHAPES = ((16, 512, 512), (1, 2048, 2056))                                    # exactly 256 partials; 257
DET_TAIL_CELLS = 1000                 # the targeted mask: the last 1000 cells
DATASET_H, DATASET_W = 480, 640       # the shipped size: three row segments


def new_engine():
    from image_matching_amd.engine import Engine
    return Engine(util.sp_config(128, 256), util.sg_config(128), "cuda")


@pytest.fixture(scope="module")
def eng():
    return new_engine()


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------- A. the row pass beyond its first segment
@pytest.mark.parametrize("case", WIDE_SHADE_CASES, ids=lambda c: f"k{c[0]}-{c[1]}x{c[2]}")
def test_shade_rows_beyond_the_first_segment(eng, case):
    ksize, H, W = case
    assert W > ROW_OUT and -(-W // ROW_OUT) in (2, 3)
    c = P.shade_case_wide(*case, first_column=ROW_OUT)
    got = shade(eng, c)
    assert got.dtype == np.float32 and got.shape == (4, H, W)
    ref = np.stack([P.shade_one(c, b) for b in range(4)])
    bound = (2 * (ksize + 2) + 8) * 2.0 ** -24
    err = np.abs(got.astype(np.float64) - ref)
    print(f"{case}: largest error / bound per image {err.reshape(4, -1).max(1) / bound}; in the columns >= {ROW_OUT}: "
          f"{err[:, :, ROW_OUT:].reshape(4, -1).max(1) / bound}")
    assert (err <= bound).all()
    plain = c['img'].astype(np.float32) / np.float32(255)
    assert np.array_equal(got[1], plain[1]) and np.array_equal(got[3], plain[3])        # 0 ellipses; on/off word clear
    for b in (0, 2):                                                                    # the bound is not met by an untouched region
        assert (got[b, :, ROW_OUT:] != plain[b, :, ROW_OUT:]).any(), b


# ---------------------------------------------------------------------------------------------- B. more than 64 images per shade call
def test_shade_beyond_the_first_chunk_of_images(eng):
    B, H, W = CHUNK_B, CHUNK_H, CHUNK_W
    assert B > 2 * SHADE_CHUNK and CHUNK_SPLIT % SHADE_CHUNK != 0
    assert set(CHUNK_EDGES) == {SHADE_CHUNK * n + d for n in (1, 2) for d in (-1, 0, 1)} and max(CHUNK_EDGES) == B - 1
    c = P.shade_batch_case(B, H, W, off=(CHUNK_OFF,), empty=(CHUNK_EMPTY,))
    ks = c['ksize']
    for n in (1, 2):                                                    # pairwise different round each chunk boundary
        assert {int(ks[SHADE_CHUNK * n + d]) for d in (-1, 0, 1)} == set(P.SHADE_BATCH_KSIZES)
    assert ks[64] != ks[0] and ks[128] not in (ks[0], ks[64])           # nor that of the same place in an earlier chunk
    assert c['on'][CHUNK_OFF] == 0 and c['n_ellipses'][CHUNK_EMPTY] == 0
    whole = shade(eng, c)
    for b in CHUNK_EDGES:
        assert np.array_equal(bits(shade(eng, pick(c, [b]))[0]), bits(whole[b])), f"image {b} alone"
    halves = np.concatenate([shade(eng, pick(c, range(CHUNK_SPLIT))), shade(eng, pick(c, range(CHUNK_SPLIT, B)))])
    differ = sorted({int(b) for b in np.nonzero((bits(halves) != bits(whole)).reshape(B, -1).any(1))[0]})
    assert not differ, f"images {differ} differ between one call and two calls split at image {CHUNK_SPLIT}"
    plain = c['img'].astype(np.float32) / np.float32(255)
    assert np.array_equal(whole[CHUNK_OFF], plain[CHUNK_OFF]) and np.array_equal(whole[CHUNK_EMPTY], plain[CHUNK_EMPTY])
    for b in (0, 64, 129):
        bound = (2 * (int(ks[b]) + 2) + 8) * 2.0 ** -24
        err = np.abs(whole[b].astype(np.float64) - P.shade_one(c, b)).max()
        print(f"image {b} (ksize {ks[b]}): largest error / bound {err / bound}")
        assert err <= bound
        assert b == CHUNK_OFF or (whole[b] != plain[b]).any()


# ---------------------------------------------------------------------------------------------- C. imx_warp_labels
@pytest.fixture(scope="module")
def wl_cases():
    """(the case, a second one of the same shape whose points land nowhere near the first's)"""
    pts, mats = R.workload_points(WL_H, WL_W, WL_COUNTS, WL_TAIL_ROW, seed=1)
    taken = np.stack([R.warp_labels(p, m, WL_H, WL_W)[0] for p, m in zip(pts, mats)]) > 0
    return (pts, mats), R.workload_points(WL_H, WL_W, WL_COUNTS, WL_TAIL_ROW, seed=2, avoid=taken)


def padded(pts_rows):
    """check_labels's layout: (B, longest + 3, 2), rows past the counts NaN; the counts"""
    pts = np.full((len(pts_rows), max(len(p) for p in pts_rows) + 3, 2), np.nan, np.float32)
    for b, p in enumerate(pts_rows):
        pts[b, :len(p)] = p
    return cuda(pts), torch.tensor([len(p) for p in pts_rows], dtype=torch.int32).cuda()


def test_warp_labels_beyond_the_fill_grid_and_256_points(eng, wl_cases):
    from image_matching_amd.engine import _ptr, _stream
    (pts_rows, mats), (other_rows, other_mats) = wl_cases
    B, H, W = WL_B, WL_H, WL_W
    assert B * H * W > WL_FILL_BLOCKS * 256 and (WL_FILL_BLOCKS * 256 - H * W) // W == WL_TAIL_ROW - 1
    assert tuple(len(p) for p in pts_rows) == WL_COUNTS and min(WL_COUNTS) > POINTS_PER_BLOCK
    # 1. the module's engine, right after a call of the same shape that left its own labels, owners and residuals behind
    check_labels(eng, other_rows, list(other_mats), H, W, "the other point set")
    first = check_labels(eng, pts_rows, list(mats), H, W, "after another point set")
    assert first[0][1, WL_TAIL_ROW:].sum() >= 100
    # 2. fresh engines whose workspaces are allocated under every poison pattern
    for p in POISONS:
        fresh = new_engine()
        fresh.set_option("debug_poison", p)
        assert same(check_labels(fresh, pts_rows, list(mats), H, W, f"fresh engine, debug_poison = {p}"), first), p
    # 3. the C ABI, labels and res between guard bands and pre-filled with the sentinel
    pts, counts = padded(pts_rows)
    assert pts.shape[1] == 303
    lab, res, flag = Banded((B, H, W)), Banded((B, 2, H, W)), torch.full((1,), 77, dtype=torch.int32, device="cuda")
    assert bool((lab.t == lab.sentinel).all()) and bool((res.t == res.sentinel).all())
    m = cuda(mats)
    rc = eng.train.imx_warp_labels(eng.handle, _ptr(pts), _ptr(counts), B, int(pts.shape[1]), _ptr(m), H, W, _ptr(lab.t), _ptr(res.t), _ptr(flag),
                                   _stream(eng.device))
    assert rc == 0, eng.lib.imx_last_error(eng.handle)
    torch.cuda.synchronize()
    assert lab.untouched() and res.untouched() and int(flag) == 0
    assert same((lab.t, res.t), first), "sentinel-filled outputs through the C ABI"
    # points_to_2D at the same shape and counts
    l2, _, flag = eng.warp_labels(pts, counts, None, H, W)
    want = [R.points_to_2d(p, H, W) for p in pts_rows]
    assert int(flag) == 0 == max(f for _, f in want)
    assert np.array_equal(l2.cpu().numpy(), np.stack([w for w, _ in want])) and l2[1, WL_TAIL_ROW:].sum() >= 100


# ---------------------------------------------------------------------------------------------- D. imx_warp_labels_bi
@pytest.fixture(scope="module")
def lb_cases():
    """(pts_rows, mats, {levels: the restatement's maps}) and a second point set that lands nowhere near the first's"""
    pts, mats = R.workload_points(LB_H, LB_W, LB_COUNTS, LB_TAIL_ROW, seed=3)
    refs = {}
    for levels in (0, 255):
        out = [S.labels_bi(p, m, LB_H, LB_W, levels) for p, m in zip(pts, mats)]
        assert not any(f for _, f in out)
        refs[levels] = np.stack([o for o, _ in out])
    return (pts, mats, refs), R.workload_points(LB_H, LB_W, LB_COUNTS, LB_TAIL_ROW, seed=4, avoid=refs[0] > 0)


@pytest.mark.parametrize("levels", (0, 255))
def test_warp_labels_bi_beyond_the_fill_grid(eng, lb_cases, levels):
    from image_matching_amd.engine import _ptr, _stream
    (pts_rows, mats, refs), (other_rows, other_mats) = lb_cases
    B, H, W = LB_B, LB_H, LB_W
    assert B * H * W > LB_FILL_BLOCKS * 256 and (LB_FILL_BLOCKS * 256 - H * W) // W == LB_TAIL_ROW - 1
    pts, counts = padded(pts_rows)
    want = refs[levels]
    assert np.count_nonzero(want[1, LB_TAIL_ROW:]) >= 100

    def held(out, flag, tag):
        assert int(flag) == 0, tag
        bad = np.nonzero(bits(out) != bits(want))
        assert not len(bad[0]), f"{tag}: {len(bad[0])} pixels differ, the first at (image, row, column) {tuple(int(v[0]) for v in bad)}"
    # 1. right after a call of the same shape with another point set
    other, _ = padded(other_rows)
    eng.warp_labels_bi(other, counts, other_mats, H, W, levels=levels, pixel_space=True)
    held(*eng.warp_labels_bi(pts, counts, mats, H, W, levels=levels, pixel_space=True), "after another point set")
    # 2. fresh engines whose workspaces are allocated under every poison pattern
    for p in POISONS:
        fresh = new_engine()
        fresh.set_option("debug_poison", p)
        held(*fresh.warp_labels_bi(pts, counts, mats, H, W, levels=levels, pixel_space=True), f"fresh engine, debug_poison = {p}")
    # 3. the C ABI, the output between guard bands and pre-filled with the sentinel
    out, flag, m = Banded((B, H, W)), torch.full((1,), 77, dtype=torch.int32, device="cuda"), cuda(mats)
    assert bool((out.t == out.sentinel).all())
    rc = eng.sploop.imx_warp_labels_bi(eng.handle, _ptr(pts), _ptr(counts), B, int(pts.shape[1]), _ptr(m), H, W, levels, _ptr(out.t), _ptr(flag),
                                       _stream(eng.device))
    assert rc == 0, eng.lib.imx_last_error(eng.handle)
    torch.cuda.synchronize()
    assert out.untouched()
    held(out.t, flag, "sentinel-filled output through the C ABI")


# ---------------------------------------------------------------------------------------------- E. detector loss beyond 256 partials
@pytest.fixture(scope="module")
def det_cases():
    """shape -> (semi, labels, the targeted mask)"""
    return {s: R.det_case(*s, seed=7) + (R.last_cells_mask(*s, DET_TAIL_CELLS),) for s in DET_SHAPES}


@pytest.mark.parametrize("shape", DET_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_detector_loss_beyond_256_partials(eng, det_cases, shape):
    B, H, W = shape
    cells = B * (H // 8) * (W // 8)
    partials = -(-cells // 256)
    assert partials == (DET_FINISH_THREADS if B > 1 else DET_FINISH_THREADS + 1) and cells >= 65536
    semi, labels, tail = det_cases[shape]
    check_det(eng, semi, labels, np.ones(shape, np.float32), f"{shape}, full mask")
    got = check_det(eng, semi, labels, tail, f"{shape}, the last {DET_TAIL_CELLS} cells")
    assert got[1] == DET_TAIL_CELLS and got[0] > 0.1
    if B > 1:                                                            # those cells' images alone: the same bits
        per = cells // B
        first = (cells - DET_TAIL_CELLS) // per
        assert per % 256 == 0 and first == B - 1
        alone = eng.detector_loss(cuda(semi[first:]), cuda(labels[first:]), cuda(tail[first:])).cpu().numpy()
        assert np.array_equal(bits(alone), bits(got.astype(np.float32))), (alone, got)


def test_detector_grad_beyond_256_partials(eng, det_cases):
    shape = DET_SHAPES[1]
    assert shape[0] * (shape[1] // 8) * (shape[2] // 8) > DET_FINISH_THREADS * 256
    semi, labels, tail = det_cases[shape]
    out, grad = eng.detector_loss_grad(cuda(semi), cuda(labels), cuda(tail))
    assert same([out], [eng.detector_loss(cuda(semi), cuda(labels), cuda(tail))]), "the value is imx_detector_loss's, bit for bit"
    loss64, g64 = G.detector_grad(semi, labels, tail)
    got = grad.cpu().numpy()
    frac = float(np.max(np.abs(got.astype(np.float64) - g64) / G.bar(g64)))
    print(f"{shape}: loss {float(out[0]):.8f} (float64 {loss64:.8f}); gradient at most {frac:.3g} of the bar from the float64 autograd, "
          f"largest |g64| {np.abs(g64).max():.3e}")
    assert frac <= 1.0
    cell_mask = R.cell_masks(tail).numpy()[:, None]
    assert cell_mask.sum() == DET_TAIL_CELLS and not got[np.broadcast_to(cell_mask == 0, got.shape)].any(), "exactly 0 where the mask is 0"
    assert np.abs(got[np.broadcast_to(cell_mask == 1, got.shape)]).max() > 1e-4, "and not there alone"


# ---------------------------------------------------------------------------------------------- F. one batch at the shipped size
def test_allss_photometric_batch_at_the_shipped_size():
    H, W = DATASET_H, DATASET_W
    assert -(-W // ROW_OUT) == 3
    plain, aug = allss_sets(H, W, SHIPPED_PHOTO)
    a, b, again = plain.batch(range(3)), aug.batch(range(3)), aug.batch(range(3))
    assert set(a) == set(b) == set(again)
    for k in a:
        if k in ('image', 'warped_img'):
            assert b[k].shape == a[k].shape and tuple(b[k].shape[-2:]) == (H, W) and b[k].dtype == torch.float32
            assert not torch.equal(a[k], b[k]) and float(b[k].min()) >= 0.0 and float(b[k].max()) <= 1.0
            assert (a[k][..., ROW_OUT:] != b[k][..., ROW_OUT:]).any() and (a[k][..., 2 * ROW_OUT:] != b[k][..., 2 * ROW_OUT:]).any()
            assert np.array_equal(bits(again[k]), bits(b[k])), f"{k}: the same batch twice"
        elif isinstance(a[k], torch.Tensor):
            assert torch.equal(a[k], b[k]), k                            # labels, masks, homographies: bit for bit
        else:
            assert a[k] == b[k], k
    one = aug.batch([1])
    for k in ('image', 'warped_img'):
        assert np.array_equal(bits(one[k][0]), bits(b[k][1])), f"{k}: sample 1 alone"
