"""SuperGlue training pairs (datasets/GlueSparse.py:24-104) around the engine: the corner sampler and its four-point matrix (host
plumbing with its own seeded random stream and float64 solve: unpinned, like the homography sampler of homoadapt.py), and the
conversion of the engine's padded device tensors into the reference's per-sample dict.  All image and keypoint arithmetic runs
in libimx (Engine.train_pairs / warp_perspective_u8 / gt_matches / match_loss)."""
import numpy as np
import torch

WARP_RANGE = 100          # GlueSparse.py:30: corner offsets drawn from [-100, 100)


def four_point_matrix(src, dst):
    """cv2.getPerspectiveTransform: the 3x3 matrix (m8 = 1) taking four points onto four points, solved in float64"""
    A, b = np.zeros((8, 8)), np.zeros(8)
    for k, ((x, y), (u, v)) in enumerate(zip(np.asarray(src, np.float64), np.asarray(dst, np.float64))):
        A[k] = [x, y, 1, 0, 0, 0, -x * u, -y * u]
        A[k + 4] = [0, 0, 0, x, y, 1, -x * v, -y * v]
        b[k], b[k + 4] = u, v
    return np.append(np.linalg.solve(A, b), 1.0).reshape(3, 3)


def sample_matrix(rng, shape_hw):
    """The random warp of GlueSparse.py:28-31: the four image corners, each moved by integer offsets, as a four-point matrix.  The
    reference unpacks `image.shape[:2]` into names that swap the axes (its `width` is the number of ROWS), so its corner list is
    (0, 0), (0, columns), (rows, 0), (rows, columns) read as (x, y) points; kept as it is, since it decides which warps are drawn."""
    rows, cols = shape_hw
    corners = np.float32([(0, 0), (0, cols), (rows, 0), (rows, cols)])
    moved = corners + rng.integers(-WARP_RANGE, WARP_RANGE, (4, 2)).astype(np.float32)
    return four_point_matrix(corners, moved)


def skip_sample(image, warped, file_name):
    """the dict of a pair with a side without keypoints (GlueSparse.py:52-61)"""
    return {'keypoints0': torch.zeros([0, 0, 2], dtype=torch.double), 'keypoints1': torch.zeros([0, 0, 2], dtype=torch.double),
            'descriptors0': torch.zeros([0, 2], dtype=torch.double), 'descriptors1': torch.zeros([0, 2], dtype=torch.double),
            'image0': image, 'image1': warped, 'file_name': file_name}


def reference_sample(host, b, image, warped, file_name, device):
    """One sample of GlueSparse.__getitem__ (:84-104) from `host`, the engine's tensors copied to numpy: same keys, containers, dtypes."""
    n0, n1 = int(host['counts0'][b]), int(host['counts1'][b])
    if n0 < 1 or n1 < 1:
        return skip_sample(image, warped, file_name)
    n, n_all = int(host['n_matches'][b]), int(host['n_all'][b])
    am = host['all_matches'][b][:, :n_all]
    return {
        'keypoints0': [host['keypoints0'][b, :n0].copy()], 'keypoints1': [host['keypoints1'][b, :n1].copy()],
        'descriptors0': list(np.ascontiguousarray(host['descriptors0'][b, :n0].T)), 'descriptors1': list(np.ascontiguousarray(host['descriptors1'][b, :n1].T)),
        'scores0': list(host['scores0'][b, :n0]), 'scores1': list(host['scores1'][b, :n1]),
        'image0': torch.from_numpy(image / 255.).double()[None].to(device), 'image1': torch.from_numpy(warped / 255.).double()[None].to(device),
        'matches': am[:, :n].copy(), 'all_matches': list(am.copy()), 'file_name': file_name,
    }


def to_host(out):
    """the device tensors of Engine.train_pairs in ONE synchronisation, as numpy"""
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}
