"""Host-side engine: one libimx handle per (device, config), weight upload, and tensor-level
wrappers of the C-ABI entry points.  torch tensors are containers only (data_ptr + stream)."""
import ctypes
import math

import numpy as np
import torch

from . import _lib as L

SP_DEFAULT = {                      # superpoint/models/superpoint_test.py:57-63
    "descriptor_dim": 256, "nms_radius": 4, "keypoint_threshold": 0.005,
    "max_keypoints": -1, "remove_borders": 4,
}
SG_DEFAULT = {                      # superglue/models/superglue_test.py:195-202
    "descriptor_dim": 256, "weights": "indoor", "keypoint_encoder": [32, 64, 128, 256],
    "GNN_layers": ["self", "cross"] * 9, "sinkhorn_iterations": 100, "match_threshold": 0.2,
}


def reference_align_corners():
    """What `int(torch.__version__[2]) > 2` (superpoint_test.py:47) evaluates to under the torch
    in this process: True for torch 1.3-1.9, False for 1.10+/2.x (third character '1'/'0')."""
    try:
        return int(torch.__version__[2]) > 2
    except ValueError:
        return False


class ImxError(RuntimeError):
    pass


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class Engine:
    """Owns an imx handle.  `sp_cfg` / `sg_cfg` are the merged reference-style config dicts."""

    def __init__(self, sp_cfg, sg_cfg, device, sp_variant=L.SP_VARIANT_BN, align_corners=None):
        self.lib = L.load_library()
        self.train = L.load_train_library()        # the training stages (include/imx_train.h), on the same handle
        self.sgtrain = L.load_sgtrain_library()    # the score product of SuperGlue's training step (include/imx_sgtrain.h), likewise
        self.spnet = L.load_spnet_library()        # the 3x3 convolutions of SuperPoint's training step (include/imx_spnet.h), likewise
        self.spnorm = L.load_spnorm_library()      # BatchNorm2d [+ ReLU] of SuperPoint's training step (include/imx_spnorm.h), likewise
        self.sppool = L.load_sppool_library()      # MaxPool2d(2) and the descriptor normalisation of that step (include/imx_sppool.h), likewise
        self.photo = L.load_photo_library()        # the photometric augmentation of that step's data (include/imx_photo.h), likewise
        self.sploop = L.load_sploop_library()      # the soft labels and the optimiser step of the training loop (include/imx_sploop.h), likewise
        self.sgloop = L.load_sgloop_library()      # the matches of SuperGlue's training forward from the loss's Sinkhorn (include/imx_sgloop.h), likewise
        self.homog = L.load_homog_library()        # the RANSAC homography fit and the corner error (include/imx_homog.h), likewise
        self.speval = L.load_speval_library()      # the mutual nearest-neighbour matcher and the pair metrics (include/imx_speval.h), likewise
        if not torch.cuda.is_available():
            raise ImxError("image_matching_amd needs a ROCm GPU (torch.cuda.is_available() is False); "
                           "there is no CPU fallback on the product path")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ImxError(f"image_matching_amd runs on 'cuda' (HIP) devices only, got {device!r}")
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", idx)
        sp = {**SP_DEFAULT, **(sp_cfg or {})}
        sg = {**SG_DEFAULT, **(sg_cfg or {})}
        cfg = L.ImxConfig()
        cfg.descriptor_dim = int(sp["descriptor_dim"])
        cfg.nms_radius = int(sp["nms_radius"])
        cfg.keypoint_threshold = float(sp["keypoint_threshold"])
        cfg.max_keypoints = int(sp["max_keypoints"])
        cfg.remove_borders = int(sp["remove_borders"])
        cfg.align_corners = int(reference_align_corners() if align_corners is None else bool(align_corners))
        cfg.sp_variant = int(sp_variant)
        layers = list(sg["GNN_layers"])
        if len(layers) > L.IMX_MAX_GNN_LAYERS:
            raise ImxError(f"at most {L.IMX_MAX_GNN_LAYERS} GNN layers supported")
        cfg.num_gnn_layers = len(layers)
        for i, name in enumerate(layers):
            cfg.gnn_layer_is_cross[i] = 1 if name == "cross" else 0
        kenc = [int(c) for c in sg["keypoint_encoder"]]
        if not 1 <= len(kenc) <= L.IMX_MAX_KENC:
            raise ImxError(f"keypoint_encoder needs 1 to {L.IMX_MAX_KENC} entries, got {len(kenc)}")
        cfg.kenc_n = len(kenc)
        for i, c in enumerate(kenc):
            cfg.kenc_channels[i] = c
        cfg.sinkhorn_iterations = int(sg["sinkhorn_iterations"])
        cfg.match_threshold = float(sg["match_threshold"])
        self.cfg = cfg
        self.d = cfg.descriptor_dim
        self.max_keypoints = cfg.max_keypoints
        self.handle = ctypes.c_void_p()
        if self.lib.imx_create(idx, ctypes.byref(cfg), ctypes.byref(self.handle)) != 0:
            raise ImxError(self.lib.imx_last_error(None).decode())
        self.loaded = {L.NET_SUPERPOINT: False, L.NET_SUPERGLUE: False}

    def __del__(self):
        try:
            if getattr(self, "handle", None) and self.handle.value:
                self.lib.imx_destroy(self.handle)
                self.handle = ctypes.c_void_p()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise ImxError(self.lib.imx_last_error(self.handle).decode())

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, net, state_dict):
        for key, val in state_dict.items():
            if key.endswith("num_batches_tracked"):
                continue
            arr = val.detach().cpu().numpy() if isinstance(val, torch.Tensor) else np.asarray(val)
            arr = np.ascontiguousarray(arr, dtype=np.float32)
            shape = (ctypes.c_int64 * max(arr.ndim, 1))(*arr.shape)
            self._check(self.lib.imx_load_weight(self.handle, net, key.encode(), arr.ctypes.data_as(ctypes.c_void_p),
                                                 arr.ndim, shape))
        self._check(self.lib.imx_finalize_weights(self.handle, net))
        self.loaded[net] = True

    # ------------------------------------------------------------------ SuperPoint
    def superpoint(self, x):
        """x (B,1,H,W) float32 cuda -> (kpts (B,K,2), scores (B,K), desc (B,K,d), counts list)."""
        x = self._image(x)
        B, _, H, W = x.shape
        counts = torch.empty(B, dtype=torch.int32, device=self.device)
        st = _stream(self.device)
        self._check(self.lib.imx_superpoint_detect(self.handle, _ptr(x), B, H, W, _ptr(counts), st))
        n = counts.cpu().tolist()                       # device sync (the reference syncs at nonzero())
        K = max(n) if n else 0
        kpts = torch.empty(B, K, 2, dtype=torch.float32, device=self.device)
        scores = torch.empty(B, K, dtype=torch.float32, device=self.device)
        desc = torch.empty(B, K, self.d, dtype=torch.float32, device=self.device)
        if K > 0:
            self._check(self.lib.imx_superpoint_describe(self.handle, B, K, _ptr(kpts), _ptr(scores), _ptr(desc), st))
        return kpts, scores, desc, n

    def superpoint_dense(self, x):
        """Dense forward (superpoint_train.py:31-57): semi (B,65,H/8,W/8), desc (B,d,H/8,W/8) unit-norm."""
        x = self._image(x)
        B, _, H, W = x.shape
        Hc, Wc = H // 2 // 2 // 2, W // 2 // 2 // 2
        semi = torch.empty(B, 65, Hc, Wc, dtype=torch.float32, device=self.device)
        desc = torch.empty(B, self.d, Hc, Wc, dtype=torch.float32, device=self.device)
        self._check(self.lib.imx_superpoint_dense(self.handle, _ptr(x), B, H, W, _ptr(semi), _ptr(desc), _stream(self.device)))
        return semi, desc

    def superpoint_batch(self, x):
        """Throughput path: SuperPoint with fixed max_keypoints = K > 0, no host sync.  Returns padded
        (kpts (B,K,2), scores (B,K), desc (B,K,d), counts (B) int32); rows >= count are zero."""
        x = self._image(x)
        B, _, H, W = x.shape
        K = self.max_keypoints
        if K <= 0:
            raise ImxError("superpoint_batch needs max_keypoints > 0")
        counts = torch.empty(B, dtype=torch.int32, device=self.device)
        kpts = torch.empty(B, K, 2, dtype=torch.float32, device=self.device)
        scores = torch.empty(B, K, dtype=torch.float32, device=self.device)
        desc = torch.empty(B, K, self.d, dtype=torch.float32, device=self.device)
        st = _stream(self.device)
        self._check(self.lib.imx_superpoint_detect(self.handle, _ptr(x), B, H, W, _ptr(counts), st))
        self._check(self.lib.imx_superpoint_describe(self.handle, B, K, _ptr(kpts), _ptr(scores), _ptr(desc), st))
        return kpts, scores, desc, counts

    def _image(self, x):
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != 1:
            raise ImxError(f"expected an image tensor of shape (B,1,H,W), got {getattr(x, 'shape', type(x))}")
        if x.device.type != "cuda":
            raise ImxError("image tensor must live on the GPU (the reference CLI moves it with .to(device)); "
                           "there is no CPU path")
        return x.to(device=self.device, dtype=torch.float32).contiguous()

    # ------------------------------------------------------------------ SuperGlue
    def superglue(self, kpts0, scores0, desc0, shape0, kpts1, scores1, desc1, shape1, n0=None, n1=None):
        """desc{0,1}: (B,d,N) tensors with arbitrary strides.  Returns matches0/1 (int64), mscores0/1."""
        dev = self.device
        kpts0 = kpts0.to(dev, torch.float32).contiguous()
        kpts1 = kpts1.to(dev, torch.float32).contiguous()
        scores0 = scores0.to(dev, torch.float32).contiguous()
        scores1 = scores1.to(dev, torch.float32).contiguous()
        desc0 = desc0.to(dev, torch.float32)
        desc1 = desc1.to(dev, torch.float32)
        B, N0 = kpts0.shape[0], kpts0.shape[1]
        N1 = kpts1.shape[1]
        if desc0.shape[1] != self.d or desc1.shape[1] != self.d:
            raise ImxError(f"descriptor dim {desc0.shape[1]} != configured descriptor_dim {self.d}")
        m0 = torch.empty(B, N0, dtype=torch.int64, device=dev)
        m1 = torch.empty(B, N1, dtype=torch.int64, device=dev)
        ms0 = torch.empty(B, N0, dtype=torch.float32, device=dev)
        ms1 = torch.empty(B, N1, dtype=torch.float32, device=dev)
        s0, s1 = desc0.stride(), desc1.stride()
        self._check(self.lib.imx_superglue_forward(
            self.handle, B,
            _ptr(kpts0), _ptr(scores0), _ptr(desc0), s0[0], s0[1], s0[2], _ptr(n0), N0, int(shape0[-2]), int(shape0[-1]),
            _ptr(kpts1), _ptr(scores1), _ptr(desc1), s1[0], s1[1], s1[2], _ptr(n1), N1, int(shape1[-2]), int(shape1[-1]),
            _ptr(m0), _ptr(m1), _ptr(ms0), _ptr(ms1), _stream(dev)))
        return m0, m1, ms0, ms1

    # ------------------------------------------------------------------ fused pairs
    def match_pairs(self, img0, img1, want_desc=False):
        """Fused Matching.forward for B pairs (max_keypoints = K > 0); no host sync.
        Returns dict of padded tensors: keypoints{0,1} (B,K,2), scores{0,1} (B,K), counts{0,1} (B),
        matches{0,1} (B,K) int64, matching_scores{0,1} (B,K) [, descriptors{0,1} (B,K,d)]."""
        img0, img1 = self._image(img0), self._image(img1)
        if img0.shape != img1.shape:
            raise ImxError("match_pairs needs equal image shapes on both sides")
        B, _, H, W = img0.shape
        K, dev = self.max_keypoints, self.device
        if K <= 0:
            raise ImxError("match_pairs needs max_keypoints > 0")
        f32, out = torch.float32, {}
        for s in "01":
            out["keypoints" + s] = torch.empty(B, K, 2, dtype=f32, device=dev)
            out["scores" + s] = torch.empty(B, K, dtype=f32, device=dev)
            out["counts" + s] = torch.empty(B, dtype=torch.int32, device=dev)
            out["matches" + s] = torch.empty(B, K, dtype=torch.int64, device=dev)
            out["matching_scores" + s] = torch.empty(B, K, dtype=f32, device=dev)
            if want_desc:
                out["descriptors" + s] = torch.empty(B, K, self.d, dtype=f32, device=dev)
        self._check(self.lib.imx_match_pairs(
            self.handle, _ptr(img0), _ptr(img1), B, H, W,
            _ptr(out["keypoints0"]), _ptr(out["keypoints1"]), _ptr(out["scores0"]), _ptr(out["scores1"]),
            _ptr(out["counts0"]), _ptr(out["counts1"]),
            _ptr(out.get("descriptors0")), _ptr(out.get("descriptors1")),
            _ptr(out["matches0"]), _ptr(out["matches1"]),
            _ptr(out["matching_scores0"]), _ptr(out["matching_scores1"]), _stream(dev)))
        return out

    def pack_records(self, pair_ids, out, pad_to=None):
        """The match records of shard.py (one row of 3 + 8K 32-bit words per pair) from match_pairs' output dict, packed by one
        kernel (imx_pack_records) on the current stream.  pair_ids: (B) int32 tensor on the device (or a list: copied once per
        call -- callers with a fixed shard keep the tensor).  Rows past B up to pad_to are padding (pair id -1)."""
        B, K = out["matches0"].shape
        rows = max(B, pad_to or 0)
        if not isinstance(pair_ids, torch.Tensor):
            pair_ids = torch.as_tensor(list(pair_ids), dtype=torch.int32)
        pair_ids = pair_ids.to(self.device, torch.int32).contiguous()
        # the kernel reads pair_ids[row] for every row < B and reinterprets raw pointers: refuse anything that is not what
        # match_pairs returns instead of reading out of bounds or through the wrong dtype
        if pair_ids.numel() != B:
            raise ImxError(f"pack_records: {pair_ids.numel()} pair ids for a batch of {B} pairs")
        want = {"keypoints0": (torch.float32, (B, K, 2)), "keypoints1": (torch.float32, (B, K, 2)), "counts0": (torch.int32, (B,)), "counts1": (torch.int32, (B,)),
                "matches0": (torch.int64, (B, K)), "matches1": (torch.int64, (B, K)), "matching_scores0": (torch.float32, (B, K)), "matching_scores1": (torch.float32, (B, K))}
        for key, (dt, shp) in want.items():
            t = out[key]
            if not (isinstance(t, torch.Tensor) and t.dtype == dt and tuple(t.shape) == shp and t.device == self.device and t.is_contiguous()):
                raise ImxError(f"pack_records: out[{key!r}] must be a contiguous {dt} tensor of shape {shp} on {self.device} "
                               f"(got {getattr(t, 'dtype', type(t))}, {tuple(getattr(t, 'shape', ()))}, {getattr(t, 'device', None)})")
        rec = torch.empty(rows, 3 + 8 * K, dtype=torch.int32, device=self.device)
        self._check(self.lib.imx_pack_records(
            self.handle, _ptr(pair_ids), B, K, _ptr(out["keypoints0"]), _ptr(out["keypoints1"]), _ptr(out["counts0"]), _ptr(out["counts1"]),
            _ptr(out["matches0"]), _ptr(out["matches1"]), _ptr(out["matching_scores0"]), _ptr(out["matching_scores1"]),
            _ptr(rec), rows, _stream(self.device)))
        return rec

    def estimate_affine_partial(self, kpts0, kpts1, matches0, counts0=None, ransac_thresh=7.0, hypotheses=512, seed=0):
        """Batched RANSAC partial-affine fit (superpoint_glue_test.py:86-92) on the GPU.
        kpts{0,1} (B,K,2), matches0 (B,K) int64.  Returns M (B,2,3), inlier mask (B,K) uint8, n_inliers (B) int32."""
        dev = self.device
        kpts0 = kpts0.to(dev, torch.float32).contiguous()
        kpts1 = kpts1.to(dev, torch.float32).contiguous()
        matches0 = matches0.to(dev, torch.int64).contiguous()
        B, K0 = matches0.shape
        K = max(K0, kpts1.shape[1])
        if K0 < K:                        # pad side 0 (unmatched) so both sides share K; indices stay valid
            kpts0 = torch.cat([kpts0, kpts0.new_zeros(B, K - K0, 2)], 1)
            matches0 = torch.cat([matches0, matches0.new_full((B, K - K0), -1)], 1)
        if kpts1.shape[1] < K:
            kpts1 = torch.cat([kpts1, kpts1.new_zeros(B, K - kpts1.shape[1], 2)], 1)
        M = torch.empty(B, 2, 3, dtype=torch.float32, device=dev)
        inl = torch.empty(B, K, dtype=torch.uint8, device=dev)
        ninl = torch.empty(B, dtype=torch.int32, device=dev)
        self._check(self.lib.imx_estimate_affine_partial(self.handle, _ptr(kpts0), _ptr(kpts1), _ptr(matches0), _ptr(counts0),
                                                         B, K, float(ransac_thresh), int(hypotheses), int(seed) & 0xFFFFFFFF,
                                                         _ptr(M), _ptr(inl), _ptr(ninl), _stream(dev)))
        return M, inl[:, :K0], ninl

    def estimate_homography(self, kpts0, kpts1, matches0, counts0=None, ransac_thresh=3.0, hypotheses=512, refine_iters=3, seed=0):
        """Batched RANSAC homography fit on the GPU, the cv2.findHomography(mkpts0, mkpts1, cv2.RANSAC, thr) counterpart of
        estimate_affine_partial (include/imx_homog.h): kpts0 (B,K0,2), kpts1 (B,K1,2) fp32, matches0 (B,K0) int64, counts0 (B) int32 or
        None = K0.  Returns H (B,3,3) float64 mapping kpts0 to kpts1 with H[2,2] = 1 (all zeros = no fit), the winning hypothesis' inlier
        mask (B,K0) uint8, n_inliers (B) int32 and best_h (B) int32 (-1 = no fit).  A pair's result does not depend on the batch around it.
        No host synchronisation."""
        who, dev = "estimate_homography", self.device
        for name, t in (("kpts0", kpts0), ("kpts1", kpts1), ("matches0", matches0)):
            if not isinstance(t, torch.Tensor) or t.device != dev:
                raise ImxError(f"{who}: {name} must be a tensor on {dev}, got {getattr(t, 'device', type(t))}")
        if matches0.dim() != 2 or matches0.dtype != torch.int64:
            raise ImxError(f"{who}: matches0 must be (B,K0) int64, got {tuple(matches0.shape)} {matches0.dtype}")
        B, K0 = (int(v) for v in matches0.shape)
        if kpts0.dtype != torch.float32 or kpts1.dtype != torch.float32:
            raise ImxError(f"{who}: keypoints must be float32, got {kpts0.dtype} and {kpts1.dtype}")
        if tuple(kpts0.shape) != (B, K0, 2) or kpts1.dim() != 3 or kpts1.shape[0] != B or kpts1.shape[2] != 2:
            raise ImxError(f"{who}: expected kpts0 ({B},{K0},2) and kpts1 ({B},K1,2), got {tuple(kpts0.shape)} and {tuple(kpts1.shape)}")
        K1 = int(kpts1.shape[1])
        if B < 1 or K0 < 1 or K1 < 1:
            raise ImxError(f"{who}: empty input B={B} K0={K0} K1={K1}")
        if counts0 is not None and not (isinstance(counts0, torch.Tensor) and counts0.dtype == torch.int32 and counts0.dim() == 1
                                        and counts0.numel() == B and counts0.device == dev and counts0.is_contiguous()):
            raise ImxError(f"{who}: counts0 must be a contiguous int32 tensor of {B} elements on {dev}")
        thr = float(ransac_thresh)
        if not (thr > 0.0 and math.isfinite(thr)):
            raise ImxError(f"{who}: ransac_thresh must be positive and finite, got {ransac_thresh!r}")
        kpts0, kpts1, matches0 = kpts0.contiguous(), kpts1.contiguous(), matches0.contiguous()
        H = torch.empty(B, 3, 3, dtype=torch.float64, device=dev)
        inl = torch.empty(B, K0, dtype=torch.uint8, device=dev)
        ninl = torch.empty(B, dtype=torch.int32, device=dev)
        best = torch.empty(B, dtype=torch.int32, device=dev)
        self._check(self.homog.imx_estimate_homography(self.handle, _ptr(kpts0), _ptr(kpts1), _ptr(matches0), _ptr(counts0), B, K0, K1, thr,
                                                       int(hypotheses), int(refine_iters), int(seed) & 0xFFFFFFFF, _ptr(H), _ptr(inl), _ptr(ninl),
                                                       _ptr(best), _stream(dev)))
        return H, inl, ninl, best

    def homography_corner_error(self, H, H_gt, size_hw):
        """The mean distance, in pixels, of the four corners of a (height, width) = size_hw image under H (B,3,3) and under H_gt (B,3,3;
        a device tensor or host matrices), in float64 on the device: (B) float64, +inf where H is all zeros (a failed fit).  No host
        synchronisation when H_gt is a tensor."""
        who, dev = "homography_corner_error", self.device
        if not isinstance(H, torch.Tensor) or H.device != dev or H.dtype != torch.float64 or H.dim() != 3 or tuple(H.shape[1:]) != (3, 3):
            raise ImxError(f"{who}: H must be a (B,3,3) float64 tensor on {dev}, got {getattr(H, 'dtype', type(H))} "
                           f"{tuple(getattr(H, 'shape', ()))} {getattr(H, 'device', None)}")
        B = int(H.shape[0])
        if B < 1:
            raise ImxError(f"{who}: empty batch")
        H, gt = H.contiguous(), self._matrices(H_gt, B, who)
        height, width = (int(v) for v in size_hw)
        if height < 1 or width < 1:
            raise ImxError(f"{who}: bad image size {size_hw!r}")
        err = torch.empty(B, dtype=torch.float64, device=dev)
        self._check(self.homog.imx_homography_corner_error(self.handle, _ptr(H), _ptr(gt), B, width, height, _ptr(err), _stream(dev)))
        return err

    def mutual_nn_match(self, desc0, desc1, n0=None, n1=None):
        """Mutual nearest neighbours by inner product -- for unit-norm descriptors the brute-force L2 matcher with cross-check of the
        SuperPoint paper's protocol (include/imx_speval.h).  desc{0,1}: (B,d,N) float32 tensors on the device, any strides (a transposed
        view of superpoint_batch's (B,K,d) is read in place); d is the tensors' own, not the configured descriptor_dim.  n0, n1: (B)
        int32 counts or None.  Returns matches0 (B,N0), matches1 (B,N1) int64 (-1 = no mutual neighbour) and sim0 (B,N0), sim1 (B,N1),
        the best similarity of every row, mutual or not.  The similarity matrix is never stored.  No host synchronisation."""
        who, dev = "mutual_nn_match", self.device
        for name, t in (("desc0", desc0), ("desc1", desc1)):
            if not isinstance(t, torch.Tensor) or t.device != dev:
                raise ImxError(f"{who}: {name} must be a tensor on {dev}, got {getattr(t, 'device', type(t))}")
            if t.dtype != torch.float32 or t.dim() != 3:
                raise ImxError(f"{who}: {name} must be (B,d,N) float32, got {tuple(t.shape)} {t.dtype}")
        if desc0.shape[0] != desc1.shape[0] or desc0.shape[1] != desc1.shape[1]:
            raise ImxError(f"{who}: the two sides differ in batch size or descriptor dim: {tuple(desc0.shape)} and {tuple(desc1.shape)}")
        B, D, N0 = (int(v) for v in desc0.shape)
        N1 = int(desc1.shape[2])
        if B < 1 or N0 < 1 or N1 < 1 or not 1 <= D <= 1024:
            raise ImxError(f"{who}: bad shape B={B} d={D} N0={N0} N1={N1} (B, N0, N1 >= 1, 1 <= d <= 1024)")
        for n in (n0, n1):
            if n is not None and not (isinstance(n, torch.Tensor) and n.dtype == torch.int32 and n.dim() == 1 and n.numel() == B
                                      and n.device == dev and n.is_contiguous()):
                raise ImxError(f"{who}: counts must be contiguous int32 tensors of {B} elements on {dev}")
        m0 = torch.empty(B, N0, dtype=torch.int64, device=dev)
        m1 = torch.empty(B, N1, dtype=torch.int64, device=dev)
        sim0 = torch.empty(B, N0, dtype=torch.float32, device=dev)
        sim1 = torch.empty(B, N1, dtype=torch.float32, device=dev)
        s0, s1 = desc0.stride(), desc1.stride()
        self._check(self.speval.imx_mutual_nn_match(self.handle, B, D, _ptr(desc0), s0[0], s0[1], s0[2], _ptr(n0), N0,
                                                    _ptr(desc1), s1[0], s1[1], s1[2], _ptr(n1), N1,
                                                    _ptr(m0), _ptr(m1), _ptr(sim0), _ptr(sim1), _stream(dev)))
        return m0, m1, sim0, sim1

    def keypoint_pair_metrics(self, kpts0, n0, kpts1, n1, H_gt, size_hw, eps=3.0, matches0=None):
        """The pair metrics of a detector under known warps (include/imx_speval.h): kpts0 (B,K0,2), kpts1 (B,K1,2) float32 (x, y), n0,
        n1 (B) int32 counts or None, H_gt (B,3,3) float64 on pixel coordinates mapping image 0 to image 1, size_hw = (height, width),
        matches0 (B,K0) int64 or None.  Returns counts (B,8) int32 = [v0, v1, r0, r1, m, c, bad, 0] and sums (B,2) float64: the points in
        the shared view, the repeated ones (a visible point of the other side within eps after warping), the matches and the correct
        ones, whether H_gt was singular, and the sums of the nearest distances of the repeated points.  K0, K1 <= 4096.  No host
        synchronisation."""
        who, dev = "keypoint_pair_metrics", self.device
        tensors = [("kpts0", kpts0), ("kpts1", kpts1), ("H_gt", H_gt)] + ([("matches0", matches0)] if matches0 is not None else [])
        for name, t in tensors:
            if not isinstance(t, torch.Tensor) or t.device != dev:
                raise ImxError(f"{who}: {name} must be a tensor on {dev}, got {getattr(t, 'device', type(t))}")
        if kpts0.dtype != torch.float32 or kpts1.dtype != torch.float32:
            raise ImxError(f"{who}: keypoints must be float32, got {kpts0.dtype} and {kpts1.dtype}")
        if kpts0.dim() != 3 or kpts1.dim() != 3 or kpts0.shape[2] != 2 or kpts1.shape[2] != 2 or kpts0.shape[0] != kpts1.shape[0]:
            raise ImxError(f"{who}: expected kpts0 (B,K0,2) and kpts1 (B,K1,2), got {tuple(kpts0.shape)} and {tuple(kpts1.shape)}")
        B, K0, K1 = int(kpts0.shape[0]), int(kpts0.shape[1]), int(kpts1.shape[1])
        if B < 1 or K0 < 1 or K1 < 1:
            raise ImxError(f"{who}: empty input B={B} K0={K0} K1={K1}")
        if H_gt.dtype != torch.float64 or tuple(H_gt.shape) != (B, 3, 3):
            raise ImxError(f"{who}: H_gt must be ({B},3,3) float64, got {tuple(H_gt.shape)} {H_gt.dtype}")
        if matches0 is not None and (matches0.dtype != torch.int64 or tuple(matches0.shape) != (B, K0)):
            raise ImxError(f"{who}: matches0 must be ({B},{K0}) int64, got {tuple(matches0.shape)} {matches0.dtype}")
        for n in (n0, n1):
            if n is not None and not (isinstance(n, torch.Tensor) and n.dtype == torch.int32 and n.dim() == 1 and n.numel() == B
                                      and n.device == dev and n.is_contiguous()):
                raise ImxError(f"{who}: counts must be contiguous int32 tensors of {B} elements on {dev}")
        height, width = (int(v) for v in size_hw)
        if height < 1 or width < 1:
            raise ImxError(f"{who}: bad image size {size_hw!r}")
        e = float(eps)
        if not (e >= 0.0 and math.isfinite(e)):
            raise ImxError(f"{who}: eps must be non-negative and finite, got {eps!r}")
        kpts0, kpts1, H_gt = kpts0.contiguous(), kpts1.contiguous(), H_gt.contiguous()
        matches0 = matches0.contiguous() if matches0 is not None else None
        counts = torch.empty(B, 8, dtype=torch.int32, device=dev)
        sums = torch.empty(B, 2, dtype=torch.float64, device=dev)
        self._check(self.speval.imx_keypoint_pair_metrics(self.handle, _ptr(kpts0), _ptr(n0), _ptr(kpts1), _ptr(n1), _ptr(matches0), _ptr(H_gt),
                                                          B, K0, K1, width, height, e, _ptr(counts), _ptr(sums), _stream(dev)))
        return counts, sums

    def knn_ratio_match(self, desc0, desc1, ratio=0.7, n0=None, n1=None):
        """Exact 2-NN + ratio test (superpoint_flann_test.py:66-74 without FLANN's approximation).
        desc{0,1}: (B,d,N) tensors, any strides.  Returns matches (B,N0) int64 (-1 = rejected), dist1, dist2 (B,N0)."""
        dev = self.device
        desc0, desc1 = desc0.to(dev, torch.float32), desc1.to(dev, torch.float32)
        # the library reads descriptor_dim channels of B pairs from both sides and B counts through raw pointers: refuse anything
        # else here instead of reading past a tensor
        if desc0.dim() != 3 or desc1.dim() != 3:
            raise ImxError(f"knn_ratio_match: descriptors must be (B,d,N), got {tuple(desc0.shape)} and {tuple(desc1.shape)}")
        if desc0.shape[1] != self.d or desc1.shape[1] != self.d:
            raise ImxError(f"knn_ratio_match: descriptor dims {desc0.shape[1]} / {desc1.shape[1]} != configured descriptor_dim {self.d}")
        if desc0.shape[0] != desc1.shape[0]:
            raise ImxError(f"knn_ratio_match: the two sides differ in batch size ({desc0.shape[0]} and {desc1.shape[0]})")
        B, _, N0 = desc0.shape
        N1 = desc1.shape[2]
        for n in (n0, n1):
            if n is not None and not (isinstance(n, torch.Tensor) and n.dtype == torch.int32 and n.dim() == 1 and n.numel() == B
                                      and n.device == dev and n.is_contiguous()):
                raise ImxError(f"knn_ratio_match: counts must be contiguous int32 tensors of {B} elements on {dev}")
        m = torch.empty(B, N0, dtype=torch.int64, device=dev)
        d1 = torch.empty(B, N0, dtype=torch.float32, device=dev)
        d2 = torch.empty(B, N0, dtype=torch.float32, device=dev)
        if N0 == 0:
            return m, d1, d2
        s0, s1 = desc0.stride(), desc1.stride()
        self._check(self.lib.imx_knn_ratio_match(self.handle, B, _ptr(desc0), s0[0], s0[1], s0[2], _ptr(n0), N0,
                                                 _ptr(desc1), s1[0], s1[1], s1[2], _ptr(n1), N1, float(ratio),
                                                 _ptr(m), _ptr(d1), _ptr(d2), _stream(dev)))
        return m, d1, d2

    def ingest(self, img_u8, size_hw=None, out=None):
        """cv2.resize + /255 of datasets/SSHIDataset.py:19-27 on the GPU.  img_u8: (B,Hs,Ws) or (Hs,Ws) uint8 tensor
        (moved to the device if needed); size_hw None = no resize.  Returns (B,1,H,W) float32 in [0,1]."""
        if img_u8.dtype != torch.uint8:
            raise TypeError("ingest expects uint8 gray images")
        src = img_u8.to(self.device, non_blocking=True)
        if src.dim() == 2:
            src = src[None]
        src = src.contiguous()
        B, Hs, Ws = src.shape
        H, W = (Hs, Ws) if size_hw is None else size_hw
        dst = out if out is not None else torch.empty(B, 1, H, W, dtype=torch.float32, device=self.device)
        self._check(self.lib.imx_ingest_resize_u8(self.handle, _ptr(src), B, Hs, Ws, Hs * Ws, _ptr(dst), H, W, _stream(self.device)))
        return dst

    def warp_affine_u8(self, src_u8, M, size_hw=None):
        """cv2.warpAffine(source_original*255, M, (W,H)) as cv2.imwrite stores it (superpoint_glue_test.py:101-113).
        src_u8 (Hs,Ws) uint8 tensor; M forward 2x3 (array-like, host).  Returns (H,W) uint8 on the device."""
        src = src_u8.to(self.device).contiguous()
        Hs, Ws = src.shape
        H, W = (Hs, Ws) if size_hw is None else size_hw
        import numpy as np
        Mh = np.ascontiguousarray(np.asarray(M, np.float64).reshape(6))
        dst = torch.empty(H, W, dtype=torch.uint8, device=self.device)
        self._check(self.lib.imx_warp_affine_u8(self.handle, _ptr(src), Hs, Ws, Mh.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                _ptr(dst), H, W, _stream(self.device)))
        return dst

    def op_nms(self, scores, radius):
        """simple_nms on a (B,H,W) score map (single-stage entry point, used by parity tests)."""
        scores = scores.to(self.device, torch.float32).contiguous()
        out = torch.empty_like(scores)
        B, H, W = scores.shape
        self._check(self.lib.imx_op_nms(self.handle, _ptr(scores), _ptr(out), B, H, W, int(radius), _stream(self.device)))
        return out

    # ------------------------------------------------------------------ homographic adaptation (pseudo-label export)
    def _f32(self, t, shape, what):
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(np.asarray(t, dtype=np.float32))
        t = t.to(self.device, torch.float32).contiguous()
        if tuple(t.shape) != tuple(shape):
            raise ImxError(f"{what}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
        return t

    def warp_homography(self, src, mats, mode="bilinear"):
        """inv_warp_image_batch (utils/utils.py:388-421).  src (N,H,W), or (H,W) shared by all N matrices, or a (H, W) pair of
        ints = an all-ones image (mode 'nearest': compute_valid_mask); mats (N,3,3).  Returns (N,H,W) float32."""
        if mode not in ("bilinear", "nearest"):
            raise ImxError(f"warp_homography: mode must be 'bilinear' or 'nearest', got {mode!r}")
        N = int(mats.shape[0])
        mats = self._f32(mats, (N, 3, 3), "warp_homography: mats")
        if isinstance(src, (tuple, list)):
            (H, W), img, shared = (int(v) for v in src), None, 1
        else:
            shared = int(src.dim() == 2)
            H, W = int(src.shape[-2]), int(src.shape[-1])
            img = self._f32(src, (H, W) if shared else (N, H, W), "warp_homography: src")
        dst = torch.empty(N, H, W, dtype=torch.float32, device=self.device)
        self._check(self.lib.imx_warp_homography(self.handle, _ptr(img), shared, N, H, W, _ptr(mats), int(mode == "nearest"),
                                                 _ptr(dst), _stream(self.device)))
        return dst

    def combine_heatmap(self, heat, mask, unwarp, want_count=False):
        """combine_heatmap (utils/utils.py:507-518), fused.  heat, mask (N,H,W); unwarp (N,3,3).  Returns the (H,W) map
        [, the (H,W) sum of the un-warped masks]."""
        N, H, W = (int(v) for v in heat.shape)
        heat = self._f32(heat, (N, H, W), "combine_heatmap: heat")
        mask = self._f32(mask, (N, H, W), "combine_heatmap: mask")
        unwarp = self._f32(unwarp, (N, 3, 3), "combine_heatmap: unwarp")
        out = torch.empty(H, W, dtype=torch.float32, device=self.device)
        cnt = torch.empty(H, W, dtype=torch.float32, device=self.device) if want_count else None
        self._check(self.lib.imx_combine_heatmap(self.handle, _ptr(heat), _ptr(mask), _ptr(unwarp), N, H, W, _ptr(out), _ptr(cnt),
                                                 _stream(self.device)))
        return (out, cnt) if want_count else out

    def superpoint_heatmap(self, x):
        """x (B,1,H,W) -> detector heatmaps (B,1,H,W): the dense SuperPoint's `semi` through flattenDetection
        (model_wrap.py:283-309 with onlyHeatmap); the descriptor head is not run."""
        x = self._image(x)
        B, _, H, W = x.shape
        heat = torch.empty(B, 1, H, W, dtype=torch.float32, device=self.device)
        self._check(self.lib.imx_superpoint_heatmap(self.handle, _ptr(x), B, H, W, _ptr(heat), _stream(self.device)))
        return heat

    def homography_adapt(self, img, warp, unwarp, want_count=False):
        """superpoint_export_pseudo.py:58-79 for one image (H,W): warp (N,3,3) are the matrices the image is warped by (the
        dataset's inv_homographies), unwarp (N,3,3) the ones the heatmaps come back by (its homographies).  Returns the
        aggregated (H,W) heatmap [, the count map]."""
        H, W = int(img.shape[-2]), int(img.shape[-1])
        N = int(warp.shape[0])
        img = self._f32(img.reshape(H, W) if isinstance(img, torch.Tensor) else img, (H, W), "homography_adapt: img")
        warp = self._f32(warp, (N, 3, 3), "homography_adapt: warp")
        unwarp = self._f32(unwarp, (N, 3, 3), "homography_adapt: unwarp")
        out = torch.empty(H, W, dtype=torch.float32, device=self.device)
        cnt = torch.empty(H, W, dtype=torch.float32, device=self.device) if want_count else None
        self._check(self.lib.imx_homography_adapt(self.handle, _ptr(img), H, W, N, _ptr(warp), _ptr(unwarp), _ptr(out), _ptr(cnt),
                                                  _stream(self.device)))
        return (out, cnt) if want_count else out

    def heatmap_points(self, heatmap, conf_thresh, nms_dist, top_k=0, subpixel=False, cap=None):
        """getPtsFromHeatmap (+ soft_argmax_points, top_k) on a (H,W) map, no host sync: returns (pts (cap,3) rows (x, y, conf)
        by descending conf, count (1) int32).  count is the number of points whatever cap is; rows past min(count, cap) are
        unwritten.  cap defaults to top_k if > 0, else to the most survivors a map of this size can have."""
        H, W = int(heatmap.shape[-2]), int(heatmap.shape[-1])
        heatmap = self._f32(heatmap.reshape(H, W) if isinstance(heatmap, torch.Tensor) else heatmap, (H, W), "heatmap_points: heatmap")
        if cap is None:
            r = max(int(nms_dist), 0) + 1
            cap = int(top_k) if top_k and top_k > 0 else -(-H // r) * -(-W // r)
        # one buffer: the rows, then the count word -- heatmap_points_host copies both in one transfer
        buf = torch.empty(int(cap) * 3 + 1, dtype=torch.float32, device=self.device)
        pts, cnt = buf[:int(cap) * 3].view(int(cap), 3), buf[int(cap) * 3:].view(torch.int32)
        self._check(self.lib.imx_heatmap_points(self.handle, _ptr(heatmap), H, W, float(conf_thresh), int(nms_dist), int(top_k or 0),
                                                int(bool(subpixel)), _ptr(pts), int(cap), _ptr(cnt), _stream(self.device)))
        return pts, cnt

    def heatmap_points_host(self, heatmap, conf_thresh, nms_dist, top_k=0, subpixel=False):
        """heatmap_points, then ONE device-to-host copy (a synchronisation): the (K,3) float32 numpy rows (x, y, conf)."""
        pts, cnt = self.heatmap_points(heatmap, conf_thresh, nms_dist, top_k=top_k, subpixel=subpixel)
        rows = pts._base.cpu().numpy()                    # pts and cnt are views of one buffer: rows, then the count word
        k = min(int(rows[-1:].view(np.int32)[0]), pts.shape[0])
        return rows[:-1].reshape(-1, 3)[:k].copy()

    # ------------------------------------------------------------------ SuperGlue training pairs (datasets/GlueSparse.py)
    def _matrices(self, M, B, what, invert=False):
        """(B,3,3) float64 on the device; `invert`: each matrix inverted on the host in double first (cv2.warpPerspective's own
        inversion; a device tensor is read back for it, so batch producers pass host matrices)."""
        if isinstance(M, torch.Tensor) and not invert:
            m = M.to(self.device, torch.float64).reshape(-1, 3, 3).contiguous()
        else:
            a = (M.detach().cpu().numpy() if isinstance(M, torch.Tensor) else np.asarray(M)).astype(np.float64).reshape(-1, 3, 3)
            if invert:
                a = np.stack([np.linalg.inv(x) for x in a])
            m = torch.from_numpy(np.ascontiguousarray(a)).to(self.device, non_blocking=True)
        if m.shape[0] != B:
            raise ImxError(f"{what}: {m.shape[0]} matrices for a batch of {B}")
        return m

    def warp_perspective_u8(self, img_u8, M, inverse=False):
        """cv2.warpPerspective(image, M, (W,H)) of datasets/GlueSparse.py:32 for a batch: img_u8 (B,H,W) or (H,W) uint8, M (B,3,3)
        forward matrices (float64, host; `inverse`: M already holds the inverses).  Returns (B,H,W) uint8 on the device."""
        if img_u8.dtype != torch.uint8:
            raise TypeError("warp_perspective_u8 expects uint8 gray images")
        src = img_u8.to(self.device, non_blocking=True)
        src = (src[None] if src.dim() == 2 else src).contiguous()
        B, H, W = src.shape
        minv = self._matrices(M, B, "warp_perspective_u8", invert=not inverse)
        dst = torch.empty(B, H, W, dtype=torch.uint8, device=self.device)
        self._check(self.lib.imx_warp_perspective_u8(self.handle, _ptr(src), H * W, _ptr(minv), _ptr(dst), B, H, W, _stream(self.device)))
        return dst

    def gt_matches(self, kpts0, kpts1, M, n0=None, n1=None, radius=3.0, want_proj=False):
        """datasets/GlueSparse.py:64-82 for B pairs, no host sync: kpts{0,1} (B,N{0,1},2) float32, M (B,3,3) forward matrices,
        n{0,1} (B) int32 counts or None.  Returns dict: gt0 (B,N0), gt1 (B,N1), all_matches (B,2,N0+N1) int64, n_matches, n_all
        (B) int32 [, projected (B,N0,2)]."""
        dev = self.device
        kpts0 = kpts0.to(dev, torch.float32).contiguous()
        kpts1 = kpts1.to(dev, torch.float32).contiguous()
        B, N0, N1 = kpts0.shape[0], kpts0.shape[1], kpts1.shape[1]
        if kpts1.shape[0] != B:
            raise ImxError("gt_matches: the two sides differ in batch size")
        m = self._matrices(M, B, "gt_matches")
        for n in (n0, n1):
            if n is not None and not (n.dtype == torch.int32 and n.numel() == B and n.device == dev and n.is_contiguous()):
                raise ImxError(f"gt_matches: counts must be contiguous int32 tensors of {B} elements on {dev}")
        out = {"gt0": torch.empty(B, N0, dtype=torch.int64, device=dev), "gt1": torch.empty(B, N1, dtype=torch.int64, device=dev),
               "all_matches": torch.empty(B, 2, N0 + N1, dtype=torch.int64, device=dev),
               "n_matches": torch.empty(B, dtype=torch.int32, device=dev), "n_all": torch.empty(B, dtype=torch.int32, device=dev)}
        if want_proj:
            out["projected"] = torch.empty(B, N0, 2, dtype=torch.float32, device=dev)
        self._check(self.lib.imx_gt_matches(self.handle, B, _ptr(kpts0), _ptr(n0), N0, _ptr(kpts1), _ptr(n1), N1, _ptr(m), float(radius),
                                            _ptr(out.get("projected")), _ptr(out["gt0"]), _ptr(out["gt1"]), _ptr(out["all_matches"]),
                                            _ptr(out["n_matches"]), _ptr(out["n_all"]), _stream(dev)))
        return out

    def match_loss(self, all_matches, n_all, matches0=None, gt0=None):
        """The objective of superglue/models/superglue_train.py:289-299 for the pairs of the LAST superglue() / match_pairs() of this
        engine: all_matches (B,2,L) int64, n_all (B) int32.  Returns loss (B) float32 [, stats (B,3) int32 = ground-truth, predicted
        and correct matches, when matches0 and gt0 (B,N0) are given]."""
        dev = self.device
        all_matches = all_matches.to(dev, torch.int64).contiguous()
        n_all = n_all.to(dev, torch.int32).contiguous()
        B, _, Lc = all_matches.shape
        if n_all.numel() != B:
            raise ImxError(f"match_loss: {n_all.numel()} column counts for a batch of {B}")
        loss = torch.empty(B, dtype=torch.float32, device=dev)
        stats = None
        if matches0 is not None and gt0 is not None:
            matches0 = matches0.to(dev, torch.int64).contiguous()
            gt0 = gt0.to(dev, torch.int64).contiguous()
            if matches0.shape != gt0.shape or matches0.shape[0] != B:
                raise ImxError(f"match_loss: matches0 {tuple(matches0.shape)} and gt0 {tuple(gt0.shape)} must both be (B,N0)")
            stats = torch.empty(B, 3, dtype=torch.int32, device=dev)
        self._check(self.lib.imx_match_loss(self.handle, B, _ptr(all_matches), _ptr(n_all), Lc, _ptr(matches0 if stats is not None else None),
                                            _ptr(gt0 if stats is not None else None), _ptr(loss), _ptr(stats), _stream(dev)))
        return (loss, stats) if stats is not None else loss

    def train_pairs(self, img_u8, M, radius=3.0):
        """B training samples of datasets/GlueSparse.py:24-104 on one stream with no host synchronisation: the warp of every image by
        its matrix, `/255` of both stacks, SuperPoint on the 2B images (max_keypoints = K > 0) and the ground-truth assignment.
        img_u8 (B,H,W) uint8, M (B,3,3) float64 forward matrices (host).  Returns dict of device tensors: warped (B,H,W) uint8,
        keypoints{0,1} (B,K,2), scores{0,1} (B,K), descriptors{0,1} (B,K,d), counts{0,1} (B), and gt_matches' entries."""
        K = self.max_keypoints
        if K <= 0:
            raise ImxError("train_pairs needs max_keypoints > 0")
        src = img_u8.to(self.device, non_blocking=True).contiguous()
        B, H, W = src.shape
        M = (M.detach().cpu().numpy() if isinstance(M, torch.Tensor) else np.asarray(M)).astype(np.float64).reshape(-1, 3, 3)
        warped = self.warp_perspective_u8(src, M)
        x = torch.empty(2 * B, 1, H, W, dtype=torch.float32, device=self.device)
        self.ingest(src, out=x[:B])
        self.ingest(warped, out=x[B:])
        kpts, scores, desc, counts = self.superpoint_batch(x)
        out = {"warped": warped, "keypoints0": kpts[:B], "keypoints1": kpts[B:], "scores0": scores[:B], "scores1": scores[B:],
               "descriptors0": desc[:B], "descriptors1": desc[B:], "counts0": counts[:B], "counts1": counts[B:]}
        out.update(self.gt_matches(out["keypoints0"], out["keypoints1"], M, counts[:B], counts[B:], radius))
        return out

    # ------------------------------------------------------------------ SuperPoint descriptor training (Train_model_heatmap.py:83-314)
    def _scaled(self, homographies, B, width, height, shift):
        """inverse(trans) @ H @ trans with trans = [[2/width, 0, shift], [0, 2/height, shift], [0, 0, 1]] in fp32: the reference's torch
        expression (homography_scaling_torch, utils/utils.py:586-589; scale_homography_torch, utils/homographies.py:121-125).  A host
        tensor is multiplied on the host, as the reference does; a device tensor on the device (no synchronisation)."""
        Hm = homographies if isinstance(homographies, torch.Tensor) else torch.as_tensor(np.asarray(homographies, dtype=np.float32))
        Hm = Hm.type(torch.float32).reshape(-1, 3, 3)
        if Hm.shape[0] != B:
            raise ImxError(f"{Hm.shape[0]} homographies for a batch of {B}")
        trans = torch.tensor([[2. / width, 0., shift], [0., 2. / height, shift], [0., 0., 1.]], dtype=torch.float32)
        inv = torch.inverse(trans)
        if Hm.device.type == "cpu":
            out = torch.stack([inv @ m @ trans for m in Hm])           # one 2-D product chain per matrix, as the reference forms it
        else:
            out = inv.to(Hm.device) @ Hm @ trans.to(Hm.device)
        return out.to(self.device, non_blocking=True).contiguous()

    def _counts(self, counts, B, what):
        if counts is None:
            return None
        c = counts if isinstance(counts, torch.Tensor) else torch.as_tensor(np.asarray(counts, dtype=np.int32))
        c = c.to(self.device, torch.int32).contiguous()
        if c.numel() != B:
            raise ImxError(f"{what}: {c.numel()} counts for a batch of {B}")
        return c

    def warp_labels(self, pts, counts, homographies, H, W, want_res=True, pixel_space=False):
        """warpLabels (datasets/data_tools.py:36-54) for B images, or ALLSS.points_to_2D with homographies=None.  pts (B,Kcap,2) (x, y),
        counts (B) int32 or None, homographies (B,3,3) on [-1,1]^2 coordinates (scaled to pixels here by the reference's expression).
        Returns (labels (B,H,W), res (B,2,H,W) or None, flag (1) int32 device word: non-zero = a point outside the image with
        homographies=None).  Two points on one pixel: the higher point index writes the residual."""
        pts = pts if isinstance(pts, torch.Tensor) else torch.as_tensor(np.asarray(pts, dtype=np.float32))
        pts = pts.to(self.device, torch.float32).contiguous()
        if pts.dim() != 3 or pts.shape[2] != 2:
            raise ImxError(f"warp_labels: pts must be (B,Kcap,2), got {tuple(pts.shape)}")
        B, K = int(pts.shape[0]), int(pts.shape[1])
        counts = self._counts(counts, B, "warp_labels")
        if homographies is None:
            mats = None
        elif pixel_space:                # the matrices already act on pixel coordinates: passed to the kernel as they are
            mats = self._f32(homographies, (B, 3, 3), "warp_labels: homographies")
        else:
            mats = self._scaled(homographies, B, float(W), float(H), -1.)
        labels = torch.empty(B, int(H), int(W), dtype=torch.float32, device=self.device)
        res = torch.empty(B, 2, int(H), int(W), dtype=torch.float32, device=self.device) if want_res else None
        flag = torch.empty(1, dtype=torch.int32, device=self.device)
        self._check(self.train.imx_warp_labels(self.handle, _ptr(pts), _ptr(counts), B, K, _ptr(mats), int(H), int(W), _ptr(labels), _ptr(res),
                                             _ptr(flag), _stream(self.device)))
        return labels, res, flag

    def erode_mask(self, mask, radius):
        """The margin of compute_valid_mask (utils/utils.py:449-452): cv2.erode by the (2r, 2r) elliptic element on (B,H,W) masks, as
        restated in tests/sptrain_ref.py (parity with OpenCV itself is unpinned).  radius 0 copies."""
        B, H, W = (int(v) for v in mask.shape)
        mask = self._f32(mask, (B, H, W), "erode_mask: mask")
        out = torch.empty_like(mask)
        self._check(self.train.imx_erode_mask(self.handle, _ptr(mask), _ptr(out), B, H, W, int(radius), _stream(self.device)))
        return out

    def detector_loss(self, semi, labels, mask, loss_type="softmax"):
        """labels2Dto3D + getMasks + detector_loss (Train_model_heatmap.py:72-81) fused: semi (B,65,H/8,W/8), labels and mask (B,H,W)
        or (B,1,H,W).  Returns a (2) device tensor {loss, sum of the cell masks}."""
        if loss_type != "softmax":
            raise NotImplementedError(f"detector_loss: only loss_type 'softmax' (the shipped yaml) is served, got {loss_type!r}")
        B, C, Hc, Wc = (int(v) for v in semi.shape)
        if C != 65:
            raise ImxError(f"detector_loss: semi must have 65 channels, got {C}")
        semi = self._f32(semi, (B, 65, Hc, Wc), "detector_loss: semi")
        labels = self._f32(labels.reshape(B, Hc * 8, Wc * 8), (B, Hc * 8, Wc * 8), "detector_loss: labels")
        mask = self._f32(mask.reshape(B, Hc * 8, Wc * 8), (B, Hc * 8, Wc * 8), "detector_loss: mask")
        out = torch.empty(2, dtype=torch.float32, device=self.device)
        self._check(self.train.imx_detector_loss(self.handle, _ptr(semi), _ptr(labels), _ptr(mask), B, Hc * 8, Wc * 8, _ptr(out),
                                               _stream(self.device)))
        return out

    def _cell_mats(self, homographies, B, Hc, Wc, cell_space):
        if cell_space:                   # the matrices already act on cell coordinates: passed to the kernel as they are
            return self._f32(homographies, (B, 3, 3), "homographies")
        return self._scaled(homographies, B, float(Wc), float(Hc), -1.)

    def desc_pairs(self, homographies, Hc, Wc, cell_space=False):
        """The first stage of desc_loss_sparse alone (sparse_loss.py:118-124), for the caller's draws: homographies (B,3,3) on [-1,1]^2
        -> (pairs (B,Hc Wc,2) int32: the compacted (a, b) flat cell indices, -1 past the count; n_valid (B) int32)."""
        B = int(homographies.shape[0]) if hasattr(homographies, "shape") and len(homographies.shape) == 3 else 1
        hcell = self._cell_mats(homographies, B, Hc, Wc, cell_space)
        pairs = torch.empty(B, int(Hc) * int(Wc), 2, dtype=torch.int32, device=self.device)
        n_valid = torch.empty(B, dtype=torch.int32, device=self.device)
        self._check(self.train.imx_desc_pairs(self.handle, _ptr(hcell), B, int(Hc), int(Wc), _ptr(pairs), _ptr(n_valid), _stream(self.device)))
        return pairs, n_valid

    def desc_loss_sparse(self, desc_a, desc_b, homographies, choice, nonmatch_b, lamda_d=250., margin=0.2, method="1d", want_pairs=False,
                         cell_space=False):
        """descriptor_loss_sparse (loss_functions/sparse_loss.py:98-174) for B images, indices in, losses out.  desc_{a,b} (B,d,Hc,Wc);
        homographies (B,3,3) on [-1,1]^2 (scaled to cells here by scale_homography_torch's expression); choice (B,M) int32 indices into
        the compacted pair list; nonmatch_b (B,M,R) int32 flat cell indices.  Returns dict: out (B,5) = {loss, lamda_d match, non_match,
        num_hard_negatives, n_valid}, mean (3), flag (1) int32 [, pairs (B,Hc Wc,2) int32]."""
        if method not in ("1d", "2d"):
            raise ImxError(f"desc_loss_sparse: method must be '1d' or '2d', got {method!r}")
        B, d, Hc, Wc = (int(v) for v in desc_a.shape)
        desc_a = self._f32(desc_a, (B, d, Hc, Wc), "desc_loss_sparse: desc_a")
        desc_b = self._f32(desc_b, (B, d, Hc, Wc), "desc_loss_sparse: desc_b")
        hcell = self._cell_mats(homographies, B, Hc, Wc, cell_space)
        choice = choice.to(self.device, torch.int32).contiguous()
        nonmatch_b = nonmatch_b.to(self.device, torch.int32).contiguous()
        if choice.dim() != 2 or choice.shape[0] != B or nonmatch_b.dim() != 3 or tuple(nonmatch_b.shape[:2]) != tuple(choice.shape):
            raise ImxError(f"desc_loss_sparse: choice {tuple(choice.shape)} must be (B,M) and nonmatch_b {tuple(nonmatch_b.shape)} (B,M,R)")
        M, R = int(choice.shape[1]), int(nonmatch_b.shape[2])
        res = {"out": torch.empty(B, 5, dtype=torch.float32, device=self.device), "mean": torch.empty(3, dtype=torch.float32, device=self.device),
               "flag": torch.empty(1, dtype=torch.int32, device=self.device)}
        if want_pairs:
            res["pairs"] = torch.empty(B, Hc * Wc, 2, dtype=torch.int32, device=self.device)
        self._check(self.train.imx_desc_loss_sparse(self.handle, _ptr(desc_a), _ptr(desc_b), B, d, Hc, Wc, _ptr(hcell), _ptr(choice), _ptr(nonmatch_b),
                                                  M, R, float(lamda_d), float(margin), 1 if method == "1d" else 2, _ptr(res["out"]),
                                                  _ptr(res["mean"]), _ptr(res.get("pairs")), _ptr(res["flag"]), _stream(self.device)))
        return res

    def sp_train_losses(self, images, pts, counts, homographies, inv_homographies, choice, nonmatch_b, erosion_radius=0, lamda_d=250.,
                        margin=0.2, method="2d", lambda_loss=1.):
        """One validation batch of Train_model_heatmap.py:83-314 on one stream without a host synchronisation: the warped images
        (inv_warp_image, bilinear) and their valid masks (nearest, eroded), both label maps, the dense SuperPoint on the 2B images, both
        detector losses and the sparse descriptor loss.  images (B,1,H,W) or (B,H,W); pts (B,Kcap,2) / counts (B): the pseudo-labels;
        homographies / inv_homographies (B,3,3) on [-1,1]^2 as ALLSS hands them out; choice (B,M) / nonmatch_b (B,M,R): the caller's draws
        (see desc_loss_sparse).  Returns a dict of device tensors: loss, loss_det, loss_det_warp, loss_desc, positive_dist, negative_dist
        (scalars), desc (the desc_loss_sparse dict), labels_2D, warped_labels, warped_res, warped_img, valid_mask, warped_valid_mask, semi,
        semi_warp, coarse_desc, coarse_desc_warp, flag (of the unwarped label map)."""
        B, H, W = int(images.shape[0]), int(images.shape[-2]), int(images.shape[-1])
        img = self._f32(images.reshape(B, H, W), (B, H, W), "sp_train_losses: images")
        inv = self._f32(inv_homographies, (B, 3, 3), "sp_train_losses: inv_homographies")
        x = torch.empty(2 * B, 1, H, W, dtype=torch.float32, device=self.device)
        x[:B, 0].copy_(img)
        st = _stream(self.device)
        self._check(self.lib.imx_warp_homography(self.handle, _ptr(img), 0, B, H, W, _ptr(inv), 0, _ptr(x[B:]), st))
        warped_mask = self.erode_mask(self.warp_homography((H, W), inv, mode="nearest"), erosion_radius)
        valid_mask = torch.ones(B, H, W, dtype=torch.float32, device=self.device)     # ALLSS: compute_valid_mask under the identity
        labels, _, flag = self.warp_labels(pts, counts, None, H, W, want_res=False)
        wlabels, wres, _ = self.warp_labels(pts, counts, homographies, H, W)
        semi, desc = self.superpoint_dense(x)
        det = self.detector_loss(semi[:B], labels, valid_mask)
        det_w = self.detector_loss(semi[B:], wlabels, warped_mask)
        dl = self.desc_loss_sparse(desc[:B], desc[B:], homographies, choice, nonmatch_b, lamda_d=lamda_d, margin=margin, method=method)
        loss = det[0] + det_w[0] + float(lambda_loss) * dl["mean"][0]
        return {"loss": loss, "loss_det": det[0], "loss_det_warp": det_w[0], "loss_desc": dl["mean"][0], "positive_dist": dl["mean"][1],
                "negative_dist": dl["mean"][2], "desc": dl, "labels_2D": labels, "warped_labels": wlabels, "warped_res": wres,
                "warped_img": x[B:], "valid_mask": valid_mask, "warped_valid_mask": warped_mask, "semi": semi[:B], "semi_warp": semi[B:],
                "coarse_desc": desc[:B], "coarse_desc_warp": desc[B:], "flag": flag}

    # ------------------------------------------------------------------ gradients of the two training losses (include/imx_train.h)
    def _gout(self, gout):
        if gout is None:
            return None
        if not isinstance(gout, torch.Tensor):                           # a fill kernel on the stream: no host-to-device copy, no wait
            return torch.full((1,), float(gout), dtype=torch.float32, device=self.device)
        return gout.to(self.device, torch.float32).reshape(1).contiguous()

    def detector_loss_grad(self, semi, labels, mask, gout=None, loss_type="softmax"):
        """detector_loss and its derivative with respect to semi in one call: returns (out (2) = {loss, sum of the cell masks},
        grad_semi (B,65,H/8,W/8) = gout d loss / d semi).  gout: a device scalar (or a number), None = 1.  The derivative is that of the
        conditioned form the library evaluates (include/imx_train.h)."""
        if loss_type != "softmax":
            raise NotImplementedError(f"detector_loss_grad: only loss_type 'softmax' (the shipped yaml) is served, got {loss_type!r}")
        B, C, Hc, Wc = (int(v) for v in semi.shape)
        if C != 65:
            raise ImxError(f"detector_loss_grad: semi must have 65 channels, got {C}")
        semi = self._f32(semi, (B, 65, Hc, Wc), "detector_loss_grad: semi")
        labels = self._f32(labels.reshape(B, Hc * 8, Wc * 8), (B, Hc * 8, Wc * 8), "detector_loss_grad: labels")
        mask = self._f32(mask.reshape(B, Hc * 8, Wc * 8), (B, Hc * 8, Wc * 8), "detector_loss_grad: mask")
        gout = self._gout(gout)
        out = torch.empty(2, dtype=torch.float32, device=self.device)
        grad = torch.empty(B, 65, Hc, Wc, dtype=torch.float32, device=self.device)
        self._check(self.train.imx_detector_loss_grad(self.handle, _ptr(semi), _ptr(labels), _ptr(mask), B, Hc * 8, Wc * 8, _ptr(gout), _ptr(out),
                                                    _ptr(grad), _stream(self.device)))
        return out, grad

    def desc_loss_sparse_grad(self, desc_a, desc_b, homographies, choice, nonmatch_b, lamda_d=250., margin=0.2, method="1d", gout=None,
                              want_pairs=False, cell_space=False):
        """desc_loss_sparse and the derivative of its batch-mean total (mean[0]) with respect to both descriptor maps in one call.  The
        arguments of desc_loss_sparse plus gout (a device scalar or a number, None = 1).  Returns its dict plus grad_a and grad_b
        (B,d,Hc,Wc).  Bit 2 of flag: an image without a valid pair (zero gradients)."""
        if method not in ("1d", "2d"):
            raise ImxError(f"desc_loss_sparse_grad: method must be '1d' or '2d', got {method!r}")
        B, d, Hc, Wc = (int(v) for v in desc_a.shape)
        desc_a = self._f32(desc_a, (B, d, Hc, Wc), "desc_loss_sparse_grad: desc_a")
        desc_b = self._f32(desc_b, (B, d, Hc, Wc), "desc_loss_sparse_grad: desc_b")
        hcell = self._cell_mats(homographies, B, Hc, Wc, cell_space)
        choice = choice.to(self.device, torch.int32).contiguous()
        nonmatch_b = nonmatch_b.to(self.device, torch.int32).contiguous()
        if choice.dim() != 2 or choice.shape[0] != B or nonmatch_b.dim() != 3 or tuple(nonmatch_b.shape[:2]) != tuple(choice.shape):
            raise ImxError(f"desc_loss_sparse_grad: choice {tuple(choice.shape)} must be (B,M) and nonmatch_b {tuple(nonmatch_b.shape)} (B,M,R)")
        M, R = int(choice.shape[1]), int(nonmatch_b.shape[2])
        gout = self._gout(gout)
        res = {"out": torch.empty(B, 5, dtype=torch.float32, device=self.device), "mean": torch.empty(3, dtype=torch.float32, device=self.device),
               "flag": torch.empty(1, dtype=torch.int32, device=self.device),
               "grad_a": torch.empty(B, d, Hc, Wc, dtype=torch.float32, device=self.device),
               "grad_b": torch.empty(B, d, Hc, Wc, dtype=torch.float32, device=self.device)}
        if want_pairs:
            res["pairs"] = torch.empty(B, Hc * Wc, 2, dtype=torch.int32, device=self.device)
        self._check(self.train.imx_desc_loss_sparse_grad(self.handle, _ptr(desc_a), _ptr(desc_b), B, d, Hc, Wc, _ptr(hcell), _ptr(choice),
                                                       _ptr(nonmatch_b), M, R, float(lamda_d), float(margin), 1 if method == "1d" else 2,
                                                       _ptr(gout), _ptr(res["out"]), _ptr(res["mean"]), _ptr(res.get("pairs")), _ptr(res["flag"]),
                                                       _ptr(res["grad_a"]), _ptr(res["grad_b"]), _stream(self.device)))
        return res

    def sp_train_loss_grads(self, images, pts, counts, homographies, inv_homographies, choice, nonmatch_b, erosion_radius=0, lamda_d=250.,
                            margin=0.2, method="2d", lambda_loss=1.):
        """sp_train_losses (same arguments, same stages, same stream, no host synchronisation) with the two losses run as
        value-and-gradient calls: returns its dict, bit-identical, plus grad_semi, grad_semi_warp (B,65,H/8,W/8), grad_desc and
        grad_desc_warp (B,d,H/8,W/8): d loss / d of what the network emitted, loss = loss_det + loss_det_warp + lambda_loss loss_desc."""
        B, H, W = int(images.shape[0]), int(images.shape[-2]), int(images.shape[-1])
        img = self._f32(images.reshape(B, H, W), (B, H, W), "sp_train_loss_grads: images")
        inv = self._f32(inv_homographies, (B, 3, 3), "sp_train_loss_grads: inv_homographies")
        x = torch.empty(2 * B, 1, H, W, dtype=torch.float32, device=self.device)
        x[:B, 0].copy_(img)
        st = _stream(self.device)
        self._check(self.lib.imx_warp_homography(self.handle, _ptr(img), 0, B, H, W, _ptr(inv), 0, _ptr(x[B:]), st))
        warped_mask = self.erode_mask(self.warp_homography((H, W), inv, mode="nearest"), erosion_radius)
        valid_mask = torch.ones(B, H, W, dtype=torch.float32, device=self.device)
        labels, _, flag = self.warp_labels(pts, counts, None, H, W, want_res=False)
        wlabels, wres, _ = self.warp_labels(pts, counts, homographies, H, W)
        semi, desc = self.superpoint_dense(x)
        det, g_semi = self.detector_loss_grad(semi[:B], labels, valid_mask)
        det_w, g_semi_w = self.detector_loss_grad(semi[B:], wlabels, warped_mask)
        dl = self.desc_loss_sparse_grad(desc[:B], desc[B:], homographies, choice, nonmatch_b, lamda_d=lamda_d, margin=margin, method=method,
                                        gout=float(lambda_loss))
        g_a, g_b = dl.pop("grad_a"), dl.pop("grad_b")
        loss = det[0] + det_w[0] + float(lambda_loss) * dl["mean"][0]
        return {"loss": loss, "loss_det": det[0], "loss_det_warp": det_w[0], "loss_desc": dl["mean"][0], "positive_dist": dl["mean"][1],
                "negative_dist": dl["mean"][2], "desc": dl, "labels_2D": labels, "warped_labels": wlabels, "warped_res": wres,
                "warped_img": x[B:], "valid_mask": valid_mask, "warped_valid_mask": warped_mask, "semi": semi[:B], "semi_warp": semi[B:],
                "coarse_desc": desc[:B], "coarse_desc_warp": desc[B:], "flag": flag, "grad_semi": g_semi, "grad_semi_warp": g_semi_w,
                "grad_desc": g_a, "grad_desc_warp": g_b}

    # ------------------------------------------------------------------ the SuperGlue match loss and its gradient (include/imx_train.h)
    def ot_match_loss_grad(self, scores, bin_score, all_matches, n_all, iters, n0=None, n1=None, gout=None, want_grad=True):
        """The objective of superglue/models/superglue_train.py:271-299 on a score matrix, with its derivative through the unrolled
        Sinkhorn: scores (B,N0,N1) fp32, bin_score a one-element fp32 device tensor (or a number), all_matches (B,2,L) int64 and n_all (B)
        int32 as gt_matches writes them, n0 / n1 (B) int32 counts or None = all, gout (B) upstream cotangents or None = 1.  Returns
        dict: loss (B), flag (B) int32 (bit 0: a listed index outside the coupling matrix) and, unless want_grad is False, grad_scores
        (B,N0,N1) (0 past the counts) and grad_bin (B).  No host synchronisation."""
        a = self._ot_args("ot_match_loss_grad", scores, bin_score, all_matches, n_all, n0, n1, gout, want_grad)
        res = a["res"]
        self._check(self.train.imx_ot_match_loss_grad(self.handle, a["B"], _ptr(a["scores"]), a["N0"], a["N1"], _ptr(a["n0"]), _ptr(a["n1"]),
                                                    _ptr(a["bin_score"]), int(iters), _ptr(a["all_matches"]), _ptr(a["n_all"]), a["L"],
                                                    _ptr(a["gout"]), _ptr(res["loss"]), _ptr(res.get("grad_scores")), _ptr(res.get("grad_bin")),
                                                    _ptr(res["flag"]), _stream(self.device)))
        return res

    def _ot_args(self, who, scores, bin_score, all_matches, n_all, n0, n1, gout, want_grad):
        """the checked, device-resident arguments of ot_match_loss_grad and of ot_match_loss_grad_matches, and the output dict"""
        dev = self.device
        if scores.dim() != 3:
            raise ImxError(f"{who}: scores must be (B,N0,N1), got {tuple(scores.shape)}")
        B, N0, N1 = (int(v) for v in scores.shape)
        scores = self._f32(scores, (B, N0, N1), f"{who}: scores")
        if not isinstance(bin_score, torch.Tensor):
            bin_score = torch.full((1,), float(bin_score), dtype=torch.float32, device=dev)
        if bin_score.numel() != 1:
            raise ImxError(f"{who}: bin_score must hold one element, got {tuple(bin_score.shape)}")
        bin_score = bin_score.detach().to(dev, torch.float32).reshape(1).contiguous()
        all_matches = all_matches.to(dev, torch.int64).contiguous()
        if all_matches.dim() != 3 or all_matches.shape[0] != B or all_matches.shape[1] != 2:
            raise ImxError(f"{who}: all_matches must be (B,2,L) with B = {B}, got {tuple(all_matches.shape)}")
        Lc = int(all_matches.shape[2])
        n_all = self._counts(n_all, B, f"{who}: n_all")
        n0, n1 = self._counts(n0, B, f"{who}: n0"), self._counts(n1, B, f"{who}: n1")
        if n_all is None:
            raise ImxError(f"{who}: n_all is required")
        if gout is not None:
            gout = gout.to(dev, torch.float32).contiguous()
            if gout.numel() != B:
                raise ImxError(f"{who}: {gout.numel()} cotangents for a batch of {B}")
        res = {"loss": torch.empty(B, dtype=torch.float32, device=dev), "flag": torch.empty(B, dtype=torch.int32, device=dev)}
        if want_grad:
            res["grad_scores"] = torch.empty(B, N0, N1, dtype=torch.float32, device=dev)
            res["grad_bin"] = torch.empty(B, dtype=torch.float32, device=dev)
        return {"B": B, "N0": N0, "N1": N1, "L": Lc, "scores": scores, "bin_score": bin_score, "all_matches": all_matches, "n_all": n_all,
                "n0": n0, "n1": n1, "gout": gout, "res": res}

    # ------------------------------------------------------------------ the matches of the training forward (include/imx_sgloop.h)
    def _match_outputs(self, who, B, N0, N1, gt0, res):
        """matches0/1 (int64), matching_scores0/1 (fp32) and, with gt0 (B,N0) int64, stats (B,3) int32, added to res; returns gt0 on the device"""
        dev = self.device
        res.update({"matches0": torch.empty(B, N0, dtype=torch.int64, device=dev), "matches1": torch.empty(B, N1, dtype=torch.int64, device=dev),
                    "matching_scores0": torch.empty(B, N0, dtype=torch.float32, device=dev),
                    "matching_scores1": torch.empty(B, N1, dtype=torch.float32, device=dev)})
        if gt0 is None:
            return None
        gt0 = gt0.to(dev, torch.int64).contiguous()
        if tuple(gt0.shape) != (B, N0):
            raise ImxError(f"{who}: gt0 must be (B,N0) = ({B},{N0}), got {tuple(gt0.shape)}")
        res["stats"] = torch.empty(B, 3, dtype=torch.int32, device=dev)
        return gt0

    @staticmethod
    def _threshold(who, threshold):
        threshold = float(threshold)
        if math.isnan(threshold):
            raise ImxError(f"{who}: threshold is NaN")
        return threshold

    def assignment_matches(self, scores, u=None, v=None, threshold=0.2, n0=None, n1=None, gt0=None):
        """The extraction of superglue/models/superglue_train.py:276-286 from scores (B,N0,N1) fp32 and the final potentials u (B,N0+1), v
        (B,N1+1) of the log-domain Sinkhorn (None = zeros): Z = ((scores + u) + v) - norm element by element, never stored.  n0 / n1 (B)
        int32 counts or None = all, gt0 (B,N0) int64 or None.  Returns dict: matches0 (B,N0), matches1 (B,N1) int64 (-1 = none, and past
        the counts), matching_scores0/1 fp32 (0 past the counts) and, with gt0, stats (B,3) int32 = [gt0 >= 0, matches0 > -1, matches0 ==
        gt0 >= 0] over the valid rows.  Among equal values the lowest index wins.  No host synchronisation."""
        who = "assignment_matches"
        if scores.dim() != 3:
            raise ImxError(f"{who}: scores must be (B,N0,N1), got {tuple(scores.shape)}")
        B, N0, N1 = (int(s) for s in scores.shape)
        scores = self._f32(scores, (B, N0, N1), f"{who}: scores")
        u = None if u is None else self._f32(u, (B, N0 + 1), f"{who}: u")
        v = None if v is None else self._f32(v, (B, N1 + 1), f"{who}: v")
        n0, n1 = self._counts(n0, B, f"{who}: n0"), self._counts(n1, B, f"{who}: n1")
        threshold = self._threshold(who, threshold)
        res = {}
        gt0 = self._match_outputs(who, B, N0, N1, gt0, res)
        self._check(self.sgloop.imx_assignment_matches(self.handle, B, _ptr(scores), N0, N1, _ptr(n0), _ptr(n1), _ptr(u), _ptr(v), threshold,
                                                       _ptr(gt0), _ptr(res["matches0"]), _ptr(res["matches1"]), _ptr(res["matching_scores0"]),
                                                       _ptr(res["matching_scores1"]), _ptr(res.get("stats")), _stream(self.device)))
        return res

    def ot_match_loss_grad_matches(self, scores, bin_score, all_matches, n_all, iters, n0=None, n1=None, gout=None, want_grad=True, threshold=0.2,
                                   gt0=None):
        """ot_match_loss_grad and assignment_matches on the potentials of that very Sinkhorn, one call: the arguments of ot_match_loss_grad
        plus threshold and gt0.  Returns its dict -- loss, flag, grad_scores and grad_bin with the same bits -- plus matches0/1,
        matching_scores0/1 and, with gt0, stats.  No host synchronisation."""
        who = "ot_match_loss_grad_matches"
        a = self._ot_args(who, scores, bin_score, all_matches, n_all, n0, n1, gout, want_grad)
        res = a["res"]
        threshold = self._threshold(who, threshold)
        gt0 = self._match_outputs(who, a["B"], a["N0"], a["N1"], gt0, res)
        self._check(self.sgloop.imx_ot_match_loss_grad_matches(
            self.handle, a["B"], _ptr(a["scores"]), a["N0"], a["N1"], _ptr(a["n0"]), _ptr(a["n1"]), _ptr(a["bin_score"]), int(iters),
            _ptr(a["all_matches"]), _ptr(a["n_all"]), a["L"], _ptr(a["gout"]), _ptr(res["loss"]), _ptr(res.get("grad_scores")),
            _ptr(res.get("grad_bin")), _ptr(res["flag"]), threshold, _ptr(gt0), _ptr(res["matches0"]), _ptr(res["matches1"]),
            _ptr(res["matching_scores0"]), _ptr(res["matching_scores1"]), _ptr(res.get("stats")), _stream(self.device)))
        return res

    # ------------------------------------------------------------------ the GNN's attention, training form (include/imx_train.h)
    def _mha_shapes(self, who, q, k, v):
        """(B, D, H, N, M) of q (B,D,H,N) and k, v (B,D,H,M), the reference's view(B, dim, heads, -1)"""
        if q.dim() != 4 or k.dim() != 4:
            raise ImxError(f"{who}: q and k must be (B,D,H,N) and (B,D,H,M), got {tuple(q.shape)} and {tuple(k.shape)}")
        B, D, H, N = (int(s) for s in q.shape)
        M = int(k.shape[3])
        if tuple(k.shape) != (B, D, H, M) or tuple(v.shape) != (B, D, H, M):
            raise ImxError(f"{who}: k and v must be ({B},{D},{H},M), got {tuple(k.shape)} and {tuple(v.shape)}")
        return B, D, H, N, M

    def mha_forward_train(self, q, k, v, nq=None, nk=None, want_lse=True):
        """attention() of superglue/models/superglue_train.py:82-86 in its training form: q (B,D,H,N), k and v (B,D,H,M) fp32 in the
        reference's own layout, nq / nk (B) int32 counts or None = all.  Returns dict: out (B,D,H,N) = softmax(q^T k / sqrt(D)) v (0 on
        queries past nq) and, unless want_lse is False, lse (B,H,N), the row log-sum-exp the backward recomputes the probabilities from.
        No (N, M) matrix is stored.  No host synchronisation."""
        dev = self.device
        B, D, H, N, M = self._mha_shapes("mha_forward_train", q, k, v)
        q, k, v = (self._f32(t, s, f"mha_forward_train: {n}") for t, s, n in ((q, (B, D, H, N), "q"), (k, (B, D, H, M), "k"), (v, (B, D, H, M), "v")))
        nq, nk = self._counts(nq, B, "mha_forward_train: nq"), self._counts(nk, B, "mha_forward_train: nk")
        res = {"out": torch.empty(B, D, H, N, dtype=torch.float32, device=dev)}
        if want_lse:
            res["lse"] = torch.empty(B, H, N, dtype=torch.float32, device=dev)
        self._check(self.train.imx_mha_forward_train(self.handle, B, H, D, N, M, _ptr(q), _ptr(k), _ptr(v), _ptr(nq), _ptr(nk),
                                                   _ptr(res["out"]), _ptr(res.get("lse")), _stream(dev)))
        return res

    def mha_backward(self, q, k, v, out, lse, dout, nq=None, nk=None, want=(True, True, True)):
        """The backward of mha_forward_train from dout (B,D,H,N), with the forward's q, k, v, out and lse: the probabilities are
        recomputed tile by tile from lse.  Returns dict with dq (B,D,H,N), dk and dv (B,D,H,M) (0 past the counts), each only where
        `want` = (dq, dk, dv) asks for it; a gradient's bits do not depend on which others are formed.  No host synchronisation."""
        dev = self.device
        B, D, H, N, M = self._mha_shapes("mha_backward", q, k, v)
        q, k, v = (self._f32(t, s, f"mha_backward: {n}") for t, s, n in ((q, (B, D, H, N), "q"), (k, (B, D, H, M), "k"), (v, (B, D, H, M), "v")))
        out, dout = self._f32(out, (B, D, H, N), "mha_backward: out"), self._f32(dout, (B, D, H, N), "mha_backward: dout")
        lse = self._f32(lse, (B, H, N), "mha_backward: lse")
        nq, nk = self._counts(nq, B, "mha_backward: nq"), self._counts(nk, B, "mha_backward: nk")
        if len(want) != 3:
            raise ImxError(f"mha_backward: want must be three flags (dq, dk, dv), got {want!r}")
        res = {}
        for name, w, n in (("dq", want[0], N), ("dk", want[1], M), ("dv", want[2], M)):
            if w:
                res[name] = torch.empty(B, D, H, n, dtype=torch.float32, device=dev)
        self._check(self.train.imx_mha_backward(self.handle, B, H, D, N, M, _ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(lse), _ptr(dout),
                                              _ptr(nq), _ptr(nk), _ptr(res.get("dq")), _ptr(res.get("dk")), _ptr(res.get("dv")), _stream(dev)))
        return res

    # ------------------------------------------------------------------ the 1x1 convolutions, training form (include/imx_train.h)
    def _conv1x1_args(self, who, x0, w, x1):
        """(B, Cout, C0, C1, N) of x0 (B,C0,N), x1 (B,C1,N) or None, w (Cout, C0+C1) or the (Cout, C0+C1, 1) parameter itself; every
        tensor a contiguous fp32 cuda tensor, otherwise ImxError (no silent copy)"""
        for t, what in ((x0, "x0"), (w, "w")) + (((x1, "x1"),) if x1 is not None else ()):
            if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.dtype != torch.float32 or not t.is_contiguous():
                raise ImxError(f"{who}: {what} must be a contiguous fp32 cuda tensor")
        if x0.dim() != 3 or (x1 is not None and (x1.dim() != 3 or x1.shape[0] != x0.shape[0] or x1.shape[2] != x0.shape[2])):
            raise ImxError(f"{who}: x0 and x1 must be (B,C0,N) and (B,C1,N), got {tuple(x0.shape)} and {None if x1 is None else tuple(x1.shape)}")
        B, C0, N = (int(s) for s in x0.shape)
        C1 = 0 if x1 is None else int(x1.shape[1])
        if w.dim() not in (2, 3) or int(w.shape[1]) != C0 + C1 or (w.dim() == 3 and int(w.shape[2]) != 1):
            raise ImxError(f"{who}: w must be (Cout,{C0 + C1}) or (Cout,{C0 + C1},1), got {tuple(w.shape)}")
        return B, int(w.shape[0]), C0, C1, N

    def conv1x1_forward_train(self, x0, w, bias=None, x1=None, n=None):
        """F.conv1d(torch.cat([x0, x1], 1), w, bias) of kernel size 1 without forming the concatenation: x0 (B,C0,N), x1 (B,C1,N) or None,
        w (Cout, C0+C1[, 1]), bias (Cout) or None, n (B) int32 counts or None = all.  Returns dict: y (B,Cout,N), 0 on columns past n.
        No host synchronisation."""
        dev = self.device
        B, Cout, C0, C1, N = self._conv1x1_args("conv1x1_forward_train", x0, w, x1)
        if bias is not None:
            bias = self._f32(bias, (Cout,), "conv1x1_forward_train: bias")
        n = self._counts(n, B, "conv1x1_forward_train: n")
        res = {"y": torch.empty(B, Cout, N, dtype=torch.float32, device=dev)}
        self._check(self.train.imx_conv1x1_forward_train(self.handle, B, Cout, C0, C1, N, _ptr(x0), _ptr(x1), _ptr(w), _ptr(bias), _ptr(n),
                                                        _ptr(res["y"]), _stream(dev)))
        return res

    def conv1x1_backward(self, x0, w, dy, x1=None, n=None, want=(True, True, True, True)):
        """The backward of conv1x1_forward_train from dy (B,Cout,N).  Returns dict with dx0 (B,C0,N), dx1 (B,C1,N) (0 past the counts),
        dw (the shape of w) and db (Cout) (overwritten, not accumulated), each only where `want` = (dx0, dx1, dw, db) asks for it;
        want[1] is ignored without x1.  A gradient's bits do not depend on which others are formed.  No host synchronisation."""
        dev = self.device
        B, Cout, C0, C1, N = self._conv1x1_args("conv1x1_backward", x0, w, x1)
        if not isinstance(dy, torch.Tensor) or dy.device.type != "cuda" or dy.dtype != torch.float32 or not dy.is_contiguous():
            raise ImxError("conv1x1_backward: dy must be a contiguous fp32 cuda tensor")
        if tuple(dy.shape) != (B, Cout, N):
            raise ImxError(f"conv1x1_backward: dy must be ({B},{Cout},{N}), got {tuple(dy.shape)}")
        n = self._counts(n, B, "conv1x1_backward: n")
        if len(want) != 4:
            raise ImxError(f"conv1x1_backward: want must be four flags (dx0, dx1, dw, db), got {want!r}")
        res = {}
        for name, wanted, shape in (("dx0", want[0], (B, C0, N)), ("dx1", want[1] and x1 is not None, (B, C1, N)),
                                    ("dw", want[2], tuple(w.shape)), ("db", want[3], (Cout,))):
            if wanted:
                res[name] = torch.empty(shape, dtype=torch.float32, device=dev)
        self._check(self.train.imx_conv1x1_backward(self.handle, B, Cout, C0, C1, N, _ptr(x0), _ptr(x1), _ptr(w), _ptr(dy), _ptr(n),
                                                   _ptr(res.get("dx0")), _ptr(res.get("dx1")), _ptr(res.get("dw")), _ptr(res.get("db")),
                                                   _stream(dev)))
        return res

    # ------------------------------------------------------------------ BatchNorm1d + ReLU, training form (include/imx_train.h)
    def _bn_args(self, who, x, per_channel, full=()):
        """(B, C, N) of x (B,C,N); per_channel: (tensor or None, name) of shape (C), full: (tensor, name) of x's shape; every tensor a
        contiguous fp32 cuda tensor, otherwise ImxError (no silent copy)"""
        for t, what in (((x, "x"),) + tuple(full) + tuple(p for p in per_channel if p[0] is not None)):
            if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.dtype != torch.float32 or not t.is_contiguous():
                raise ImxError(f"{who}: {what} must be a contiguous fp32 cuda tensor")
        if x.dim() != 3:
            raise ImxError(f"{who}: x must be (B,C,N), got {tuple(x.shape)}")
        B, C, N = (int(s) for s in x.shape)
        for t, what in full:
            if tuple(t.shape) != (B, C, N):
                raise ImxError(f"{who}: {what} must be ({B},{C},{N}), got {tuple(t.shape)}")
        for t, what in per_channel:
            if t is not None and tuple(t.shape) != (C,):
                raise ImxError(f"{who}: {what} must be ({C},), got {tuple(t.shape)}")
        return B, C, N

    def bn_relu_forward_train(self, x, gamma, beta, running_mean=None, running_var=None, num_batches_tracked=None, n=None, training=True,
                              momentum=0.1, eps=1e-5):
        """F.relu(F.batch_norm(x, running_mean, running_var, gamma, beta, training, momentum, eps)) on x (B,C,N) in one launch; n (B) int32
        counts or None = all: the statistics are those of the valid columns of all pairs.  In training mode running_mean / running_var (C)
        and num_batches_tracked (one int64) are updated in place where given; in evaluation mode the running statistics are required.
        Returns dict: y (B,C,N) (0 past the counts), mean and rstd (C), what bn_relu_backward needs beside x.  No host synchronisation."""
        dev = self.device
        B, C, N = self._bn_args("bn_relu_forward_train", x, ((gamma, "gamma"), (beta, "beta"), (running_mean, "running_mean"),
                                                             (running_var, "running_var")))
        if num_batches_tracked is not None and (not isinstance(num_batches_tracked, torch.Tensor) or num_batches_tracked.device.type != "cuda"
                                                or num_batches_tracked.dtype != torch.int64 or num_batches_tracked.numel() != 1):
            raise ImxError("bn_relu_forward_train: num_batches_tracked must be a cuda int64 tensor of one element")
        n = self._counts(n, B, "bn_relu_forward_train: n")
        res = {"y": torch.empty(B, C, N, dtype=torch.float32, device=dev), "mean": torch.empty(C, dtype=torch.float32, device=dev),
               "rstd": torch.empty(C, dtype=torch.float32, device=dev)}
        self._check(self.train.imx_bn_relu_forward_train(self.handle, B, C, N, 1 if training else 0, float(eps), float(momentum), _ptr(x), _ptr(gamma),
                                                       _ptr(beta), _ptr(n), _ptr(running_mean), _ptr(running_var), _ptr(num_batches_tracked),
                                                       _ptr(res["y"]), _ptr(res["mean"]), _ptr(res["rstd"]), _stream(dev)))
        return res

    def bn_relu_backward(self, x, gamma, beta, mean, rstd, dy, n=None, training=True, want=(True, True, True)):
        """The backward of bn_relu_forward_train from dy (B,C,N), with the forward's x, mean and rstd: the ReLU mask is recomputed, y is not
        an input.  Returns dict with dx (B,C,N) (0 past the counts), dgamma and dbeta (C) (overwritten, not accumulated), each only where
        `want` = (dx, dgamma, dbeta) asks for it; a gradient's bits do not depend on which others are formed.  No host synchronisation."""
        dev = self.device
        B, C, N = self._bn_args("bn_relu_backward", x, ((gamma, "gamma"), (beta, "beta"), (mean, "mean"), (rstd, "rstd")), ((dy, "dy"),))
        if mean is None or rstd is None:
            raise ImxError("bn_relu_backward: mean and rstd are required")
        n = self._counts(n, B, "bn_relu_backward: n")
        if len(want) != 3:
            raise ImxError(f"bn_relu_backward: want must be three flags (dx, dgamma, dbeta), got {want!r}")
        res = {}
        for name, wanted, shape in (("dx", want[0], (B, C, N)), ("dgamma", want[1], (C,)), ("dbeta", want[2], (C,))):
            if wanted:
                res[name] = torch.empty(shape, dtype=torch.float32, device=dev)
        self._check(self.train.imx_bn_relu_backward(self.handle, B, C, N, 1 if training else 0, _ptr(x), _ptr(gamma), _ptr(beta), _ptr(mean),
                                                  _ptr(rstd), _ptr(dy), _ptr(n), _ptr(res.get("dx")), _ptr(res.get("dgamma")),
                                                  _ptr(res.get("dbeta")), _stream(dev)))
        return res

    # ------------------------------------------------------------------ the score product, training form (include/imx_sgtrain.h)
    def _score_args(self, who, a, b, scale, dscores=None):
        """(B, D, N0, N1, scale) of a (B,D,N0) and b (B,D,N1); every tensor a contiguous fp32 cuda tensor, otherwise ImxError (no silent
        copy); scale None = D ** -0.5"""
        for t, what in ((a, "a"), (b, "b")) + (((dscores, "dscores"),) if dscores is not None else ()):
            if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.dtype != torch.float32 or not t.is_contiguous():
                raise ImxError(f"{who}: {what} must be a contiguous fp32 cuda tensor")
        if a.dim() != 3 or b.dim() != 3 or a.shape[0] != b.shape[0] or a.shape[1] != b.shape[1]:
            raise ImxError(f"{who}: a and b must be (B,D,N0) and (B,D,N1), got {tuple(a.shape)} and {tuple(b.shape)}")
        B, D, N0 = (int(s) for s in a.shape)
        N1 = int(b.shape[2])
        if dscores is not None and tuple(dscores.shape) != (B, N0, N1):
            raise ImxError(f"{who}: dscores must be ({B},{N0},{N1}), got {tuple(dscores.shape)}")
        return B, D, N0, N1, float(D) ** -0.5 if scale is None else float(scale)

    def score_product_forward_train(self, a, b, n0=None, n1=None, scale=None):
        """torch.einsum('bdn,bdm->bnm', a, b) * scale (superglue/models/superglue_train.py:267-268): a (B,D,N0), b (B,D,N1), n0 / n1 (B)
        int32 counts or None = all, scale None = D ** -0.5, the reference's.  Returns dict: scores (B,N0,N1), 0 on rows past n0 and
        columns past n1.  No host synchronisation."""
        dev = self.device
        B, D, N0, N1, scale = self._score_args("score_product_forward_train", a, b, scale)
        n0, n1 = self._counts(n0, B, "score_product_forward_train: n0"), self._counts(n1, B, "score_product_forward_train: n1")
        res = {"scores": torch.empty(B, N0, N1, dtype=torch.float32, device=dev)}
        self._check(self.sgtrain.imx_score_product_forward_train(self.handle, B, D, N0, N1, _ptr(a), _ptr(b), _ptr(n0), _ptr(n1), scale,
                                                                 _ptr(res["scores"]), _stream(dev)))
        return res

    def score_product_backward(self, a, b, dscores, n0=None, n1=None, scale=None, want=(True, True)):
        """The backward of score_product_forward_train from dscores (B,N0,N1).  Returns dict with da (B,D,N0) and db (B,D,N1) (0 past the
        counts), each only where `want` = (da, db) asks for it; a gradient's bits do not depend on whether the other is formed.  No host
        synchronisation."""
        dev = self.device
        B, D, N0, N1, scale = self._score_args("score_product_backward", a, b, scale, dscores)
        n0, n1 = self._counts(n0, B, "score_product_backward: n0"), self._counts(n1, B, "score_product_backward: n1")
        if len(want) != 2:
            raise ImxError(f"score_product_backward: want must be two flags (da, db), got {want!r}")
        res = {}
        for name, wanted, shape in (("da", want[0], (B, D, N0)), ("db", want[1], (B, D, N1))):
            if wanted:
                res[name] = torch.empty(shape, dtype=torch.float32, device=dev)
        self._check(self.sgtrain.imx_score_product_backward(self.handle, B, D, N0, N1, _ptr(a), _ptr(b), _ptr(dscores), _ptr(n0), _ptr(n1), scale,
                                                            _ptr(res.get("da")), _ptr(res.get("db")), _stream(dev)))
        return res

    # ------------------------------------------------------------------ the 3x3 convolutions, training form (include/imx_spnet.h)
    def _conv3x3_args(self, who, x, w, dy=None):
        """(B, Cout, Cin, H, W) of x (B,Cin,H,W), w (Cout,Cin,3,3) and dy (B,Cout,H,W) or None; every tensor a contiguous fp32 cuda tensor,
        otherwise ImxError (no silent copy)"""
        for t, what in ((x, "x"), (w, "w")) + (((dy, "dy"),) if dy is not None else ()):
            if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.dtype != torch.float32 or not t.is_contiguous():
                raise ImxError(f"{who}: {what} must be a contiguous fp32 cuda tensor")
        if x.dim() != 4:
            raise ImxError(f"{who}: x must be (B,Cin,H,W), got {tuple(x.shape)}")
        B, Cin, H, W = (int(s) for s in x.shape)
        if w.dim() != 4 or tuple(w.shape[1:]) != (Cin, 3, 3):
            raise ImxError(f"{who}: w must be (Cout,{Cin},3,3), got {tuple(w.shape)}")
        Cout = int(w.shape[0])
        if dy is not None and tuple(dy.shape) != (B, Cout, H, W):
            raise ImxError(f"{who}: dy must be ({B},{Cout},{H},{W}), got {tuple(dy.shape)}")
        return B, Cout, Cin, H, W

    def conv3x3_forward_train(self, x, w, bias=None):
        """F.conv2d(x, w, bias, padding=1) for a 3x3 weight: x (B,Cin,H,W), w (Cout,Cin,3,3), bias (Cout) or None, NCHW in place.  Returns
        dict: y (B,Cout,H,W).  No host synchronisation."""
        dev = self.device
        B, Cout, Cin, H, W = self._conv3x3_args("conv3x3_forward_train", x, w)
        if bias is not None:
            bias = self._f32(bias, (Cout,), "conv3x3_forward_train: bias")
        res = {"y": torch.empty(B, Cout, H, W, dtype=torch.float32, device=dev)}
        self._check(self.spnet.imx_conv3x3_forward_train(self.handle, B, Cout, Cin, H, W, _ptr(x), _ptr(w), _ptr(bias), _ptr(res["y"]),
                                                        _stream(dev)))
        return res

    def conv3x3_backward(self, x, w, dy, want=(True, True, True)):
        """The backward of conv3x3_forward_train from dy (B,Cout,H,W).  Returns dict with dx (B,Cin,H,W), dw (Cout,Cin,3,3) and db (Cout)
        (overwritten, not accumulated), each only where `want` = (dx, dw, db) asks for it.  A gradient's bits do not depend on which others
        are formed.  No host synchronisation."""
        dev = self.device
        B, Cout, Cin, H, W = self._conv3x3_args("conv3x3_backward", x, w, dy)
        if len(want) != 3:
            raise ImxError(f"conv3x3_backward: want must be three flags (dx, dw, db), got {want!r}")
        res = {}
        for name, wanted, shape in (("dx", want[0], (B, Cin, H, W)), ("dw", want[1], (Cout, Cin, 3, 3)), ("db", want[2], (Cout,))):
            if wanted:
                res[name] = torch.empty(shape, dtype=torch.float32, device=dev)
        self._check(self.spnet.imx_conv3x3_backward(self.handle, B, Cout, Cin, H, W, _ptr(x), _ptr(w), _ptr(dy), _ptr(res.get("dx")),
                                                   _ptr(res.get("dw")), _ptr(res.get("db")), _stream(dev)))
        return res

    # ------------------------------------------------------------------ BatchNorm2d [+ ReLU], training form (include/imx_spnorm.h)
    def _bn2d_args(self, who, x, per_channel, dy=None):
        """(B, C, HW) of x (B,C,H,W); per_channel: (tensor or None, name) of shape (C); dy of x's shape or None; every tensor a contiguous
        fp32 cuda tensor, otherwise ImxError (no silent copy)"""
        for t, what in ((x, "x"),) + (((dy, "dy"),) if dy is not None else ()) + tuple(p for p in per_channel if p[0] is not None):
            if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.dtype != torch.float32 or not t.is_contiguous():
                raise ImxError(f"{who}: {what} must be a contiguous fp32 cuda tensor")
        if x.dim() != 4:
            raise ImxError(f"{who}: x must be (B,C,H,W), got {tuple(x.shape)}")
        B, C, H, W = (int(s) for s in x.shape)
        if dy is not None and tuple(dy.shape) != (B, C, H, W):
            raise ImxError(f"{who}: dy must be ({B},{C},{H},{W}), got {tuple(dy.shape)}")
        for t, what in per_channel:
            if t is not None and tuple(t.shape) != (C,):
                raise ImxError(f"{who}: {what} must be ({C},), got {tuple(t.shape)}")
        return B, C, H * W

    def bn2d_forward_train(self, x, gamma, beta, running_mean=None, running_var=None, num_batches_tracked=None, relu=True, training=True,
                           momentum=0.1, eps=1e-5):
        """F.batch_norm(x, running_mean, running_var, gamma, beta, training, momentum, eps) on x (B,C,H,W), NCHW in place, followed by F.relu
        when `relu`.  In training mode running_mean / running_var (C) and num_batches_tracked (one int64) are updated in place where given;
        in evaluation mode the running statistics are required.  Returns dict: y (B,C,H,W), mean and rstd (C), what bn2d_backward needs
        beside x.  No host synchronisation."""
        dev = self.device
        B, C, HW = self._bn2d_args("bn2d_forward_train", x, ((gamma, "gamma"), (beta, "beta"), (running_mean, "running_mean"),
                                                             (running_var, "running_var")))
        if gamma is None or beta is None:
            raise ImxError("bn2d_forward_train: gamma and beta are required")
        if num_batches_tracked is not None and (not isinstance(num_batches_tracked, torch.Tensor) or num_batches_tracked.device.type != "cuda"
                                                or num_batches_tracked.dtype != torch.int64 or num_batches_tracked.numel() != 1):
            raise ImxError("bn2d_forward_train: num_batches_tracked must be a cuda int64 tensor of one element")
        res = {"y": torch.empty_like(x), "mean": torch.empty(C, dtype=torch.float32, device=dev),
               "rstd": torch.empty(C, dtype=torch.float32, device=dev)}
        self._check(self.spnorm.imx_bn2d_forward_train(self.handle, B, C, HW, 1 if relu else 0, 1 if training else 0, float(eps), float(momentum),
                                                       _ptr(x), _ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var),
                                                       _ptr(num_batches_tracked), _ptr(res["y"]), _ptr(res["mean"]), _ptr(res["rstd"]),
                                                       _stream(dev)))
        return res

    def bn2d_backward(self, x, gamma, beta, mean, rstd, dy, relu=True, training=True, want=(True, True, True)):
        """The backward of bn2d_forward_train from dy (B,C,H,W), with the forward's x, mean and rstd: the ReLU mask is recomputed, y is not
        an input.  Returns dict with dx (B,C,H,W), dgamma and dbeta (C) (overwritten, not accumulated), each only where `want` = (dx,
        dgamma, dbeta) asks for it; a gradient's bits do not depend on which others are formed.  No host synchronisation."""
        dev = self.device
        B, C, HW = self._bn2d_args("bn2d_backward", x, ((gamma, "gamma"), (beta, "beta"), (mean, "mean"), (rstd, "rstd")), dy)
        if gamma is None or beta is None or mean is None or rstd is None or dy is None:
            raise ImxError("bn2d_backward: gamma, beta, mean, rstd and dy are required")
        if len(want) != 3:
            raise ImxError(f"bn2d_backward: want must be three flags (dx, dgamma, dbeta), got {want!r}")
        res = {}
        for name, wanted, shape in (("dx", want[0], tuple(x.shape)), ("dgamma", want[1], (C,)), ("dbeta", want[2], (C,))):
            if wanted:
                res[name] = torch.empty(shape, dtype=torch.float32, device=dev)
        self._check(self.spnorm.imx_bn2d_backward(self.handle, B, C, HW, 1 if relu else 0, 1 if training else 0, _ptr(x), _ptr(gamma), _ptr(beta),
                                                  _ptr(mean), _ptr(rstd), _ptr(dy), _ptr(res.get("dx")), _ptr(res.get("dgamma")),
                                                  _ptr(res.get("dbeta")), _stream(dev)))
        return res

    # ------------------------------------------------------------------ MaxPool2d(2) and desc / ||desc||_2, training form (include/imx_sppool.h)
    @staticmethod
    def _sppool_tensor(who, t, what, dtype=torch.float32):
        """t is a contiguous cuda tensor of `dtype`, otherwise ImxError (no silent copy)"""
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.dtype != dtype or not t.is_contiguous():
            raise ImxError(f"{who}: {what} must be a contiguous {str(dtype).replace('torch.', '')} cuda tensor")

    def maxpool2_forward_train(self, x, want_idx=True):
        """F.max_pool2d(x, 2) on x (B,C,H,W), NCHW in place: kernel 2, stride 2, no padding, floor.  Returns dict: y (B,C,H//2,W//2) and
        idx, a torch.uint8 tensor of y's shape holding 2 row + col of each window's maximum (PyTorch's tie and NaN rule), what
        maxpool2_backward needs; idx is None with want_idx=False (evaluation), y has the same bits.  No host synchronisation."""
        who = "maxpool2_forward_train"
        self._sppool_tensor(who, x, "x")
        if x.dim() != 4:
            raise ImxError(f"{who}: x must be (B,C,H,W), got {tuple(x.shape)}")
        B, C, H, W = (int(s) for s in x.shape)
        y = torch.empty((B, C, H // 2, W // 2), dtype=torch.float32, device=x.device)
        idx = torch.empty((B, C, H // 2, W // 2), dtype=torch.uint8, device=x.device) if want_idx else None
        self._check(self.sppool.imx_maxpool2_forward_train(self.handle, B, C, H, W, _ptr(x), _ptr(y), _ptr(idx), _stream(self.device)))
        return {"y": y, "idx": idx}

    def maxpool2_backward(self, idx, dy, shape):
        """The backward of maxpool2_forward_train for an input of `shape` = (B,C,H,W): dx holds dy (B,C,H//2,W//2) at the element idx
        recorded for each window and +0 everywhere else, written in full.  Returns dict: dx.  No host synchronisation."""
        who = "maxpool2_backward"
        self._sppool_tensor(who, idx, "idx", torch.uint8)
        self._sppool_tensor(who, dy, "dy")
        if len(shape) != 4:
            raise ImxError(f"{who}: shape must be (B,C,H,W), got {tuple(shape)}")
        B, C, H, W = (int(s) for s in shape)
        for t, what in ((idx, "idx"), (dy, "dy")):
            if tuple(t.shape) != (B, C, H // 2, W // 2):
                raise ImxError(f"{who}: {what} must be ({B},{C},{H // 2},{W // 2}), got {tuple(t.shape)}")
        dx = torch.empty((B, C, H, W), dtype=torch.float32, device=dy.device)
        self._check(self.sppool.imx_maxpool2_backward(self.handle, B, C, H, W, _ptr(idx), _ptr(dy), _ptr(dx), _stream(self.device)))
        return {"dx": dx}

    def l2norm_forward_train(self, x):
        """x / torch.norm(x, p=2, dim=1, keepdim=True) on x (B,C,H,W) or (B,C,N): a true division, no epsilon (a zero vector gives NaN
        in its own pixel).  Returns dict: y of x's shape and norm (B,H,W) or (B,N), what l2norm_backward needs.  No host synchronisation."""
        who = "l2norm_forward_train"
        self._sppool_tensor(who, x, "x")
        if x.dim() not in (3, 4):
            raise ImxError(f"{who}: x must be (B,C,H,W) or (B,C,N), got {tuple(x.shape)}")
        B, C = int(x.shape[0]), int(x.shape[1])
        HW = x.numel() // max(B * C, 1)
        res = {"y": torch.empty_like(x), "norm": torch.empty((B,) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)}
        self._check(self.sppool.imx_l2norm_forward_train(self.handle, B, C, HW, _ptr(x), _ptr(res["y"]), _ptr(res["norm"]), _stream(self.device)))
        return res

    def l2norm_backward(self, y, norm, dy):
        """The backward of l2norm_forward_train from dy of y's shape, with the forward's y and norm: dx = (dy - y sum_c(y dy)) / norm.
        Returns dict: dx.  No host synchronisation."""
        who = "l2norm_backward"
        for t, what in ((y, "y"), (norm, "norm"), (dy, "dy")):
            self._sppool_tensor(who, t, what)
        if y.dim() not in (3, 4):
            raise ImxError(f"{who}: y must be (B,C,H,W) or (B,C,N), got {tuple(y.shape)}")
        if dy.shape != y.shape or tuple(norm.shape) != (int(y.shape[0]),) + tuple(y.shape[2:]):
            raise ImxError(f"{who}: dy must be {tuple(y.shape)} and norm {(int(y.shape[0]),) + tuple(y.shape[2:])}, got {tuple(dy.shape)} and {tuple(norm.shape)}")
        B, C = int(y.shape[0]), int(y.shape[1])
        HW = y.numel() // max(B * C, 1)
        dx = torch.empty_like(y)
        self._check(self.sppool.imx_l2norm_backward(self.handle, B, C, HW, _ptr(y), _ptr(norm), _ptr(dy), _ptr(dx), _stream(self.device)))
        return {"dx": dx}

    # ------------------------------------------------------------------ photometric augmentation (include/imx_photo.h)
    def _photo_tensor(self, who, t, what, dtype, shape):
        """t is a contiguous cuda tensor of `dtype` and `shape`, otherwise ImxError (no silent copy)"""
        self._sppool_tensor(who, t, what, dtype)
        if tuple(t.shape) != tuple(shape):
            raise ImxError(f"{who}: {what} must be {tuple(shape)}, got {tuple(t.shape)}")

    def photo_pixels(self, images, lut, noise_scale, thresh, table, blur_kernel, blur_on, key):
        """imx_photo_pixels on images (B,H,W) float32 in [0,1]: the per-image table lut (B,256) uint8, Gaussian noise of noise_scale (B),
        impulse noise below thresh (B) from table (256) uint8, the 3x3 correlation blur_kernel (B,9) where blur_on (B) is set; per-pixel
        draws from Philox4x32-10 under key (B,2).  thresh, blur_on and key are int32 tensors (key and thresh hold uint32 bit patterns).
        Returns (B,H,W) uint8.  No host synchronisation."""
        who = "photo_pixels"
        self._sppool_tensor(who, images, "images")
        if images.dim() != 3:
            raise ImxError(f"{who}: images must be (B,H,W), got {tuple(images.shape)}")
        B, H, W = (int(s) for s in images.shape)
        i32, u8, f32 = torch.int32, torch.uint8, torch.float32
        for t, what, dt, shape in ((lut, "lut", u8, (B, 256)), (noise_scale, "noise_scale", f32, (B,)), (thresh, "thresh", i32, (B,)),
                                   (table, "table", u8, (256,)), (blur_kernel, "blur_kernel", f32, (B, 9)), (blur_on, "blur_on", i32, (B,)),
                                   (key, "key", i32, (B, 2))):
            self._photo_tensor(who, t, what, dt, shape)
        out = torch.empty((B, H, W), dtype=u8, device=images.device)
        self._check(self.photo.imx_photo_pixels(self.handle, B, H, W, _ptr(images), _ptr(lut), _ptr(noise_scale), _ptr(thresh), _ptr(table),
                                                _ptr(blur_kernel), _ptr(blur_on), _ptr(key), _ptr(out), _stream(self.device)))
        return out

    def photo_shade(self, images_u8, ellipses, n_ellipses, taps, ksize, transparency, on):
        """imx_photo_shade on images_u8 (B,H,W) uint8: the union of ellipses (B,E,5) = (cx, cy, ax, ay, degrees), the first n_ellipses (B)
        int32 of each image, blurred with the Gaussian taps (B,Kcap) of which image b uses ksize[b] -- a HOST sequence of B odd
        integers in 3..Kcap, read during the call -- and applied with transparency (B); on (B) int32 clear leaves the image / 255.
        Returns (B,H,W) float32.  No host synchronisation."""
        who = "photo_shade"
        self._sppool_tensor(who, images_u8, "images_u8", torch.uint8)
        if images_u8.dim() != 3 or ellipses.dim() != 3 or taps.dim() != 2:
            raise ImxError(f"{who}: images_u8 must be (B,H,W), ellipses (B,E,5) and taps (B,Kcap)")
        B, H, W = (int(s) for s in images_u8.shape)
        E, Kcap = int(ellipses.shape[1]), int(taps.shape[1])
        i32, f32 = torch.int32, torch.float32
        for t, what, dt, shape in ((ellipses, "ellipses", f32, (B, E, 5)), (n_ellipses, "n_ellipses", i32, (B,)), (taps, "taps", f32, (B, Kcap)),
                                   (transparency, "transparency", f32, (B,)), (on, "on", i32, (B,))):
            self._photo_tensor(who, t, what, dt, shape)
        ks = np.ascontiguousarray(np.asarray(ksize, dtype=np.int32).reshape(-1))
        if ks.size != B:
            raise ImxError(f"{who}: ksize must hold {B} integers on the host, got {ks.size}")
        out = torch.empty((B, H, W), dtype=f32, device=images_u8.device)
        self._check(self.photo.imx_photo_shade(self.handle, B, H, W, E, Kcap, _ptr(images_u8), _ptr(ellipses), _ptr(n_ellipses), _ptr(taps),
                                               ks.ctypes.data_as(ctypes.c_void_p), _ptr(transparency), _ptr(on), _ptr(out), _stream(self.device)))
        return out

    def photometric(self, images, params):
        """The reference's imgPhotometric (datasets/ALLSS.py:116-128) for a batch: images (B,1,H,W) or (B,H,W) float32 in [0,1], params the
        dict of host arrays photometric.sample_params drew (one entry per image).  Both calls on the current stream; returns float32
        (B,1,H,W).  No host synchronisation."""
        who = "photometric"
        x = images[:, 0] if images.dim() == 4 else images
        self._sppool_tensor(who, x, "images")
        dev = x.device

        def up(name, as_i32=False):
            a = np.ascontiguousarray(params[name])
            return torch.from_numpy(a.view(np.int32) if as_i32 else a).to(dev)
        u8 = self.photo_pixels(x, up("lut"), up("noise_scale"), up("thresh", True), up("table"), up("blur_kernel"), up("blur_on"),
                               up("key", True))
        out = self.photo_shade(u8, up("ellipses"), up("n_ellipses"), up("taps"), params["ksize"], up("transparency"), up("shade_on"))
        return out[:, None]

    # ------------------------------------------------------------------ the training loop (include/imx_sploop.h)
    def warp_labels_bi(self, pts, counts, homographies, H, W, levels=0, pixel_space=False):
        """get_labels_bi (datasets/data_tools.py:9-34) as warpLabels(..., bilinear=True) calls it, for B images: pts (B,Kcap,2) (x, y),
        counts (B) int32 or None, homographies (B,3,3) on [-1,1]^2 coordinates (scaled to pixels here as warp_labels does).  levels = 0:
        the bilinear weights (`warped_labels_bi`); levels = 255: floor(255 w) / 255, the 8-bit round trip of ImgAugTransform.__call__
        (`warped_labels_gaussian` where the blur is the identity).  Returns (out (B,H,W), flag (1) int32 device word: bit 0 = a weight
        outside [0,1] (a warped coordinate in (-1,0)), bit 1 = a non-finite warped point, dropped).  Several entries on one pixel: the
        highest order index k count + i writes.  No host synchronisation."""
        who = "warp_labels_bi"
        pts = pts if isinstance(pts, torch.Tensor) else torch.as_tensor(np.asarray(pts, dtype=np.float32))
        pts = pts.to(self.device, torch.float32).contiguous()
        if pts.dim() != 3 or pts.shape[2] != 2:
            raise ImxError(f"{who}: pts must be (B,Kcap,2), got {tuple(pts.shape)}")
        if int(levels) not in (0, 255):
            raise ImxError(f"{who}: levels must be 0 or 255, got {levels!r}")
        B, K = int(pts.shape[0]), int(pts.shape[1])
        counts = self._counts(counts, B, who)
        if pixel_space:                  # the matrices already act on pixel coordinates: passed to the kernel as they are
            mats = self._f32(homographies, (B, 3, 3), f"{who}: homographies")
        else:
            mats = self._scaled(homographies, B, float(W), float(H), -1.)
        out = torch.empty(B, int(H), int(W), dtype=torch.float32, device=self.device)
        flag = torch.empty(1, dtype=torch.int32, device=self.device)
        self._check(self.sploop.imx_warp_labels_bi(self.handle, _ptr(pts), _ptr(counts), B, K, _ptr(mats), int(H), int(W), int(levels), _ptr(out),
                                                   _ptr(flag), _stream(self.device)))
        return out, flag

    def adam_flat(self, p, g, m, v, lr, betas, eps, weight_decay, step, zero_grad=False):
        """One step of torch.optim.Adam (amsgrad=False, maximize=False) on four flat fp32 cuda tensors of n floats, IN PLACE, one launch:
        p parameters, g gradients, m exp_avg, v exp_avg_sq.  `step` is the step count t >= 1 AFTER this step, a host integer: the bias
        corrections are formed here in double.  zero_grad stores 0 to g after reading it.  1-D contiguous views are taken as they
        are (no copy); anything else raises.  No host synchronisation."""
        who = "adam_flat"
        n = int(p.numel())
        for t, what in ((p, "p"), (g, "g"), (m, "m"), (v, "v")):
            self._sppool_tensor(who, t, what)
            if t.dim() != 1 or int(t.numel()) != n:
                raise ImxError(f"{who}: {what} must be a flat tensor of {n} floats, got {tuple(t.shape)}")
        step = int(step)
        if step < 1:
            raise ImxError(f"{who}: step must be >= 1, got {step}")
        b1, b2 = float(betas[0]), float(betas[1])
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ImxError(f"{who}: bad scalar: betas must lie in [0, 1), got {betas!r}")
        step_size = float(lr) / (1.0 - b1 ** step)
        inv_sqrt_bc2 = 1.0 / math.sqrt(1.0 - b2 ** step)
        self._check(self.sploop.imx_adam_flat(self.handle, _ptr(p), _ptr(g), _ptr(m), _ptr(v), n, step_size, b1, b2, inv_sqrt_bc2, float(eps),
                                              float(weight_decay), int(bool(zero_grad)), _stream(self.device)))

    # ------------------------------------------------------------------ kernel-form options (include/imx.h: imx_set_option)
    def set_option(self, key, value):
        """'mfma' = 'x3' | 'f32', 'latency_forms' = 'auto' | 'off' | 'on' | 'unfused', 'conv' = 'wino' | 'wino_h' | 'wino32' | 'direct',
        'gnn_tail' = 'auto' | 'fused' | 'bf16x3' | 'unfused', 'attention' = 'auto' | 'f16x2' | 'bf16x3', 'linear' = 'auto' | 'f16x2' | 'bf16x3';
        the A/B switches 'conv_swizzle' = 'on' | 'off', 'qkv_amax' = 'epilogue' | 'kernel', 'sinkhorn_group' = 'auto' | 1 | 2 | 4,
        'sinkhorn_prefetch' = 'auto' | 'off' | 'on'; the test hook 'debug_poison' = 'off' | 'nan' | 'huge' | 'zero' (include/imx.h)."""
        self._check(self.lib.imx_set_option(self.handle, key.encode(), str(value).encode()))
        return self

    def get_option(self, key):
        return self.lib.imx_get_option(self.handle, key.encode()).decode()

    # ------------------------------------------------------------------ debug / timing
    def set_debug(self, on=True):
        self._check(self.lib.imx_set_debug(self.handle, int(on)))

    def fetch(self, name):
        shape = (ctypes.c_int64 * 4)()
        nd = ctypes.c_int(0)
        self._check(self.lib.imx_debug_fetch(self.handle, name.encode(), None, 0, shape, ctypes.byref(nd)))
        shp = tuple(shape[i] for i in range(nd.value))
        out = np.empty(shp, dtype=np.float32)
        self._check(self.lib.imx_debug_fetch(self.handle, name.encode(), out.ctypes.data_as(ctypes.c_void_p),
                                             out.size, shape, ctypes.byref(nd)))
        return out

    def set_timing(self, on=True):
        self._check(self.lib.imx_set_timing(self.handle, int(on)))

    def timing_reset(self):
        self._check(self.lib.imx_timing_reset(self.handle))

    def timing_report(self, forms=False):
        """[(name, launches, total_ms)] of the instrumented launches; forms=True appends the kernel form of each row
        ('gemm_x3:bf16x3', ...) as the library reports it (imx_timing_form)."""
        n = self.lib.imx_timing_report(self.handle, -1, None, None, None)
        if n < 0:
            self._check(n)
        rows = []
        for i in range(n):
            name, cnt, ms = ctypes.c_char_p(), ctypes.c_int64(), ctypes.c_double()
            self._check(self.lib.imx_timing_report(self.handle, i, ctypes.byref(name), ctypes.byref(cnt), ctypes.byref(ms)))
            row = (name.value.decode(), cnt.value, ms.value)
            rows.append(row + (self.lib.imx_timing_form(self.handle, i).decode(),) if forms else row)
        return rows
