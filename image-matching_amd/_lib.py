"""ctypes binding of libimx.so (C ABI: include/imx.h), libimx_train.so (include/imx_train.h), libimx_sgtrain.so
(include/imx_sgtrain.h), libimx_spnet.so (include/imx_spnet.h), libimx_spnorm.so (include/imx_spnorm.h), libimx_sppool.so (include/imx_sppool.h),
libimx_photo.so (include/imx_photo.h), libimx_sploop.so (include/imx_sploop.h), libimx_sgloop.so (include/imx_sgloop.h), libimx_homog.so
(include/imx_homog.h) and libimx_speval.so (include/imx_speval.h): eleven libraries.  There is no CPU fallback: if the library is missing or no GPU is present the product path raises."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libimx.so")

IMX_MAX_GNN_LAYERS = 64
IMX_MAX_KENC = 8
NET_SUPERPOINT, NET_SUPERGLUE = 0, 1
SP_VARIANT_BN, SP_VARIANT_OFFICIAL = 0, 1

EXPORTS = (
    "imx_create", "imx_destroy", "imx_last_error", "imx_load_weight", "imx_finalize_weights",
    "imx_superpoint_detect", "imx_superpoint_describe", "imx_superpoint_dense", "imx_superglue_forward",
    "imx_match_pairs", "imx_pack_records", "imx_gather_records", "imx_estimate_affine_partial", "imx_knn_ratio_match", "imx_ingest_resize_u8", "imx_warp_affine_u8", "imx_op_nms",
    "imx_warp_homography", "imx_combine_heatmap", "imx_superpoint_heatmap", "imx_homography_adapt", "imx_heatmap_points",
    "imx_warp_perspective_u8", "imx_gt_matches", "imx_match_loss", "imx_set_debug", "imx_debug_fetch", "imx_set_timing",
    "imx_timing_report", "imx_timing_reset", "imx_timing_form", "imx_set_option", "imx_get_option", "imx_version",
)


class ImxConfig(ctypes.Structure):
    _fields_ = [
        ("descriptor_dim", ctypes.c_int32),
        ("nms_radius", ctypes.c_int32),
        ("keypoint_threshold", ctypes.c_float),
        ("max_keypoints", ctypes.c_int32),
        ("remove_borders", ctypes.c_int32),
        ("align_corners", ctypes.c_int32),
        ("sp_variant", ctypes.c_int32),
        ("num_gnn_layers", ctypes.c_int32),
        ("gnn_layer_is_cross", ctypes.c_int32 * IMX_MAX_GNN_LAYERS),
        ("kenc_n", ctypes.c_int32),
        ("kenc_channels", ctypes.c_int32 * IMX_MAX_KENC),
        ("sinkhorn_iterations", ctypes.c_int32),
        ("match_threshold", ctypes.c_float),
    ]


# libimx_train.so (C ABI: include/imx_train.h): the training stages, on libimx.so's handles -- name -> argtypes, one line per entry point
TRAIN_LIB_PATH = os.path.join(_HERE, "libimx_train.so")
_vp, _i32, _f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
_TRAIN_ARGTYPES = {
    # SuperPoint descriptor training: labels, masks, the forward values of the two losses
    "imx_warp_labels": [_vp, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp],
    "imx_erode_mask": [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp],
    "imx_detector_loss": [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp],
    "imx_desc_pairs": [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp],
    "imx_desc_loss_sparse": [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _f32, _f32, _i32, _vp, _vp, _vp, _vp, _vp],
    # the two losses as value-and-gradient calls
    "imx_detector_loss_grad": [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp],
    "imx_desc_loss_sparse_grad": [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _f32, _f32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    # the SuperGlue match loss through the unrolled Sinkhorn, value-and-gradient
    "imx_ot_match_loss_grad": [_vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp],
    # the GNN's attention, 1x1 convolutions and BatchNorm1d + ReLU in their training form, forward and backward
    "imx_mha_forward_train": [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "imx_mha_backward": [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "imx_conv1x1_forward_train": [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "imx_conv1x1_backward": [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "imx_bn_relu_forward_train": [_vp, _i32, _i32, _i32, _i32, _f32, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "imx_bn_relu_backward": [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
}
TRAIN_EXPORTS = tuple(_TRAIN_ARGTYPES)

# libimx_sgtrain.so (C ABI: include/imx_sgtrain.h): the score product of SuperGlue's training step, on libimx.so's handles -- a library of
# its own because libimx_train.so's symbol table is pinned to imx_train.h; name -> argtypes, one line per entry point
SGTRAIN_LIB_PATH = os.path.join(_HERE, "libimx_sgtrain.so")
_SGTRAIN_ARGTYPES = {
    "imx_score_product_forward_train": [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _f32, _vp, _vp],
    "imx_score_product_backward": [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _vp],
}
SGTRAIN_EXPORTS = tuple(_SGTRAIN_ARGTYPES)

# libimx_spnet.so (C ABI: include/imx_spnet.h): the 3x3 convolutions of SuperPoint's training step, on libimx.so's handles -- a library of
# its own because the other three symbol tables are pinned to their headers; name -> argtypes, one line per entry point
SPNET_LIB_PATH = os.path.join(_HERE, "libimx_spnet.so")
_SPNET_ARGTYPES = {
    "imx_conv3x3_forward_train": [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp],
    "imx_conv3x3_backward": [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
}
SPNET_EXPORTS = tuple(_SPNET_ARGTYPES)

# libimx_spnorm.so (C ABI: include/imx_spnorm.h): BatchNorm2d [+ ReLU] of SuperPoint's training step on NCHW maps, on libimx.so's handles -- a
# library of its own because the other four symbol tables are pinned to their headers; name -> argtypes, one line per entry point
SPNORM_LIB_PATH = os.path.join(_HERE, "libimx_spnorm.so")
_SPNORM_ARGTYPES = {
    "imx_bn2d_forward_train": [_vp, _i32, _i32, _i32, _i32, _i32, _f32, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "imx_bn2d_backward": [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
}
SPNORM_EXPORTS = tuple(_SPNORM_ARGTYPES)

# libimx_sppool.so (C ABI: include/imx_sppool.h): MaxPool2d(2) and the descriptor normalisation of SuperPoint's training step on NCHW maps, on
# libimx.so's handles -- a library of its own because the other five symbol tables are pinned to their headers; name -> argtypes
SPPOOL_LIB_PATH = os.path.join(_HERE, "libimx_sppool.so")
_SPPOOL_ARGTYPES = {
    "imx_maxpool2_forward_train": [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp],
    "imx_maxpool2_backward": [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp],
    "imx_l2norm_forward_train": [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp],
    "imx_l2norm_backward": [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp],
}
SPPOOL_EXPORTS = tuple(_SPPOOL_ARGTYPES)

# libimx_photo.so (C ABI: include/imx_photo.h): the photometric augmentation of SuperPoint's training data, on libimx.so's handles -- a library
# of its own because the other six symbol tables are pinned to their headers; name -> argtypes
PHOTO_LIB_PATH = os.path.join(_HERE, "libimx_photo.so")
_PHOTO_ARGTYPES = {
    "imx_photo_pixels": [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "imx_photo_shade": [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
}
PHOTO_EXPORTS = tuple(_PHOTO_ARGTYPES)

# libimx_sploop.so (C ABI: include/imx_sploop.h): the bilinear label splat of gaussian_label and the flat Adam step of SuperPoint's training
# loop, on libimx.so's handles -- a library of its own because the other seven symbol tables are pinned to their headers; name -> argtypes
SPLOOP_LIB_PATH = os.path.join(_HERE, "libimx_sploop.so")
_f64, _i64 = ctypes.c_double, ctypes.c_int64
_SPLOOP_ARGTYPES = {
    "imx_warp_labels_bi": [_vp, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _vp],
    "imx_adam_flat": [_vp, _vp, _vp, _vp, _vp, _i64, _f64, _f64, _f64, _f64, _f64, _f64, _i32, _vp],
}
SPLOOP_EXPORTS = tuple(_SPLOOP_ARGTYPES)

# libimx_sgloop.so (C ABI: include/imx_sgloop.h): the matches of SuperGlue's training forward from the loss's own Sinkhorn, on libimx.so's
# handles -- a library of its own because the other eight symbol tables are pinned to their headers; name -> argtypes
SGLOOP_LIB_PATH = os.path.join(_HERE, "libimx_sgloop.so")
_SGLOOP_ARGTYPES = {
    "imx_assignment_matches": [_vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "imx_ot_match_loss_grad_matches": [_vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp,
                                       _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
}
SGLOOP_EXPORTS = tuple(_SGLOOP_ARGTYPES)

# libimx_homog.so (C ABI: include/imx_homog.h): the batched RANSAC homography fit on matched keypoints and the corner error of a fit against a
# known warp, on libimx.so's handles -- a library of its own because the other nine symbol tables are pinned to their headers; name -> argtypes
HOMOG_LIB_PATH = os.path.join(_HERE, "libimx_homog.so")
_u32 = ctypes.c_uint32
_HOMOG_ARGTYPES = {
    "imx_estimate_homography": [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _f64, _i32, _i32, _u32, _vp, _vp, _vp, _vp, _vp],
    "imx_homography_corner_error": [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp],
}
HOMOG_EXPORTS = tuple(_HOMOG_ARGTYPES)

# libimx_speval.so (C ABI: include/imx_speval.h): the mutual nearest-neighbour descriptor matcher and the pair metrics of SuperPoint's validation
# under a known warp, on libimx.so's handles -- a library of its own because the other ten symbol tables are pinned to their headers; name -> argtypes
SPEVAL_LIB_PATH = os.path.join(_HERE, "libimx_speval.so")
_SPEVAL_ARGTYPES = {
    "imx_mutual_nn_match": [_vp, _i32, _i32, _vp, _i64, _i64, _i64, _vp, _i32, _vp, _i64, _i64, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _vp],
    "imx_keypoint_pair_metrics": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f64, _vp, _vp, _vp],
}
SPEVAL_EXPORTS = tuple(_SPEVAL_ARGTYPES)

_lib = None
_train = None
_sgtrain = None
_spnet = None
_spnorm = None
_sppool = None
_photo = None
_sploop = None
_sgloop = None
_homog = None
_speval = None


def load_library():
    """Load libimx.so (built by __graft_entry__.build() / `make -C image-matching_amd/csrc`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"libimx.so not found at {LIB_PATH}: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc, gfx950). image_matching_amd has no CPU fallback.")
    # torch must bring ITS HIP runtime into the process first: the library shares device memory and streams with torch
    # tensors, and loading libimx.so (linked against /opt/rocm's libamdhip64) before torch left the process with two
    # runtimes -- imx_create then saw no device (measured: build() followed by smoke() in one interpreter).
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    vp, i32, i64, f32p = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    lib.imx_version.restype = ctypes.c_char_p
    lib.imx_create.argtypes = [i32, ctypes.POINTER(ImxConfig), ctypes.POINTER(vp)]
    lib.imx_destroy.argtypes = [vp]
    lib.imx_last_error.argtypes = [vp]
    lib.imx_last_error.restype = ctypes.c_char_p
    lib.imx_load_weight.argtypes = [vp, i32, ctypes.c_char_p, vp, i32, ctypes.POINTER(i64)]
    lib.imx_finalize_weights.argtypes = [vp, i32]
    lib.imx_superpoint_detect.argtypes = [vp, f32p, i32, i32, i32, vp, vp]
    lib.imx_superpoint_describe.argtypes = [vp, i32, i32, f32p, f32p, f32p, vp]
    lib.imx_superpoint_dense.argtypes = [vp, f32p, i32, i32, i32, f32p, f32p, vp]
    lib.imx_superglue_forward.argtypes = [vp, i32,
                                          f32p, f32p, f32p, i64, i64, i64, vp, i32, i32, i32,
                                          f32p, f32p, f32p, i64, i64, i64, vp, i32, i32, i32,
                                          vp, vp, f32p, f32p, vp]
    lib.imx_match_pairs.argtypes = [vp, f32p, f32p, i32, i32, i32] + [vp] * 12 + [vp]
    lib.imx_pack_records.argtypes = [vp, vp, i32, i32] + [vp] * 9 + [i32, vp]
    lib.imx_gather_records.argtypes = [vp, vp, i32, i32, vp, i32, vp, vp]
    lib.imx_estimate_affine_partial.argtypes = [vp, f32p, f32p, vp, vp, i32, i32, ctypes.c_float, i32, ctypes.c_uint32, f32p, vp, vp, vp]
    lib.imx_knn_ratio_match.argtypes = [vp, i32, f32p, i64, i64, i64, vp, i32, f32p, i64, i64, i64, vp, i32, ctypes.c_float, vp, f32p, f32p, vp]
    lib.imx_ingest_resize_u8.argtypes = [vp, vp, i32, i32, i32, i64, f32p, i32, i32, vp]
    lib.imx_warp_affine_u8.argtypes = [vp, vp, i32, i32, ctypes.POINTER(ctypes.c_double), vp, i32, i32, vp]
    lib.imx_op_nms.argtypes = [vp, f32p, f32p, i32, i32, i32, i32, vp]
    lib.imx_warp_homography.argtypes = [vp, f32p, i32, i32, i32, i32, f32p, i32, f32p, vp]
    lib.imx_combine_heatmap.argtypes = [vp, f32p, f32p, f32p, i32, i32, i32, f32p, f32p, vp]
    lib.imx_superpoint_heatmap.argtypes = [vp, f32p, i32, i32, i32, f32p, vp]
    lib.imx_homography_adapt.argtypes = [vp, f32p, i32, i32, i32, f32p, f32p, f32p, f32p, vp]
    lib.imx_heatmap_points.argtypes = [vp, f32p, i32, i32, ctypes.c_float, i32, i32, i32, f32p, i32, vp, vp]
    lib.imx_warp_perspective_u8.argtypes = [vp, vp, i64, vp, vp, i32, i32, i32, vp]
    lib.imx_gt_matches.argtypes = [vp, i32, f32p, vp, i32, f32p, vp, i32, vp, ctypes.c_double, f32p, vp, vp, vp, vp, vp, vp]
    lib.imx_match_loss.argtypes = [vp, i32, vp, vp, i32, vp, vp, f32p, vp, vp]
    lib.imx_set_debug.argtypes = [vp, i32]
    lib.imx_debug_fetch.argtypes = [vp, ctypes.c_char_p, vp, i64, ctypes.POINTER(i64), ctypes.POINTER(i32)]
    lib.imx_set_timing.argtypes = [vp, i32]
    lib.imx_timing_reset.argtypes = [vp]
    lib.imx_timing_report.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(i64),
                                      ctypes.POINTER(ctypes.c_double)]
    lib.imx_timing_form.argtypes = [vp, i32]
    lib.imx_timing_form.restype = ctypes.c_char_p
    lib.imx_set_option.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p]
    lib.imx_get_option.argtypes = [vp, ctypes.c_char_p]
    lib.imx_get_option.restype = ctypes.c_char_p
    for name in EXPORTS:
        getattr(lib, name)          # raises AttributeError if a declared symbol is missing
    _lib = lib
    return lib


def load_train_library():
    """Load libimx_train.so (built beside libimx.so by the same make); libimx.so is loaded first: it makes the handles."""
    global _train
    if _train is not None:
        return _train
    load_library()
    if not os.path.exists(TRAIN_LIB_PATH):
        raise RuntimeError(f"libimx_train.so not found at {TRAIN_LIB_PATH}: build it with `make -C image-matching_amd/csrc`")
    lib = ctypes.CDLL(TRAIN_LIB_PATH)
    for name, argtypes in _TRAIN_ARGTYPES.items():
        getattr(lib, name).argtypes = argtypes          # raises AttributeError if a declared symbol is missing
    _train = lib
    return lib


def load_sgtrain_library():
    """Load libimx_sgtrain.so (built beside libimx.so by the same make); libimx.so is loaded first: it makes the handles."""
    global _sgtrain
    if _sgtrain is not None:
        return _sgtrain
    load_library()
    if not os.path.exists(SGTRAIN_LIB_PATH):
        raise RuntimeError(f"libimx_sgtrain.so not found at {SGTRAIN_LIB_PATH}: build it with `make -C image-matching_amd/csrc`")
    lib = ctypes.CDLL(SGTRAIN_LIB_PATH)
    for name, argtypes in _SGTRAIN_ARGTYPES.items():
        getattr(lib, name).argtypes = argtypes          # raises AttributeError if a declared symbol is missing
    _sgtrain = lib
    return lib


def load_spnet_library():
    """Load libimx_spnet.so (built beside libimx.so by the same make); libimx.so is loaded first: it makes the handles."""
    global _spnet
    if _spnet is not None:
        return _spnet
    load_library()
    if not os.path.exists(SPNET_LIB_PATH):
        raise RuntimeError(f"libimx_spnet.so not found at {SPNET_LIB_PATH}: build it with `make -C image-matching_amd/csrc`")
    lib = ctypes.CDLL(SPNET_LIB_PATH)
    for name, argtypes in _SPNET_ARGTYPES.items():
        getattr(lib, name).argtypes = argtypes          # raises AttributeError if a declared symbol is missing
    _spnet = lib
    return lib


def load_spnorm_library():
    """Load libimx_spnorm.so (built beside libimx.so by the same make); libimx.so is loaded first: it makes the handles."""
    global _spnorm
    if _spnorm is not None:
        return _spnorm
    load_library()
    if not os.path.exists(SPNORM_LIB_PATH):
        raise RuntimeError(f"libimx_spnorm.so not found at {SPNORM_LIB_PATH}: build it with `make -C image-matching_amd/csrc`")
    lib = ctypes.CDLL(SPNORM_LIB_PATH)
    for name, argtypes in _SPNORM_ARGTYPES.items():
        getattr(lib, name).argtypes = argtypes          # raises AttributeError if a declared symbol is missing
    _spnorm = lib
    return lib


def load_sppool_library():
    """Load libimx_sppool.so (built beside libimx.so by the same make); libimx.so is loaded first: it makes the handles."""
    global _sppool
    if _sppool is not None:
        return _sppool
    load_library()
    if not os.path.exists(SPPOOL_LIB_PATH):
        raise RuntimeError(f"libimx_sppool.so not found at {SPPOOL_LIB_PATH}: build it with `make -C image-matching_amd/csrc`")
    lib = ctypes.CDLL(SPPOOL_LIB_PATH)
    for name, argtypes in _SPPOOL_ARGTYPES.items():
        getattr(lib, name).argtypes = argtypes          # raises AttributeError if a declared symbol is missing
    _sppool = lib
    return lib


def load_photo_library():
    """Load libimx_photo.so (built beside libimx.so by the same make); libimx.so is loaded first: it makes the handles."""
    global _photo
    if _photo is not None:
        return _photo
    load_library()
    if not os.path.exists(PHOTO_LIB_PATH):
        raise RuntimeError(f"libimx_photo.so not found at {PHOTO_LIB_PATH}: build it with `make -C image-matching_amd/csrc`")
    lib = ctypes.CDLL(PHOTO_LIB_PATH)
    for name, argtypes in _PHOTO_ARGTYPES.items():
        getattr(lib, name).argtypes = argtypes          # raises AttributeError if a declared symbol is missing
    _photo = lib
    return lib


def load_sploop_library():
    """Load libimx_sploop.so (built beside libimx.so by the same make); libimx.so is loaded first: it makes the handles."""
    global _sploop
    if _sploop is not None:
        return _sploop
    load_library()
    if not os.path.exists(SPLOOP_LIB_PATH):
        raise RuntimeError(f"libimx_sploop.so not found at {SPLOOP_LIB_PATH}: build it with `make -C image-matching_amd/csrc`")
    lib = ctypes.CDLL(SPLOOP_LIB_PATH)
    for name, argtypes in _SPLOOP_ARGTYPES.items():
        getattr(lib, name).argtypes = argtypes          # raises AttributeError if a declared symbol is missing
    _sploop = lib
    return lib


def load_sgloop_library():
    """Load libimx_sgloop.so (built beside libimx.so by the same make); libimx.so is loaded first: it makes the handles."""
    global _sgloop
    if _sgloop is not None:
        return _sgloop
    load_library()
    if not os.path.exists(SGLOOP_LIB_PATH):
        raise RuntimeError(f"libimx_sgloop.so not found at {SGLOOP_LIB_PATH}: build it with `make -C image-matching_amd/csrc`")
    lib = ctypes.CDLL(SGLOOP_LIB_PATH)
    for name, argtypes in _SGLOOP_ARGTYPES.items():
        getattr(lib, name).argtypes = argtypes          # raises AttributeError if a declared symbol is missing
    _sgloop = lib
    return lib


def load_homog_library():
    """Load libimx_homog.so (built beside libimx.so by the same make); libimx.so is loaded first: it makes the handles."""
    global _homog
    if _homog is not None:
        return _homog
    load_library()
    if not os.path.exists(HOMOG_LIB_PATH):
        raise RuntimeError(f"libimx_homog.so not found at {HOMOG_LIB_PATH}: build it with `make -C image-matching_amd/csrc`")
    lib = ctypes.CDLL(HOMOG_LIB_PATH)
    for name, argtypes in _HOMOG_ARGTYPES.items():
        getattr(lib, name).argtypes = argtypes          # raises AttributeError if a declared symbol is missing
    _homog = lib
    return lib


def load_speval_library():
    """Load libimx_speval.so (built beside libimx.so by the same make); libimx.so is loaded first: it makes the handles."""
    global _speval
    if _speval is not None:
        return _speval
    load_library()
    if not os.path.exists(SPEVAL_LIB_PATH):
        raise RuntimeError(f"libimx_speval.so not found at {SPEVAL_LIB_PATH}: build it with `make -C image-matching_amd/csrc`")
    lib = ctypes.CDLL(SPEVAL_LIB_PATH)
    for name, argtypes in _SPEVAL_ARGTYPES.items():
        getattr(lib, name).argtypes = argtypes          # raises AttributeError if a declared symbol is missing
    _speval = lib
    return lib
