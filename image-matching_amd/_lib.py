"""ctypes binding of libimx.so (C ABI: include/imx.h).  There is no CPU fallback: if the
library is missing or no GPU is present the product path raises."""
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


# libimx_sptrain.so (C ABI: include/imx_sptrain.h): the descriptor-training stages, on libimx.so's handles
SPTRAIN_LIB_PATH = os.path.join(_HERE, "libimx_sptrain.so")
SPTRAIN_EXPORTS = ("imx_warp_labels", "imx_erode_mask", "imx_detector_loss", "imx_desc_pairs", "imx_desc_loss_sparse")
# libimx_spgrad.so (C ABI: include/imx_spgrad.h): the two training losses as value-and-gradient calls, on libimx.so's handles
SPGRAD_LIB_PATH = os.path.join(_HERE, "libimx_spgrad.so")
SPGRAD_EXPORTS = ("imx_detector_loss_grad", "imx_desc_loss_sparse_grad")
# libimx_otgrad.so (C ABI: include/imx_otgrad.h): the SuperGlue match loss through the unrolled Sinkhorn, value-and-gradient, on libimx.so's handles
OTGRAD_LIB_PATH = os.path.join(_HERE, "libimx_otgrad.so")
OTGRAD_EXPORTS = ("imx_ot_match_loss_grad",)
# libimx_mhagrad.so (C ABI: include/imx_mhagrad.h): the GNN's attention in its training form (forward with the row log-sum-exp, backward), on libimx.so's handles
MHAGRAD_LIB_PATH = os.path.join(_HERE, "libimx_mhagrad.so")
MHAGRAD_EXPORTS = ("imx_mha_forward_train", "imx_mha_backward")
# libimx_lingrad.so (C ABI: include/imx_lingrad.h): the 1x1 convolutions of the GNN in their training form (forward, and the gradients at the inputs, weight and bias), on libimx.so's handles
LINGRAD_LIB_PATH = os.path.join(_HERE, "libimx_lingrad.so")
LINGRAD_EXPORTS = ("imx_conv1x1_forward_train", "imx_conv1x1_backward")
# libimx_bngrad.so (C ABI: include/imx_bngrad.h): BatchNorm1d + ReLU of the MLPs in their training form (forward and backward, one launch each), on libimx.so's handles
BNGRAD_LIB_PATH = os.path.join(_HERE, "libimx_bngrad.so")
BNGRAD_EXPORTS = ("imx_bn_relu_forward_train", "imx_bn_relu_backward")

_lib = None
_sptrain = None
_spgrad = None
_otgrad = None
_mhagrad = None
_lingrad = None
_bngrad = None


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


def load_sptrain_library():
    """Load libimx_sptrain.so (built beside libimx.so by the same make); libimx.so is loaded first: it makes the handles."""
    global _sptrain
    if _sptrain is not None:
        return _sptrain
    load_library()
    if not os.path.exists(SPTRAIN_LIB_PATH):
        raise RuntimeError(f"libimx_sptrain.so not found at {SPTRAIN_LIB_PATH}: build it with `make -C image-matching_amd/csrc`")
    lib = ctypes.CDLL(SPTRAIN_LIB_PATH)
    vp, i32, f32p = ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p
    lib.imx_warp_labels.argtypes = [vp, f32p, vp, i32, i32, f32p, i32, i32, f32p, f32p, vp, vp]
    lib.imx_erode_mask.argtypes = [vp, f32p, f32p, i32, i32, i32, i32, vp]
    lib.imx_detector_loss.argtypes = [vp, f32p, f32p, f32p, i32, i32, i32, f32p, vp]
    lib.imx_desc_loss_sparse.argtypes = [vp, f32p, f32p, i32, i32, i32, i32, f32p, vp, vp, i32, i32, ctypes.c_float, ctypes.c_float, i32,
                                         f32p, f32p, vp, vp, vp]
    lib.imx_desc_pairs.argtypes = [vp, f32p, i32, i32, i32, vp, vp, vp]
    for name in SPTRAIN_EXPORTS:
        getattr(lib, name)
    _sptrain = lib
    return lib


def load_spgrad_library():
    """Load libimx_spgrad.so (built beside libimx.so by the same make); libimx.so is loaded first: it makes the handles."""
    global _spgrad
    if _spgrad is not None:
        return _spgrad
    load_library()
    if not os.path.exists(SPGRAD_LIB_PATH):
        raise RuntimeError(f"libimx_spgrad.so not found at {SPGRAD_LIB_PATH}: build it with `make -C image-matching_amd/csrc`")
    lib = ctypes.CDLL(SPGRAD_LIB_PATH)
    vp, i32, f32p = ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p
    lib.imx_detector_loss_grad.argtypes = [vp, f32p, f32p, f32p, i32, i32, i32, f32p, f32p, f32p, vp]
    lib.imx_desc_loss_sparse_grad.argtypes = [vp, f32p, f32p, i32, i32, i32, i32, f32p, vp, vp, i32, i32, ctypes.c_float, ctypes.c_float, i32,
                                              f32p, f32p, f32p, vp, vp, f32p, f32p, vp]
    for name in SPGRAD_EXPORTS:
        getattr(lib, name)
    _spgrad = lib
    return lib


def load_otgrad_library():
    """Load libimx_otgrad.so (built beside libimx.so by the same make); libimx.so is loaded first: it makes the handles."""
    global _otgrad
    if _otgrad is not None:
        return _otgrad
    load_library()
    if not os.path.exists(OTGRAD_LIB_PATH):
        raise RuntimeError(f"libimx_otgrad.so not found at {OTGRAD_LIB_PATH}: build it with `make -C image-matching_amd/csrc`")
    lib = ctypes.CDLL(OTGRAD_LIB_PATH)
    vp, i32, f32p = ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p
    lib.imx_ot_match_loss_grad.argtypes = [vp, i32, f32p, i32, i32, vp, vp, f32p, i32, vp, vp, i32, f32p, f32p, f32p, f32p, vp, vp]
    for name in OTGRAD_EXPORTS:
        getattr(lib, name)
    _otgrad = lib
    return lib


def load_mhagrad_library():
    """Load libimx_mhagrad.so (built beside libimx.so by the same make); libimx.so is loaded first: it makes the handles."""
    global _mhagrad
    if _mhagrad is not None:
        return _mhagrad
    load_library()
    if not os.path.exists(MHAGRAD_LIB_PATH):
        raise RuntimeError(f"libimx_mhagrad.so not found at {MHAGRAD_LIB_PATH}: build it with `make -C image-matching_amd/csrc`")
    lib = ctypes.CDLL(MHAGRAD_LIB_PATH)
    vp, i32, f32p = ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p
    lib.imx_mha_forward_train.argtypes = [vp, i32, i32, i32, i32, i32, f32p, f32p, f32p, vp, vp, f32p, f32p, vp]
    lib.imx_mha_backward.argtypes = [vp, i32, i32, i32, i32, i32, f32p, f32p, f32p, f32p, f32p, f32p, vp, vp, f32p, f32p, f32p, vp]
    for name in MHAGRAD_EXPORTS:
        getattr(lib, name)
    _mhagrad = lib
    return lib


def load_lingrad_library():
    """Load libimx_lingrad.so (built beside libimx.so by the same make); libimx.so is loaded first: it makes the handles."""
    global _lingrad
    if _lingrad is not None:
        return _lingrad
    load_library()
    if not os.path.exists(LINGRAD_LIB_PATH):
        raise RuntimeError(f"libimx_lingrad.so not found at {LINGRAD_LIB_PATH}: build it with `make -C image-matching_amd/csrc`")
    lib = ctypes.CDLL(LINGRAD_LIB_PATH)
    vp, i32, f32p = ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p
    lib.imx_conv1x1_forward_train.argtypes = [vp, i32, i32, i32, i32, i32, f32p, f32p, f32p, f32p, vp, f32p, vp]
    lib.imx_conv1x1_backward.argtypes = [vp, i32, i32, i32, i32, i32, f32p, f32p, f32p, f32p, vp, f32p, f32p, f32p, f32p, vp]
    for name in LINGRAD_EXPORTS:
        getattr(lib, name)
    _lingrad = lib
    return lib


def load_bngrad_library():
    """Load libimx_bngrad.so (built beside libimx.so by the same make); libimx.so is loaded first: it makes the handles."""
    global _bngrad
    if _bngrad is not None:
        return _bngrad
    load_library()
    if not os.path.exists(BNGRAD_LIB_PATH):
        raise RuntimeError(f"libimx_bngrad.so not found at {BNGRAD_LIB_PATH}: build it with `make -C image-matching_amd/csrc`")
    lib = ctypes.CDLL(BNGRAD_LIB_PATH)
    vp, i32, f32, f32p = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_void_p
    lib.imx_bn_relu_forward_train.argtypes = [vp, i32, i32, i32, i32, f32, f32, f32p, f32p, f32p, vp, f32p, f32p, vp, f32p, f32p, f32p, vp]
    lib.imx_bn_relu_backward.argtypes = [vp, i32, i32, i32, i32, f32p, f32p, f32p, f32p, f32p, f32p, vp, f32p, f32p, f32p, vp]
    for name in BNGRAD_EXPORTS:
        getattr(lib, name)
    _bngrad = lib
    return lib
