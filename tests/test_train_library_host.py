"""The two shared libraries and their tables, stated once: libimx.so exports the 34 entry points of include/imx.h, libimx_train.so the 14
of include/imx_train.h, and nothing else; the ctypes binding declares the same names with the argument counts of the C signatures.
No GPU."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the entry points of the training library by stage, with the number of arguments of each C signature
TRAIN_ENTRY_POINTS = {
    "imx_warp_labels": 12, "imx_erode_mask": 8, "imx_detector_loss": 9, "imx_desc_loss_sparse": 20, "imx_desc_pairs": 8,
    "imx_detector_loss_grad": 11, "imx_desc_loss_sparse_grad": 23,
    "imx_ot_match_loss_grad": 18,
    "imx_mha_forward_train": 14, "imx_mha_backward": 18,
    "imx_conv1x1_forward_train": 13, "imx_conv1x1_backward": 16,
    "imx_bn_relu_forward_train": 18, "imx_bn_relu_backward": 16,
}


def test_the_two_libraries_export_what_their_headers_declare():
    from image_matching_amd import _lib
    header = open(os.path.join(ROOT, "include", "imx_train.h")).read()
    declared = set(re.findall(r"^IMX_API [^\n]*?\b(imx_\w+)\(", header, re.M))
    assert declared == set(_lib.TRAIN_EXPORTS) == set(TRAIN_ENTRY_POINTS)
    assert not declared & set(_lib.EXPORTS)
    assert len(_lib.EXPORTS) == len(set(_lib.EXPORTS)) == 34 and len(_lib.TRAIN_EXPORTS) == len(set(_lib.TRAIN_EXPORTS)) == 14
    # the declarations themselves: as many parameters as the table says (no parameter of the ABI is a function pointer: commas separate them)
    for name, n_args in TRAIN_ENTRY_POINTS.items():
        params = re.search(r"^IMX_API int " + name + r"\(([^)]*)\);", header, re.M | re.S).group(1)
        assert len(params.split(",")) == n_args, name
    nm = shutil.which("nm") or shutil.which("llvm-nm")
    assert nm, "nm (binutils) or llvm-nm is needed to read the dynamic symbol tables: without it nothing here would check them"

    def table(path):
        out = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert table(_lib.TRAIN_LIB_PATH) == declared
    assert table(_lib.LIB_PATH) == set(_lib.EXPORTS)
    lib = _lib.load_train_library()
    for name, n_args in TRAIN_ENTRY_POINTS.items():
        assert len(getattr(lib, name).argtypes) == n_args, name
