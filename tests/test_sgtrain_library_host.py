"""The third shared library and its table: libimx_sgtrain.so exports the two entry points of include/imx_sgtrain.h and nothing else, the
ctypes binding declares the same names with the argument counts of the C signatures, none of them is an entry point of libimx.so or
libimx_train.so, and the header is plain C.  No GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the entry points with the number of arguments of each C signature
SGTRAIN_ENTRY_POINTS = {"imx_score_product_forward_train": 12, "imx_score_product_backward": 14}


def test_the_library_exports_what_its_header_declares():
    from image_matching_amd import _lib
    header = open(os.path.join(ROOT, "include", "imx_sgtrain.h")).read()
    declared = set(re.findall(r"^IMX_API [^\n]*?\b(imx_\w+)\(", header, re.M))
    assert declared == set(_lib.SGTRAIN_EXPORTS) == set(SGTRAIN_ENTRY_POINTS)
    assert len(_lib.SGTRAIN_EXPORTS) == len(set(_lib.SGTRAIN_EXPORTS)) == 2
    assert not declared & set(_lib.EXPORTS) and not declared & set(_lib.TRAIN_EXPORTS)
    # the declarations themselves: as many parameters as the table says (no parameter of the ABI is a function pointer: commas separate them)
    for name, n_args in SGTRAIN_ENTRY_POINTS.items():
        params = re.search(r"^IMX_API int " + name + r"\(([^)]*)\);", header, re.M | re.S).group(1)
        assert len(params.split(",")) == n_args, name
    nm = shutil.which("nm") or shutil.which("llvm-nm")
    assert nm, "nm (binutils) or llvm-nm is needed to read the dynamic symbol table: without it nothing here would check it"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.SGTRAIN_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {ln.split()[-1] for ln in out.splitlines() if ln.strip()} == declared
    lib = _lib.load_sgtrain_library()
    for name, n_args in SGTRAIN_ENTRY_POINTS.items():
        assert len(getattr(lib, name).argtypes) == n_args == len(_lib._SGTRAIN_ARGTYPES[name]), name


def test_header_is_plain_c(tmp_path):
    """include/imx_sgtrain.h compiles as C99 with every warning an error, and a C caller of both entry points links against the library"""
    from image_matching_amd import _lib
    if not shutil.which("gcc") or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("gcc / ROCm headers not present")
    src = tmp_path / "use_sgtrain.c"
    src.write_text('#include "imx_sgtrain.h"\n'
                   "int main(void) {\n"
                   "  int rc = imx_score_product_forward_train(0, 1, 1, 1, 1, 0, 0, 0, 0, 1.0f, 0, 0);\n"
                   "  rc += imx_score_product_backward(0, 1, 1, 1, 1, 0, 0, 0, 0, 0, 1.0f, 0, 0, 0);\n"
                   "  return rc == -2 ? 0 : 1;\n"           # a null handle is an error code, not a crash
                   "}\n")
    libdir = os.path.dirname(_lib.SGTRAIN_LIB_PATH)
    exe = str(tmp_path / "use_sgtrain")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                    "-D__HIP_PLATFORM_AMD__", str(src), "-L" + libdir, "-limx_sgtrain", "-L/opt/rocm/lib", "-lamdhip64", "-o", exe], check=True)
    env = dict(os.environ, LD_LIBRARY_PATH=libdir + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    assert subprocess.run([exe], env=env, timeout=120).returncode == 0
