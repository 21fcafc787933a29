"""The eleventh shared library and its table: libimx_speval.so exports the two entry points of include/imx_speval.h and nothing else, the
ctypes binding declares the same names with the argument counts of the C signatures, none of them is an entry point of the other ten
libraries, whose tables are as they were, the header is plain C, its kernels use no scratch memory and spill no register, and the metric
kernel's LDS fits a CU at the largest size it serves.  No GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the entry points with the number of arguments of each C signature
SPEVAL_ENTRY_POINTS = {"imx_mutual_nn_match": 20, "imx_keypoint_pair_metrics": 16}


def _ten_other_tables():
    from image_matching_amd import _lib
    return ((_lib.LIB_PATH, _lib.EXPORTS), (_lib.TRAIN_LIB_PATH, _lib.TRAIN_EXPORTS), (_lib.SGTRAIN_LIB_PATH, _lib.SGTRAIN_EXPORTS),
            (_lib.SPNET_LIB_PATH, _lib.SPNET_EXPORTS), (_lib.SPNORM_LIB_PATH, _lib.SPNORM_EXPORTS), (_lib.SPPOOL_LIB_PATH, _lib.SPPOOL_EXPORTS),
            (_lib.PHOTO_LIB_PATH, _lib.PHOTO_EXPORTS), (_lib.SPLOOP_LIB_PATH, _lib.SPLOOP_EXPORTS), (_lib.SGLOOP_LIB_PATH, _lib.SGLOOP_EXPORTS),
            (_lib.HOMOG_LIB_PATH, _lib.HOMOG_EXPORTS))


def _dynamic_symbols(path):
    nm = shutil.which("nm") or shutil.which("llvm-nm")
    assert nm, "nm (binutils) or llvm-nm is needed to read the dynamic symbol table: without it nothing here would check it"
    out = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_the_library_exports_what_its_header_declares():
    from image_matching_amd import _lib
    header = open(os.path.join(ROOT, "include", "imx_speval.h")).read()
    declared = set(re.findall(r"^IMX_API [^\n]*?\b(imx_\w+)\(", header, re.M))
    assert declared == set(_lib.SPEVAL_EXPORTS) == set(SPEVAL_ENTRY_POINTS)
    assert len(_lib.SPEVAL_EXPORTS) == len(set(_lib.SPEVAL_EXPORTS)) == 2
    for _, other in _ten_other_tables():
        assert not declared & set(other)
    # the declarations themselves: as many parameters as the table says (no parameter of the ABI is a function pointer: commas separate them)
    for name, n_args in SPEVAL_ENTRY_POINTS.items():
        params = re.search(r"^IMX_API int " + name + r"\(([^)]*)\);", header, re.M | re.S).group(1)
        assert len(params.split(",")) == n_args, name
    assert _dynamic_symbols(_lib.SPEVAL_LIB_PATH) == declared
    lib = _lib.load_speval_library()
    for name, n_args in SPEVAL_ENTRY_POINTS.items():
        assert len(getattr(lib, name).argtypes) == n_args == len(_lib._SPEVAL_ARGTYPES[name]), name


def test_the_ten_other_tables_are_as_they_were():
    """34 / 14 / 2 / 2 / 2 / 4 / 2 / 2 / 2 / 2 entry points: the new library took nothing from the others and added nothing to them"""
    tables = _ten_other_tables()
    assert tuple(len(t) for _, t in tables) == (34, 14, 2, 2, 2, 4, 2, 2, 2, 2)
    for path, table in tables:
        assert _dynamic_symbols(path) == set(table), path


def test_header_is_plain_c(tmp_path):
    """include/imx_speval.h compiles as C99 with every warning an error, and a C caller of the two entry points links against the
    library and gets an error code from a null handle"""
    from image_matching_amd import _lib
    if not shutil.which("gcc") or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("gcc / ROCm headers not present")
    src = tmp_path / "use_speval.c"
    src.write_text('#include "imx_speval.h"\n'
                   "int main(void) {\n"
                   "  int rc = imx_mutual_nn_match(0, 1, 128, 0, 0, 0, 0, 0, 4, 0, 0, 0, 0, 0, 4, 0, 0, 0, 0, 0);\n"
                   "  rc += imx_keypoint_pair_metrics(0, 0, 0, 0, 0, 0, 0, 1, 4, 4, 640, 480, 3.0, 0, 0, 0);\n"
                   "  return rc == -2 ? 0 : 1;\n"           # a null handle is an error code from each call, not a crash
                   "}\n")
    libdir = os.path.dirname(_lib.SPEVAL_LIB_PATH)
    exe = str(tmp_path / "use_speval")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                    "-D__HIP_PLATFORM_AMD__", str(src), "-L" + libdir, "-limx_speval", "-L/opt/rocm/lib", "-lamdhip64", "-o", exe], check=True)
    env = dict(os.environ, LD_LIBRARY_PATH=libdir + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    assert subprocess.run([exe], env=env, timeout=120).returncode == 0


def test_the_kernels_use_no_scratch_and_no_spills():
    """-Rpass-analysis=kernel-resource-usage of csrc/speval.hip for gfx950, with the Makefile's flags: the three kernels -- the search,
    the mutual test and the pair metrics -- report ScratchSize 0 and no SGPR or VGPR spill; the metric kernel's static LDS plus its
    staging at 4096 keypoints a side (two float64 coordinates per point) fits the 160 KB of LDS of a CU"""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not present")
    csrc = os.path.join(ROOT, "image-matching_amd", "csrc")
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-mllvm", "-amdgpu-mfma-vgpr-form=1", "--cuda-device-only",
                          "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "speval.hip"), "-o", os.devnull],
                         capture_output=True, text=True, check=True).stderr
    kernels = re.findall(r"Function Name: (\S+)", out)
    assert len(kernels) == 3
    for stem in ("mnn_search_kernel", "mnn_mutual_kernel", "pair_metrics_kernel"):
        assert sum(stem in k for k in kernels) == 1, stem
    for key in (r"ScratchSize \[bytes/lane\]", "SGPRs Spill", "VGPRs Spill"):
        values = re.findall(key + r": (\d+)", out)
        assert len(values) == 3 and set(values) == {"0"}, (key, values)
    static = dict(zip(kernels, (int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", out))))
    metric = next(v for k, v in static.items() if "pair_metrics_kernel" in k)
    assert metric + 2 * 4096 * 2 * 8 <= 160 * 1024, static
