"""The device CSR transpose without a GPU: its host-side
planning (csrc/rthx_transpose_plan.h) through tests/transpose_plan_check.cpp,
built with AddressSanitizer and UBSan; the argument checks of
rthx_csr_transpose and rthx_solve_grey_result that come before any device
work; and that csrc/ is free of sort libraries.
"""
import ctypes as C
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest

from rthx import abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytraceheattransfer.jl_amd", "csrc")


def test_plan_covers_bits_tiles_and_scratch(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "transpose_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "transpose_plan_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "transpose plan ok: %d cases" % (2 * 70000 + 9 * 6 * 2) in out.stdout


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-s", "-C", CSRC], check=True)
    return _lib.load()


def _transpose(lib, n_rows, n_cols, rp, ci, vv, out=True):
    i64, i32, dp = C.c_int64, C.c_int32, C.c_double
    nnz = max(len(ci) if ci is not None else 0, 1)
    trp = np.zeros(max(min(n_cols, 1 << 20), 0) + 1, dtype=np.int64) if out else None
    tci = np.zeros(nnz, dtype=np.int32) if out else None
    tv = np.zeros(nnz) if out else None
    return lib.rthx_csr_transpose(0, n_rows, n_cols, abi.ptr(rp, i64), abi.ptr(ci, i32), abi.ptr(vv, dp),
                                  abi.ptr(trp, i64), abi.ptr(tci, i32), abi.ptr(tv, dp), None)


def test_csr_transpose_validation_without_gpu(lib):
    """Malformed matrices are refused on the host, before any device call."""
    assert lib.rthx_abi_version() == 5
    rp = np.array([0, 2, 3], dtype=np.int64)
    ci = np.array([0, 2, 1], dtype=np.int32)
    vv = np.array([1.0, 2.0, 3.0])
    # NULL arguments
    assert _transpose(lib, 2, 3, None, ci, vv) == abi.RTHX_EINVAL
    assert _transpose(lib, 2, 3, rp, None, vv) == abi.RTHX_EINVAL
    assert _transpose(lib, 2, 3, rp, ci, None) == abi.RTHX_EINVAL
    assert _transpose(lib, 2, 3, rp, ci, vv, out=False) == abi.RTHX_EINVAL
    assert _transpose(lib, -1, 3, rp, ci, vv) == abi.RTHX_EINVAL
    # row_ptr[0] != 0, non-monotone row_ptr
    assert _transpose(lib, 2, 3, np.array([1, 2, 3], dtype=np.int64), ci, vv) == abi.RTHX_EINVAL
    assert b"row_ptr[0]" in lib.rthx_last_error()
    assert _transpose(lib, 2, 3, np.array([0, 3, 2], dtype=np.int64), ci, vv) == abi.RTHX_EINVAL
    assert b"monotone" in lib.rthx_last_error()
    # a column out of range (either side), a NaN and an infinite value
    assert _transpose(lib, 2, 2, rp, ci, vv) == abi.RTHX_EINVAL
    assert _transpose(lib, 2, 3, rp, np.array([0, -1, 1], dtype=np.int32), vv) == abi.RTHX_EINVAL
    assert _transpose(lib, 2, 3, rp, ci, np.array([1.0, np.nan, 3.0])) == abi.RTHX_EINVAL
    assert _transpose(lib, 2, 3, rp, ci, np.array([1.0, 2.0, np.inf])) == abi.RTHX_EINVAL
    assert b"bad CSR entry" in lib.rthx_last_error()
    # sizes at 2^31: n_rows, n_cols (row_ptr is not read past [0]), nnz
    assert _transpose(lib, 2 ** 31, 3, rp, ci, vv) == abi.RTHX_ERANGE
    assert _transpose(lib, 2, 2 ** 31, rp, ci, vv) == abi.RTHX_ERANGE
    assert _transpose(lib, 1, 3, np.array([0, 2 ** 31], dtype=np.int64), ci, vv) == abi.RTHX_ERANGE
    assert _transpose(lib, 2 ** 31 - 1, 3, np.array([0, 2 ** 31], dtype=np.int64), ci, vv) == abi.RTHX_ERANGE


def test_solve_grey_result_validation_without_gpu(lib):
    dp = C.c_double
    n = 4
    co, h, j, g = np.ones(n), np.ones(n), np.empty(n), np.empty(n)
    a = abi.SolveArgs()
    a.device, a.memory, a.itmax, a.rtol, a.atol = 0, 50, 0, 1e-12, 1e-8
    ptrs = (abi.ptr(co, dp), abi.ptr(h, dp), C.byref(a), abi.ptr(j, dp), abi.ptr(g, dp), None)
    assert lib.rthx_solve_grey_result(None, n, *ptrs) == abi.RTHX_EINVAL
    r = C.c_void_p()
    assert lib.rthx_result_create(C.byref(r)) == 0
    try:
        assert lib.rthx_solve_grey_result(r, n, *ptrs) == abi.RTHX_ESTATE  # no trace in it
    finally:
        lib.rthx_result_destroy(r)


def test_no_sort_library_in_csrc():
    """The transpose is the project's own kernel: no hipCUB / rocPRIM include
    or mention is left under csrc/."""
    files = [p for p in glob.glob(os.path.join(CSRC, "*")) if os.path.isfile(p)]
    assert len(files) > 20
    hits = []
    for p in files:
        text = open(p, errors="replace").read().lower()
        hits += [os.path.basename(p) for word in ("hipcub", "rocprim") if word in text]
    assert not hits, hits
    assert os.path.exists(os.path.join(CSRC, "rthx_transpose_kernels.hip"))


def test_new_symbols_declared_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "rthx.h")).read()
    for name in ("rthx_csr_transpose", "rthx_solve_grey_result"):
        assert name in abi.EXPORTED_SYMBOLS and ("int %s(" % name) in header
        assert hasattr(lib, name)
