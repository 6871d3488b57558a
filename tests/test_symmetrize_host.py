"""The device CSR symmetrisation without a GPU: the argument
checks of rthx_csr_symmetrize, which all come before any device call, and the
declaration and export of the two functions the round added
(rthx_csr_symmetrize, rthx_smooth_get_build).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from rthx import abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytraceheattransfer.jl_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-s", "-C", CSRC], check=True)
    return _lib.load()


def _sym(lib, n, rp, ci, vv, w=None, out=True, nnz_out=True):
    i64, i32, dp = C.c_int64, C.c_int32, C.c_double
    cap = 2 * max(len(ci) if ci is not None else 0, 1)
    xrp = np.zeros(max(min(n, 1 << 20), 0) + 1, dtype=np.int64) if out else None
    xci = np.zeros(cap, dtype=np.int32)
    xv = np.zeros(cap)
    xnnz = C.c_int64(-1)
    return lib.rthx_csr_symmetrize(0, n, abi.ptr(rp, i64), abi.ptr(ci, i32), abi.ptr(vv, dp), abi.ptr(w, dp), cap,
                                   abi.ptr(xrp, i64), abi.ptr(xci, i32), abi.ptr(xv, dp),
                                   C.byref(xnnz) if nnz_out else None, None)


def test_csr_symmetrize_validation_without_gpu(lib):
    """Malformed matrices and weights are refused on the host, before any
    device call, each with its code.  (The x_cap protocol -- RTHX_ERANGE with
    the size needed when X does not fit -- needs the merged size, which only
    the device pass computes: tests/test_gpu_symmetrize.py covers it.)"""
    assert lib.rthx_abi_version() == 5
    rp = np.array([0, 2, 3, 3], dtype=np.int64)
    ci = np.array([0, 2, 1], dtype=np.int32)
    vv = np.array([1.0, 2.0, 3.0])
    w = np.array([1.0, 2.0, 0.5])
    E, R = abi.RTHX_EINVAL, abi.RTHX_ERANGE
    # NULL arguments
    assert _sym(lib, 3, None, ci, vv) == E
    assert _sym(lib, 3, rp, ci, vv, out=False) == E
    assert _sym(lib, 3, rp, ci, vv, nnz_out=False) == E
    assert _sym(lib, 3, rp, None, vv) == E
    assert _sym(lib, 3, rp, ci, None) == E
    assert b"null CSR arrays" in lib.rthx_last_error()
    assert _sym(lib, -1, rp, ci, vv) == E
    # row_ptr[0] != 0, non-monotone row_ptr
    assert _sym(lib, 3, np.array([1, 2, 3, 3], dtype=np.int64), ci, vv) == E
    assert b"row_ptr[0]" in lib.rthx_last_error()
    assert _sym(lib, 3, np.array([0, 3, 2, 3], dtype=np.int64), ci, vv) == E
    assert b"monotone" in lib.rthx_last_error()
    # a column out of range on either side
    assert _sym(lib, 3, rp, np.array([0, 3, 1], dtype=np.int32), vv) == E
    assert b"bad CSR entry" in lib.rthx_last_error()
    assert _sym(lib, 3, rp, np.array([-1, 2, 1], dtype=np.int32), vv) == E
    # a row that descends, a row with a repeated column: the message names the row
    assert _sym(lib, 3, rp, np.array([2, 0, 1], dtype=np.int32), vv) == E
    assert b"row 0 is not strictly column-ascending" in lib.rthx_last_error()
    rp2 = np.array([0, 1, 3, 3], dtype=np.int64)
    assert _sym(lib, 3, rp2, np.array([0, 1, 1], dtype=np.int32), vv) == E
    assert b"row 1 is not strictly column-ascending" in lib.rthx_last_error()
    # non-finite values and weights
    assert _sym(lib, 3, rp, ci, np.array([1.0, np.nan, 3.0])) == E
    assert _sym(lib, 3, rp, ci, np.array([1.0, 2.0, -np.inf])) == E
    assert _sym(lib, 3, rp, ci, vv, w=np.array([1.0, np.nan, 1.0])) == E
    assert _sym(lib, 3, rp, ci, vv, w=np.array([1.0, 1.0, np.inf])) == E
    assert b"weights" in lib.rthx_last_error()
    # sizes at 2^31: n (row_ptr is not read past [0]), nnz
    assert _sym(lib, 2 ** 31, rp, ci, vv) == R
    assert _sym(lib, 1, np.array([0, 2 ** 31], dtype=np.int64), ci, vv) == R
    # a well-formed call passes every check: what is left is the device
    # (RTHX_EDEVICE on a machine without one)
    assert _sym(lib, 3, rp, ci, vv, w=w) in (abi.RTHX_OK, abi.RTHX_EDEVICE)


def test_smooth_get_build_null_handle(lib):
    on, ms = C.c_int32(7), C.c_double(7.0)
    assert lib.rthx_smooth_get_build(None, C.byref(on), C.byref(ms)) == abi.RTHX_EINVAL
    assert on.value == 7 and ms.value == 7.0


def test_new_symbols_declared_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "rthx.h")).read()
    for name in ("rthx_csr_symmetrize", "rthx_smooth_get_build"):
        assert name in abi.EXPORTED_SYMBOLS and ("int %s(" % name) in header
        assert hasattr(lib, name)
    assert "#define RTHX_ABI_VERSION 5" in header
    import rthx

    assert callable(rthx.csr_symmetrize)
