"""The sparse pipeline's host side without a GPU:
csrc/rthx_csr_host.h -- the one CSR check, the one host transpose and the
symmetric part -- through tests/csr_host_check.cpp, built with
AddressSanitizer and UBSan; and rthx_solve_grey's validation of a sparse F,
which comes from that check before the device is opened.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from rthx import abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytraceheattransfer.jl_amd", "csrc")


def test_check_transpose_and_symmetric_part(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "csr_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "csr_host_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    check = 25                            # refusals, switches, empty rows
    transpose = 5 * 4 * 3 * 2 * 6 + 3     # shapes x densities x (un)sorted x variants; one column; Host form
    symmetric = 5 * 3 * 3 + 2             # sizes x densities x repeats; symmetric and unmatched patterns
    assert "csr host ok: %d cases" % (check + transpose + symmetric) in out.stdout


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-s", "-C", CSRC], check=True)
    return _lib.load()


def _solve(lib, n, rp, ci, vv):
    i64, i32, dp = C.c_int64, C.c_int32, C.c_double
    co, h, j, g = np.full(n, 0.5), np.ones(n), np.empty(n), np.empty(n)
    a = abi.SolveArgs()
    a.device, a.memory, a.itmax, a.rtol, a.atol = 0, 50, 0, 1e-12, 1e-8
    return lib.rthx_solve_grey(abi.ptr(rp, i64), abi.ptr(ci, i32), abi.ptr(vv, dp), None, n, abi.ptr(co, dp),
                               abi.ptr(h, dp), C.byref(a), abi.ptr(j, dp), abi.ptr(g, dp), None)


def test_solve_grey_sparse_validation_without_gpu(lib):
    """A malformed sparse F is refused on the host, before the device is
    opened: RTHX_EINVAL on a machine without a GPU too."""
    n = 4
    rp = np.array([0, 1, 2, 3, 4], dtype=np.int64)
    ci = np.array([1, 0, 3, 2], dtype=np.int32)
    vv = np.array([0.5, 0.25, 0.5, 0.25])
    E = abi.RTHX_EINVAL
    # a row pointer that jumps past nnz = row_ptr[n] and comes back: no entry is read
    assert _solve(lib, n, np.array([0, 5, 2, 3, 4], dtype=np.int64), ci, vv) == E
    assert b"monotone" in lib.rthx_last_error()
    assert _solve(lib, n, np.array([1, 1, 2, 3, 4], dtype=np.int64), ci, vv) == E
    assert b"row_ptr[0]" in lib.rthx_last_error()
    assert _solve(lib, n, None, ci, vv) == E
    assert _solve(lib, n, rp, None, vv) == E
    assert b"null CSR arrays" in lib.rthx_last_error()
    # a non-finite value, a column out of range on either side
    for bad in (np.nan, np.inf):
        assert _solve(lib, n, rp, ci, np.array([0.5, bad, 0.5, 0.25])) == E
        assert b"bad CSR entry" in lib.rthx_last_error()
    for bad in (n, -1):
        assert _solve(lib, n, rp, np.array([1, 0, bad, 2], dtype=np.int32), vv) == E
        assert b"bad CSR entry" in lib.rthx_last_error()
    # a well-formed call passes every check: what is left is the device
    assert _solve(lib, n, rp, ci, vv) in (abi.RTHX_OK, abi.RTHX_EDEVICE)
