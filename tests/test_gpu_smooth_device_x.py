"""The sparse smoothing set-up on the device:
rthx_smooth_F_result builds X = (Diagonal(w) F + (Diagonal(w) F)') / 2 from
the trace's counts where they lie (csrc/rthx_symmetrize_kernels.hip), while
rthx_smooth_F builds it on the host from the CSR it is given.  X is fixed to
the bit and every AP reduction runs in a fixed order, so the two smoothing
results are held bit-equal: indptr, indices and the bytes of data.

Sparsity by construction: a row holds at most R entries, so the density is at
most R / N < 1/4 in every sparse case here.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import helpers as H

pytestmark = pytest.mark.gpu


def _trace(hip, dom, R, seed=2):
    flat = dom.flat()
    args, _k = hip.make_args(0, R, H.NUDGE, seed, 0, flat.n_emitters, 1)
    dd = hip.DeviceDomain(flat, 0)
    res = hip.DeviceResult()
    res.trace(dd, args)
    return dd, res, flat.n_emitters


def _build(hip, handle):
    on, ms = C.c_int32(-1), C.c_double(-1.0)
    assert hip.load().rthx_smooth_get_build(handle.handle, C.byref(on), C.byref(ms)) == 0
    return on.value, ms.value


def _both_routes(hip, dom, res, N, n):
    """(host-route result, its handle, device-route result, its handle) of one
    trace's leading n x n block with the same weights."""
    from rthx.smoothing import get_w, smooth_F, smooth_F_device

    rp, cols, vals = res.F()
    F = sp.csr_matrix((vals, cols, rp), shape=(N, N))[:n, :n].tocsr()
    w = get_w(dom)
    i_host, i_dev = {}, {}
    A, ha = smooth_F(F, w, dom.num_surfaces, verbose=False, info=i_host, keep_device=True)
    hb = smooth_F_device(res, n, w, dom.num_surfaces, verbose=False, info=i_dev)
    B = hb.host()
    assert sp.issparse(A) and sp.issparse(B) and not i_host["dense"] and not i_dev["dense"]
    assert i_dev["x_on_device"] == 1 and i_host["x_on_device"] == 0
    assert i_dev["x_build_ms"] > 0.0 and i_dev["x_build_ms"] <= i_dev["ms_ap"]
    assert _build(hip, hb)[0] == 1 and _build(hip, ha)[0] == 0
    assert i_host["ap_iters"] == i_dev["ap_iters"]
    return A, ha, B, hb


def _assert_same_bytes(A, B):
    assert A.shape == B.shape
    assert np.array_equal(A.indptr, B.indptr)
    assert np.array_equal(A.indices, B.indices)
    diff = np.max(np.abs(A.data - B.data)) if A.nnz else 0.0
    print(f"n = {A.shape[0]}, nnz = {A.nnz}: max |host - device| = {diff:.3g}")
    assert np.array_equal(A.data.view(np.uint64), B.data.view(np.uint64))


@pytest.fixture(scope="module")
def scatter25(hip):
    """square_domain(25, sigma_s = 5) at R = 150: N = 725, density <= 0.21."""
    dom = H.square_domain(25, sigma_s=5.0)
    dd, res, N = _trace(hip, dom, 150)
    assert N == 725
    yield dom, res, N
    res.close()
    dd.close()


def test_square12_whole_matrix(hip):
    dom = H.square_domain(12, sigma_s=5.0)
    dd, res, N = _trace(hip, dom, 30)  # N = 192, density <= 0.16
    try:
        assert N == 192
        A, ha, B, hb = _both_routes(hip, dom, res, N, N)
        ha.close()
        hb.close()
    finally:
        res.close()
        dd.close()
    _assert_same_bytes(A, B)


@pytest.mark.parametrize("n", [725, 400])
def test_square25_whole_and_leading_block(hip, scatter25, n):
    """n = 400 cuts every row that reaches past column 399: the block keeps a
    prefix of each row (tp::Source with src != off)."""
    dom, res, N = scatter25
    A, ha, B, hb = _both_routes(hip, dom, res, N, n)
    ha.close()
    hb.close()
    assert A.shape == (n, n)
    _assert_same_bytes(A, B)


def test_grey_solve_on_both_handles_is_bit_equal(hip, scatter25):
    from rthx import abi

    dom, res, N = scatter25
    A, ha, B, hb = _both_routes(hip, dom, res, N, N)
    lib = hip.load()
    rng = np.random.default_rng(3)
    co = rng.uniform(0.05, 0.95, N)
    h = rng.uniform(0.0, 2.0, N)
    out = []
    try:
        for handle in (ha, hb):
            a = abi.SolveArgs()
            a.device, a.memory, a.itmax, a.rtol, a.atol = 0, 50, 0, 1e-12, 1e-8
            j, g = np.full(N, np.nan), np.full(N, np.nan)
            info = abi.SolveInfo()
            dp = C.c_double
            rc = lib.rthx_solve_grey_smoothed(handle.handle, abi.ptr(co, dp), abi.ptr(h, dp), C.byref(a),
                                              abi.ptr(j, dp), abi.ptr(g, dp), C.byref(info))
            assert rc == abi.RTHX_OK, lib.rthx_last_error()
            assert np.all(np.isfinite(j)) and np.all(np.isfinite(g))
            out.append((j, g))
    finally:
        ha.close()
        hb.close()
    (j0, g0), (j1, g1) = out
    assert np.array_equal(j0.view(np.uint64), j1.view(np.uint64))
    assert np.array_equal(g0.view(np.uint64), g1.view(np.uint64))


def test_dense_result_reports_no_device_build(hip):
    from rthx.smoothing import get_w, smooth_F_device

    dom = H.square_domain(11)
    dd, res, N = _trace(hip, dom, 6000)
    try:
        info = {}
        h = smooth_F_device(res, N, get_w(dom), dom.num_surfaces, verbose=False, info=info)
        on, ms = _build(hip, h)
        h.close()
    finally:
        res.close()
        dd.close()
    assert info["dense"] and info["x_on_device"] == 0 and on == 0 and ms == 0.0


def test_mesh_builds_sparse_x_on_device(hip):
    dom = H.square_domain(12, sigma_s=5.0)
    assert dom(30 * 192, seed=5, verbose=False) is None
    assert dom.last_smooth_info["dense"] == 0
    assert dom.last_smooth_info["x_on_device"] == 1
    assert dom.last_smooth_info["x_build_ms"] > 0.0
