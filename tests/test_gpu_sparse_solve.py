"""GERT solves on sparse, device-resident F: F' is formed on
the device by the transpose kernels (csrc/rthx_transpose_kernels.hip) from a
trace result's counts (rthx_solve_grey_result) or from a sparse smoothing
result's CSR (rthx_solve_grey_smoothed, rthx_solve_spectral,
rthx_spectral_apply), and the existing operators run on it.

The independent check is the host route: the same matrix copied to the host
and handed back as CSR, which rthx_solve_grey / rthx_solve_spectral transpose
on one CPU thread.  Both routes hand the operator the same arrays, so the
results are expected to be bit-equal (printed); asserted are the bars of the
tests these mirror: same_T of tests/test_gpu_solve.py (1e-9 relative), and
between device and host forms of the spectral calls the bars of
tests/test_gpu_spectral_solve.py (apply 1e-12 of max |y|, j rtol / atol
1e-10, T 1e-6 K).
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import helpers as H
import spectral_ref as R

pytestmark = pytest.mark.gpu

DP = C.c_double


def same_T(T, T0):
    """tests/test_gpu_solve.py same_T: 1e-9 relative where the element emits,
    T^4 to (1 K)^4 on elements held at 0 K."""
    hot = T0 > 5.0
    return bool(np.allclose(T[hot], T0[hot], rtol=1e-9, atol=0) and np.all(T[~hot] ** 4 < 1.0 + T0[~hot] ** 4))


def grey_T(dom, F):
    from rthx.equilibrium import equilibrium_grey

    info = {}
    T, j, Abs, r = equilibrium_grey(dom, F, info=info)
    assert info["converged"] == 1
    return T, j, Abs + r, info


# --------------------------------------------------------------------------
# solve from a raw trace
# --------------------------------------------------------------------------
@pytest.mark.parametrize("block", ["all_emitters", "surfaces_only"])
def test_solve_from_device_counts(hip, block):
    from rthx.exchange import DeviceF, exchange_ray_tracing

    dom = H.square_domain(11) if block == "all_emitters" else H.square_domain(11, kappa=0.0, epsilon=0.6)
    assert dom.surfaces_only == (block == "surfaces_only")
    exchange_ray_tracing(dom, 1_000_000, H.NUDGE, False, None, seed=3, lazy=True)
    Fdev = dom.F_raw_device()
    assert isinstance(Fdev, DeviceF)
    n = dom.num_surfaces + (0 if dom.surfaces_only else dom.num_volumes)
    T, j, g, info = grey_T(dom, Fdev)
    assert info["F_form"] == "result" and info["n"] == n
    err = dom.energy_error
    Fh = Fdev.host()  # rthx_result_copy_F: all N rows and columns
    assert Fh.shape == (dom.num_emitters,) * 2
    Th, jh, gh, info_h = grey_T(dom, Fh)
    assert info_h["F_form"] == "host_csr"
    print(f"{block}: j bit-equal {np.array_equal(j, jh)}, g bit-equal {np.array_equal(g, gh)}, "
          f"max |dT| {np.max(np.abs(T - Th)):.3e}, iterations {info['iterations']} / {info_h['iterations']}")
    assert same_T(T, Th)
    ns = dom.num_surfaces
    Tw0, Tg0, err0 = H.solve_grey(dom, Fh[:n, :n].tocsr())
    T0 = np.concatenate([Tw0, Tg0])[:n]
    hot = T0 > 5.0
    print(f"{block} against the direct solve: max rel dT (hot) {np.max(np.abs(T[hot] / T0[hot] - 1.0)):.3e}, "
          f"max T (cold) {np.max(T[~hot], initial=0.0):.3e} / {np.max(T0[~hot], initial=0.0):.3e}, "
          f"residual {info['residual']:.3e} of tolerance {info['tolerance']:.3e}")
    if block == "all_emitters":  # (the checks of test_sparse_F_raw_matches_direct_solve)
        assert same_T(T[:ns], Tw0) and same_T(T[ns:], Tg0)
        assert abs(err) < 1e-4 and abs(err0) < 1e-4
    else:
        # The surfaces-only block is held against the host-CSR solve above.
        # Against the direct solve only the emitting walls are compared: a wall
        # held at 0 K has e = j - r at GMRES's residual (1.2e-8 W of a
        # tolerance of 2.5e-8), and T = (e / (eps sigma A))^(1/4) with
        # eps sigma A = 3.1e-9 W/K^4 turns that into about 1 K on either route
        # (1.03 K measured, the same on both), past same_T's (1 K)^4.
        assert np.allclose(T[hot], T0[hot], rtol=1e-9, atol=0)


def test_sharded_and_multi_device_results_are_refused(hip):
    from rthx import abi

    lib = hip.load()
    dom = H.square_domain(5)
    flat = dom.flat()
    N = flat.n_emitters
    co, h, j, g = np.full(N, 0.5), np.ones(N), np.empty(N), np.empty(N)
    a = abi.SolveArgs()
    a.device, a.memory, a.itmax, a.rtol, a.atol = 0, 50, 0, 1e-12, 1e-8
    ptrs = (abi.ptr(co, DP), abi.ptr(h, DP), C.byref(a), abi.ptr(j, DP), abi.ptr(g, DP), None)
    dd = hip.DeviceDomain(flat, 0)
    md = hip.MultiDeviceDomain(flat, [0, 0])
    res = hip.DeviceResult()
    try:
        args, _k = hip.make_args(0, 500, H.NUDGE, 1, 1, N, 3)  # rows 1, 4, 7, ...
        res.trace(dd, args)
        assert lib.rthx_solve_grey_result(res.handle, N, *ptrs) == abi.RTHX_EINVAL
        assert b"every emitter row" in lib.rthx_last_error()
        args, _k = hip.make_args(0, 500, H.NUDGE, 1, 0, N, 1)
        res.trace(md, args)
        assert lib.rthx_solve_grey_result(res.handle, N, *ptrs) == abi.RTHX_EINVAL
        assert b"single-device" in lib.rthx_last_error()
        # a whole single-device trace: n beyond its rows is refused, n = N solves
        res.trace(dd, args)
        assert lib.rthx_solve_grey_result(res.handle, N + 1, *ptrs) == abi.RTHX_EINVAL
        info = abi.SolveInfo()
        assert lib.rthx_solve_grey_result(res.handle, N, *ptrs[:-1], C.byref(info)) == abi.RTHX_OK
        assert info.converged == 1 and info.n == N
    finally:
        res.close()
        md.close()
        dd.close()


# --------------------------------------------------------------------------
# solve from a sparse smoothing result; the domain level
# --------------------------------------------------------------------------
_SPARSE41 = {}


def sparse41():
    """H.square_domain(41) traced and smoothed on the device at 200 000 rays
    (density ~ 6 %: the smoothing result is sparse), once for the tests below."""
    if not _SPARSE41:
        dom = H.square_domain(41)
        dom(200_000, seed=5, verbose=False)
        handle = dom.F_smooth_handle()
        assert handle is not None and not handle.dense
        assert dom.F_smooth_device() is None  # (the dense-only accessor keeps its contract)
        _SPARSE41.update(dom=dom, handle=handle, F0=handle.host())
    return _SPARSE41


def test_grey_solve_on_sparse_smoothing_result(hip):
    c = sparse41()
    dom, handle, F0 = c["dom"], c["handle"], c["F0"]
    n = F0.shape[0]
    assert sp.issparse(F0) and F0.nnz / n ** 2 < 0.25
    T, j, g, info = grey_T(dom, None)  # dom.F_smooth, where it lies
    assert info["F_form"] == "smoothed_sparse"
    Th, jh, gh, info_h = grey_T(dom, F0.copy())
    assert info_h["F_form"] == "host_csr"
    print(f"n {n}, nnz {F0.nnz}: j bit-equal {np.array_equal(j, jh)}, g bit-equal {np.array_equal(g, gh)}, "
          f"max |dT| {np.max(np.abs(T - Th)):.3e}")
    assert same_T(T, Th)
    # the handle's own CSR is as it was
    F1 = handle.host()
    assert np.array_equal(F1.indptr, F0.indptr) and np.array_equal(F1.indices, F0.indices)
    assert np.array_equal(F1.data, F0.data)
    # a second solve reads the F' kept in the handle
    T2, j2, _, _ = grey_T(dom, None)
    assert np.array_equal(j2, j)


def test_domain_level_solve_takes_the_sparse_handle(hip):
    from rthx.equilibrium import solve_equilibrium

    c = sparse41()
    dom, F0 = c["dom"], c["F0"]
    T, j, Abs, r = solve_equilibrium(dom)
    assert dom.last_solve_info["F_form"] == "smoothed_sparse"  # no host CSR was passed
    assert dom.last_solve_info["converged"] == 1
    Th, _, _, _ = solve_equilibrium(dom, F0.copy())
    assert dom.last_solve_info["F_form"] == "host_csr"
    assert same_T(T, Th)
    # dom.F_smooth itself (the host copy of the handle) is recognised too
    T3, _, _, _ = solve_equilibrium(dom, dom.F_smooth)
    assert dom.last_solve_info["F_form"] == "smoothed_sparse" and np.array_equal(T3, T)


# --------------------------------------------------------------------------
# spectral calls on sparse handles
# --------------------------------------------------------------------------
def _sparse_handles(seeds):
    """Sparse smoothing results of H.square_domain(17) (n = 357) traced with
    30 rays per emitter, one per seed, and their host CSR."""
    from rthx._lib import HipBackend
    from rthx.smoothing import get_w, smooth_F_device

    dom = H.square_domain(17, epsilon=0.6)
    n = dom.num_emitters
    out = []
    for seed in seeds:
        _F, _info, _rays, res = HipBackend().trace_F(dom, 0, 30, H.NUDGE, seed, 0, False, host=False)
        try:
            h = smooth_F_device(res, n, get_w(dom), dom.num_surfaces, verbose=False)
        finally:
            res.close()
        assert not h.dense
        out.append((h, h.host()))
    return dom, n, out


def _bands(mats, n, handles):
    from rthx import abi
    from rthx.equilibrium import _band_struct

    keep = []
    arr = (abi.SpectralBand * len(mats))(*[_band_struct(m, n, h, keep) for m, h in zip(mats, handles)])
    return arr, keep


@pytest.mark.parametrize("form", ["shared", "per_band"])
def test_spectral_calls_on_sparse_handles(hip, form):
    from rthx import abi
    from rthx._lib import check
    from rthx.equilibrium import solve_spectral

    lib = hip.load()
    K = 2
    dom, n, hs = _sparse_handles([21] if form == "shared" else [21, 22])
    handles = [h for h, _ in hs]
    mats = [F for _, F in hs]
    try:
        rng = np.random.default_rng(len(form))
        x, b, f = rng.standard_normal((K, n)), rng.random((K, n)), rng.random((K, n))
        radeq = (rng.random(n) < 0.5).astype(np.uint8)
        out = {}
        for route, (mm, hh) in {"device": ([None] * len(mats), handles), "host": (mats, [None] * len(mats))}.items():
            bands, keep = _bands(mm, n, hh)
            g, y = np.empty((K, n)), np.empty((K, n))
            check(lib.rthx_spectral_apply(bands, len(mm), n, K, 0, abi.ptr(x, DP), abi.ptr(b, DP), abi.ptr(f, DP),
                                          abi.ptr(radeq, C.c_uint8), abi.ptr(g, DP), abi.ptr(y, DP)))
            out[route] = (g, y)
            del keep
        (g, y), (g0, y0) = out["device"], out["host"]
        print(f"{form}: apply g bit-equal {np.array_equal(g, g0)}, y bit-equal {np.array_equal(y, y0)}")
        assert np.max(np.abs(g - g0)) <= 1e-12 * np.max(np.abs(g0))
        assert np.max(np.abs(y - y0)) <= 1e-12 * np.max(np.abs(y0))
        # against numpy too (the bar of test_banded_apply_matches_numpy)
        D = [R.dense(m) for m in mats]
        g_np = np.array([D[k if len(D) > 1 else 0].T @ x[k] for k in range(K)])
        assert np.max(np.abs(g - g_np)) <= 1e-12 * np.max(np.abs(g_np))

        # the solve: two bands with different reflectivities over the grey domain's elements
        b1, prop1, size, T_in, q_in = R.domain_arrays(dom)
        bb = np.vstack([b1[0], np.clip(b1[0] + 0.25, 0.0, 1.0)])
        prop = np.vstack([prop1[0], 0.7 * prop1[0]])
        limits = np.array([1e-7, 3e-6, 1e-2])
        Fd = [None] * len(mats)
        jd, gd, Td, ed, info_d = solve_spectral(Fd if len(Fd) > 1 else Fd[0], limits, bb, prop, size, T_in, q_in,
                                                handles=handles)
        jh, gh, Th, eh, info_h = solve_spectral(mats if len(mats) > 1 else mats[0], limits, bb, prop, size, T_in,
                                                q_in)
        print(f"{form}: solve j bit-equal {np.array_equal(jd, jh)}, max |dT| {np.max(np.abs(Td - Th)):.3e}, "
              f"outer {info_d['outer_iterations']} / {info_h['outer_iterations']}")
        assert info_d["converged"] == 1 and info_h["converged"] == 1
        assert np.max(np.abs(Td - Th)) <= 1e-6
        np.testing.assert_allclose(jd, jh, rtol=1e-10, atol=1e-10)
        # the handles' own CSR is as it was
        for h, F0 in hs:
            F1 = h.host()
            assert np.array_equal(F1.indptr, F0.indptr) and np.array_equal(F1.indices, F0.indices)
            assert np.array_equal(F1.data, F0.data)
    finally:
        for h in handles:
            h.close()
