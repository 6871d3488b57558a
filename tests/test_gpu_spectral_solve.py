"""Spectral GERT solve on the device (rthx_solve_spectral, rthx.equilibrium;
DESIGN.md §7f): the two kernels alone against numpy, the solve against the
grey device solve where the two must coincide, against isothermal enclosures,
against the numpy restatement of the reference's iteration
(tests/spectral_ref.py), against its own equations, and the host layer.

Tolerances.  Kernels: 1e-12 of max |y| (fp64 sums in another order, the bar of
tests/test_gpu_smooth.py); Planck fractions 1e-13 absolute (a 100-term sum of
terms <= 1 with an exp good to an ulp).  Solves: the reference's own bars --
shared-F grey vs spectral 1e-4 K / rtol 1e-4 (test_shared_F_grey_vs_spectral.jl),
isothermal 1e-3 K (test_spectral_isothermal.jl), deterministic comparisons
1e-6 K and rtol 1e-8 (test_3d_mixed_eps_grey_vs_spectral.jl:35-36), energy
error 1e-6 W.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

import helpers as H
import spectral_ref as R

pytestmark = pytest.mark.gpu

DP = C.c_double
LIMITS5 = np.logspace(-7, -2, 6)
REF3D = json.load(open(os.path.join(H.GOLDEN, "reference_3d.json")))


# --------------------------------------------------------------------------
# 1. the banded operator alone
# --------------------------------------------------------------------------
def _bands(mats, n, handles=None):
    """(ctypes array of rthx_spectral_band, keepalive) from dense arrays,
    scipy CSR matrices or SmoothHandles."""
    from rthx import abi
    from rthx.equilibrium import _band_struct

    keep = []
    hs = handles or [None] * len(mats)
    arr = (abi.SpectralBand * len(mats))(*[_band_struct(m, n, h, keep) for m, h in zip(mats, hs)])
    return arr, keep


def _apply(lib, bands, n_mats, n, K, x, b, f, radeq):
    from rthx import abi
    from rthx._lib import check

    g = np.empty((K, n))
    y = np.empty((K, n))
    check(lib.rthx_spectral_apply(bands, n_mats, n, K, 0, abi.ptr(x, DP), abi.ptr(b, DP), abi.ptr(f, DP),
                                  abi.ptr(radeq, C.c_uint8), abi.ptr(g, DP), abi.ptr(y, DP)))
    return g, y


def _apply_numpy(mats, K, x, b, f, radeq):
    D = [R.dense(m) for m in mats]
    g = np.array([D[k if len(D) > 1 else 0].T @ x[k] for k in range(K)])
    absorbed = np.sum((1.0 - b) * g, axis=0)
    return g, x - b * g - radeq[None, :] * f * absorbed[None, :]


def _sparse_band(n, rng, empty=False):
    """A CSR band with empty rows and empty columns (or no entry at all)."""
    if empty:
        return sp.csr_matrix((n, n))
    M = sp.random(n, n, density=min(1.0, 8.0 / n), random_state=np.random.RandomState(int(rng.integers(1 << 30))),
                  format="lil")
    M[::3, :] = 0.0
    M[:, 1::4] = 0.0
    M = M.tocsr()
    M.eliminate_zeros()
    return M


def _check_apply(lib, mats, n, K, rng, handles=None, ref_mats=None):
    bands, keep = _bands(mats, n, handles)
    x = rng.standard_normal((K, n))
    b = rng.random((K, n))
    f = rng.random((K, n))
    for mode in ("none", "all", "mixed"):
        radeq = {"none": np.zeros(n, np.uint8), "all": np.ones(n, np.uint8),
                 "mixed": (rng.random(n) < 0.5).astype(np.uint8)}[mode]
        g, y = _apply(lib, bands, len(mats), n, K, x, b, f, radeq)
        g0, y0 = _apply_numpy(ref_mats or mats, K, x, b, f, radeq.astype(np.float64))
        assert np.max(np.abs(g - g0)) <= 1e-12 * max(np.max(np.abs(g0)), 1e-300), mode
        assert np.max(np.abs(y - y0)) <= 1e-12 * np.max(np.abs(y0)), mode
    del keep


@pytest.mark.parametrize("K", [1, 3, 10])
@pytest.mark.parametrize("n", [1, 45, 65, 257, 1000])  # 65, 257, 1000: lane, column-tile and row-chunk remainders
@pytest.mark.parametrize("form", ["dense", "csr", "shared", "shared_csr"])
def test_banded_apply_matches_numpy(hip, form, n, K):
    lib = hip.load()
    rng = np.random.default_rng(1000 * n + 10 * K + len(form))
    if form == "dense":
        mats = [rng.random((n, n)) / n for _ in range(K)]
    elif form == "csr":
        mats = [_sparse_band(n, rng, empty=(k == 1)) for k in range(K)]
    elif form == "shared":
        mats = [rng.random((n, n)) / n]
    else:
        mats = [_sparse_band(n, rng)]
    _check_apply(lib, mats, n, K, rng)


def test_banded_apply_mixed_forms_and_empty_matrix(hip):
    """Dense and CSR bands in one operator, and an operator of empty matrices."""
    lib = hip.load()
    rng = np.random.default_rng(7)
    n, K = 257, 4
    mats = [rng.random((n, n)) / n, _sparse_band(n, rng), _sparse_band(n, rng, empty=True), rng.random((n, n)) / n]
    _check_apply(lib, mats, n, K, rng)
    _check_apply(lib, [sp.csr_matrix((n, n))], n, 3, rng)


@pytest.mark.parametrize("n", [45, 65, 257, 1000])
def test_banded_apply_on_device_resident_smoothing_result(hip, n):
    """F as a dense rthx_smooth_F result read in place: shared by K = 1, 3, 10
    bands, and once per band (n_matrices = K = 3).  (n = 1 has no smoothing
    result: nothing to smooth.)"""
    from rthx import abi
    from rthx.smoothing import smooth_F

    lib = hip.load()
    rng = np.random.default_rng(n)
    F_raw = rng.random((n, n)) + 0.05
    F_raw /= F_raw.sum(axis=1, keepdims=True)
    Fs, handle = smooth_F(F_raw, np.ones(n), n, max_iters=3, verbose=False, keep_device=True)
    try:
        assert handle.dense
        Fs = R.dense(Fs)
        for K in (1, 3, 10):
            _check_apply(lib, [None], n, K, rng, handles=[handle], ref_mats=[Fs])
        _check_apply(lib, [None] * 3, n, 3, rng, handles=[handle] * 3, ref_mats=[Fs] * 3)
        # a result on another device than the call's is refused before any launch
        bands, keep = _bands([None], n, [handle])
        x = np.ones((1, n))
        g = np.empty((1, n))
        none = C.cast(None, C.POINTER(DP))
        rc = lib.rthx_spectral_apply(bands, 1, n, 1, 1, abi.ptr(x, DP), none, none, C.cast(None, C.POINTER(C.c_uint8)),
                                     abi.ptr(g, DP), none)
        assert rc == abi.RTHX_EINVAL and b"another device" in lib.rthx_last_error()
    finally:
        handle.close()


# --------------------------------------------------------------------------
# 2. the Planck kernel alone
# --------------------------------------------------------------------------
PLANCK_T = np.array([np.nan, -1.0, 0.0, 1e-3, 3.0, 300.0, 1000.0, 5800.0, 1e6, 1e9])


@pytest.mark.parametrize("K", [1, 3, 10])
@pytest.mark.parametrize("span", [(-8, -1), (-7, -2)])
def test_planck_fractions_match_host(hip, span, K):
    from rthx import abi
    from rthx._lib import check
    from rthx.direct import bins_emission_fractions

    lib = hip.load()
    limits = np.logspace(span[0], span[1], K + 1)
    T = np.tile(PLANCK_T, 7)  # more than one wave
    n = len(T)
    rng = np.random.default_rng(K)
    prop = rng.random((K, n))
    prop[:, 3::11] = 0.0  # elements that emit nothing: the row stays prop .* w = 0
    plain = np.empty((K, n))
    weighted = np.empty((K, n))
    check(lib.rthx_spectral_fractions(abi.ptr(limits, DP), K, abi.ptr(T, DP), abi.ptr(prop, DP), n, 0,
                                      abi.ptr(plain, DP), abi.ptr(weighted, DP)))
    ref = bins_emission_fractions(limits, K, T).T
    assert np.max(np.abs(plain - ref)) <= 1e-13
    assert np.max(np.abs(plain.sum(axis=0) - 1.0)) <= 1e-15 * K
    wref = prop * ref
    s = wref.sum(axis=0)
    wref[:, s > 0] /= s[s > 0]
    assert np.max(np.abs(weighted - wref)) <= 1e-13
    # plain alone (no prop, no weighted output)
    plain2 = np.empty((K, n))
    none = C.cast(None, C.POINTER(DP))
    check(lib.rthx_spectral_fractions(abi.ptr(limits, DP), K, abi.ptr(T, DP), none, n, 0, abi.ptr(plain2, DP), none))
    assert np.array_equal(plain2, plain)


# --------------------------------------------------------------------------
# 3. shared F, grey versus spectral with non-uniform b
# --------------------------------------------------------------------------
def _all_j(dom, spectral):
    ns = dom.num_surfaces
    j = np.zeros(ns + dom.num_volumes)
    for (c, f, w), s in dom.surface_mapping.items():
        v = dom.fine_mesh[c - 1][f - 1].j_w[w - 1]
        assert (np.ndim(v) == 1) == spectral
        j[s - 1] = np.sum(v)
    for (c, f), v in dom.volume_mapping.items():
        jg = dom.fine_mesh[c - 1][f - 1].j_g
        assert (np.ndim(jg) == 1) == spectral
        j[ns + v - 1] = np.sum(jg)
    return j


def test_shared_F_grey_vs_spectral_nonuniform_b(hip):
    """test/test_shared_F_grey_vs_spectral.jl: reflecting walls (b = 0.7) and
    non-scattering volumes (b = 0), spectrally uniform properties, one traced
    F for both solves."""
    from rthx.equilibrium import equilibrium_grey, equilibrium_spectral, solve_equilibrium, solve_spectral

    K = 10
    limits = np.logspace(-8, -1, K + 1)
    grey = H.square_domain(5, kappa=1.0, sigma_s=0.0, epsilon=0.3)
    spec = R.spectral_square(5, K, 1.0, 0.3, limits=limits)
    spec(200_000, seed=11, verbose=False)
    F = spec.F_smooth
    assert isinstance(F, list) and len(F) == K and all(m is F[0] for m in F)
    _, jg, _, _ = equilibrium_grey(grey, F[0])
    info = {}
    Ts_all, js, _, _ = equilibrium_spectral(spec, F, info=info)
    assert info["converged"] == 1 and js.shape == (K, len(jg))
    ns = grey.num_surfaces
    T_grey = np.array([ff.T_g for ff in grey.fine_mesh[0]])
    T_spec = np.array([ff.T_g for ff in spec.fine_mesh[0]])
    assert np.max(np.abs(T_spec - T_grey)) < 1e-4
    assert np.array_equal(T_spec, Ts_all[ns:][[spec.volume_mapping[(1, f)] - 1 for f in range(1, 26)]])
    np.testing.assert_allclose(_all_j(spec, True), _all_j(grey, False), rtol=1e-4, atol=0)
    hot = T_grey > 1.0
    assert np.max(np.abs((T_spec[hot] / T_grey[hot]) ** 4 - 1.0)) < 1e-4
    # the same through solve_equilibrium (dispatch on spectral_mode)
    T2, j2, _, _ = solve_equilibrium(spec, F)
    assert np.array_equal(T2, Ts_all) and np.array_equal(j2, js)
    # K = 1 is the grey system itself
    b, prop, size, T_in, q_in = R.domain_arrays(grey)
    j1, g1, T1, e1, i1 = solve_spectral(F[0], np.array([1e-8, 0.1]), b, prop, size, T_in, q_in)
    assert i1["converged"] == 1
    np.testing.assert_allclose(j1[0], jg, rtol=1e-10, atol=0)


# --------------------------------------------------------------------------
# 4. isothermal enclosures
# --------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["uniform", "selective_eps_shared_F", "selective_kappa_per_band_F"])
def test_isothermal_enclosure(hip, case):
    """test/test_spectral_isothermal.jl: walls at 1000 K, the gas in radiative
    equilibrium takes 1000 K whatever the spectral properties."""
    from rthx.equilibrium import solve_equilibrium

    kappa, eps = {"uniform": (1.0, 1.0), "selective_eps_shared_F": (1.0, [0.3, 0.3, 0.3, 0.9, 0.9]),
                  "selective_kappa_per_band_F": (np.linspace(0.5, 1.5, 5), 1.0)}[case]
    dom = R.spectral_square(5, 5, kappa, eps, T_walls=(1000.0,) * 4, limits=LIMITS5)
    assert dom.spectral_mode == ("spectral_uniform" if case == "uniform" else "spectral_variable")
    dom(200_000, seed=12, verbose=False)
    if case == "uniform":
        assert dom.F_smooth_device() is not None  # read in place on the device
    elif case == "selective_eps_shared_F":
        assert all(m is dom.F_smooth[0] for m in dom.F_smooth)
    else:
        assert dom.F_smooth[0] is not dom.F_smooth[4]
    T, j, Abs, r = solve_equilibrium(dom)
    Tg = np.array([ff.T_g for ff in dom.fine_mesh[0]])
    assert np.max(np.abs(Tg - 1000.0)) < 1e-3
    assert np.max(np.abs(T[dom.num_surfaces:] - 1000.0)) < 1e-3


# --------------------------------------------------------------------------
# 5., 6., 8. against the restatement, the equations, the host layer
# --------------------------------------------------------------------------
_CASE5 = {}


def _case5(participating):
    """The mixed-boundary 5 x 5 square: traced and smoothed once, the
    restatement run once, shared by the tests below."""
    if participating not in _CASE5:
        kappa = np.linspace(0.5, 1.5, 5) if participating else 0.0
        dom = R.spectral_square(5, 5, kappa, [0.3, 0.3, 0.3, 0.9, 0.9], T_walls=(1000.0, 300.0, -1.0, 0.0),
                                q_walls=(0.0, 0.0, -100.0, 0.0), q_in_g=1250.0 if participating else 0.0,
                                limits=LIMITS5)
        assert dom.surfaces_only == (not participating)
        dom(200_000, seed=13, verbose=False)
        arrays = R.domain_arrays(dom)
        n = arrays[0].shape[1]
        assert n == (45 if participating else 20)
        q_in = arrays[4]  # -20 W per element of wall 3, 50 W per volume
        assert sorted(set(np.round(q_in, 9))) == ([-20.0, 0.0, 50.0] if participating else [-20.0, 0.0])
        assert np.sum(q_in < 0) == 5 and np.sum(q_in > 0) == n - 20
        F = [R.dense(m)[:n, :n] for m in dom.F_smooth]
        ref = R.reference_solve(F, LIMITS5, *arrays)
        _CASE5[participating] = dict(dom=dom, arrays=arrays, F=F, ref=ref, n=n, device={})
    return _CASE5[participating]


def _case5_device(participating, sparse):
    from rthx.equilibrium import solve_spectral

    c = _case5(participating)
    if sparse not in c["device"]:
        F = [sp.csr_matrix(m) for m in c["F"]] if sparse else c["F"]
        c["device"][sparse] = solve_spectral(F, LIMITS5, *c["arrays"])
    return c, c["device"][sparse]


@pytest.mark.parametrize("sparse", [False, True], ids=["dense_F", "sparse_F"])
@pytest.mark.parametrize("participating", [True, False], ids=["participating", "surfaces_only"])
def test_solve_matches_restatement(hip, participating, sparse):
    c, (j, g, T, e, info) = _case5_device(participating, sparse)
    j_ref, T_ref, e_ref, sweeps = c["ref"]
    print(f"outer {info['outer_iterations']}, gmres {info['gmres_iterations']}, restatement sweeps {sweeps}, "
          f"max |dT| {np.max(np.abs(T - T_ref)):.3e}, max |dj| {np.max(np.abs(j - j_ref)):.3e}, "
          f"max rel dj {np.max(np.abs(j - j_ref) / np.abs(j_ref)):.3e}, min |j| {np.min(np.abs(j_ref)):.3e}")
    assert info["converged"] == 1
    assert info["outer_iterations"] < 60
    assert np.max(np.abs(T - T_ref)) <= 1e-6
    np.testing.assert_allclose(j, j_ref, rtol=1e-8, atol=1e-8)


@pytest.mark.parametrize("participating", [True, False], ids=["participating", "surfaces_only"])
def test_returned_state_satisfies_the_equations(hip, participating):
    c, (j, g, T, e, info) = _case5_device(participating, False)
    b, prop, size, T_in, q_in = c["arrays"]
    F = c["F"]
    K = 5
    Rset = T_in <= -0.1
    g0 = np.array([F[k].T @ j[k] for k in range(K)])
    f = R.weighted_fractions(LIMITS5, T, prop)
    for k in range(K):
        res = np.linalg.norm(j[k] - b[k] * g0[k] - e * f[k])
        print(f"band {k}: residual {res:.3e} of ||e|| {np.linalg.norm(e):.3e}")
        assert res <= 1e-9 * np.linalg.norm(e)
    bal = np.abs(e - q_in - np.sum((1.0 - b) * g0, axis=0))[Rset]
    print(f"balance on R: {bal.max():.3e} of max e {e.max():.3e}")
    assert np.max(bal) <= 1e-9 * np.max(e)
    # e = size sigma T^4 sum_k prop_k w_k(T) on every element
    w = R.plain_fractions(LIMITS5, T)
    e_T = size * H.STEFAN_BOLTZMANN * T ** 4 * np.sum(prop * w, axis=0)
    np.testing.assert_allclose(e[Rset], e_T[Rset], rtol=1e-9)
    np.testing.assert_allclose(e[~Rset], e_T[~Rset], rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("participating", [True, False], ids=["participating", "surfaces_only"])
def test_host_layer_writes_results(hip, participating):
    """Per band j = e + r up to the clamp e = max(j - r, 0)
    (writeResultsToDomainSpectralBin!): j - r = j - b g equals e f >= 0 to the
    residual of the last linear solve, which is below its tolerance
    (info["tolerance"] = atol + rtol ||rhs||), so that is the bound."""
    from rthx.equilibrium import equilibrium_spectral

    c = _case5(participating)
    dom = c["dom"]
    info = {}
    info_T, j, Abs, r = equilibrium_spectral(dom, info=info)
    assert info["converged"] == 1 and info["residual"] <= info["tolerance"] < 1e-7
    K = 5
    assert len(dom.energy_error) == K and max(abs(v) for v in dom.energy_error) < 1e-6
    q_prescribed = 0.0
    for (cc, f, w), s in dom.surface_mapping.items():
        face = dom.fine_mesh[cc - 1][f - 1]
        k = w - 1
        for name in ("j_w", "g_a_w", "e_w", "r_w", "g_w", "i_w"):
            assert len(getattr(face, name)[k]) == K, name
        np.testing.assert_allclose(face.j_w[k], face.e_w[k] + face.r_w[k], rtol=1e-12, atol=info["tolerance"])
        np.testing.assert_allclose(face.g_w[k], face.g_a_w[k] + face.r_w[k], rtol=1e-15)
        if face.T_in_w[k] > -0.1:
            assert face.T_w[k] == face.T_in_w[k]
            q_prescribed += face.q_w[k]
        else:
            assert face.q_w[k] == face.q_in_w[k] and face.T_w[k] == info_T[s - 1]
    if participating:
        for (cc, f), v in dom.volume_mapping.items():
            face = dom.fine_mesh[cc - 1][f - 1]
            for name in ("j_g", "g_a_g", "e_g", "r_g", "g_g", "i_g"):
                assert len(getattr(face, name)) == K, name
            np.testing.assert_allclose(face.j_g, face.e_g + face.r_g, rtol=1e-12, atol=info["tolerance"])
            assert face.q_g == face.q_in_g and face.T_g == info_T[dom.num_surfaces + v - 1]
    q_radeq = -100.0 + (1250.0 if participating else 0.0)
    assert abs(q_prescribed + q_radeq) < 1e-6
    # the device result is the one of the direct call on the same matrices
    _, (j0, g0, T0, e0, _) = _case5_device(participating, False)
    np.testing.assert_allclose(j, j0, rtol=1e-10, atol=1e-10)


def test_spectral_domain_without_band_limits_raises(hip):
    from rthx.equilibrium import solve_equilibrium

    dom = R.spectral_square(3, 5, 1.0, [0.3, 0.3, 0.3, 0.9, 0.9])
    F = np.full((21, 21), 1.0 / 21)
    with pytest.raises(ValueError, match="band limits"):
        solve_equilibrium(dom, F)
    dom.wavelength_band_limits = [1e-6, 2e-6, 3e-6]
    with pytest.raises(ValueError, match="at least 4"):
        solve_equilibrium(dom, F)
    dom.wavelength_band_limits = [1e-6, 2e-6, 2e-6, 3e-6, 4e-6, 5e-6]
    with pytest.raises(ValueError, match="strictly increasing"):
        solve_equilibrium(dom, F)
    dom.wavelength_band_limits = [-1e-6, 2e-6, 2.5e-6, 3e-6, 4e-6, 5e-6]
    with pytest.raises(ValueError, match="positive"):
        solve_equilibrium(dom, F)


# --------------------------------------------------------------------------
# 7. 3D enclosures
# --------------------------------------------------------------------------
def _cube(epsilon, T_in_w=(1000.0, 300.0, -1.0, -1.0, -1.0, -1.0), limits=None):
    from rthx import ViewFactorDomain3D

    dom = ViewFactorDomain3D(REF3D["cube_points"], REF3D["cube_faces"], 4, [0.0] * 6, list(T_in_w), epsilon)
    if limits is not None:
        dom.wavelength_band_limits = np.asarray(limits)
    dom()
    return dom


LIMITS3 = [1e-6, 3e-6, 8e-6, 1e-3]


def test_3d_mixed_epsilon_grey_vs_spectral(hip):
    """test/test_3d_mixed_eps_grey_vs_spectral.jl: bin-uniform epsilon, so the
    spectral problem is the grey problem partitioned."""
    from rthx.equilibrium import solve_equilibrium

    eps = [0.3, 0.3, 0.3, 0.9, 0.9, 0.9]
    grey = _cube(list(eps))
    solve_equilibrium(grey)
    spec = _cube([np.full(3, e) for e in eps], limits=LIMITS3)
    assert spec.spectral_mode != "grey" and np.array_equal(spec.F_smooth, grey.F_smooth)
    T, j, Abs, r = solve_equilibrium(spec)
    assert j.shape == (3, 96)
    Tg = np.array([s.T_w for s in grey.subfaces()])
    Ts = np.array([s.T_w for s in spec.subfaces()])
    assert np.max(np.abs(Ts - Tg)) < 1e-6
    jg = np.array([s.j_w for s in grey.subfaces()])
    js = np.array([np.sum(s.j_w) for s in spec.subfaces()])
    np.testing.assert_allclose(js, jg, rtol=1e-8, atol=0)
    eg = np.array([s.e_w for s in grey.subfaces()])
    es = np.array([np.sum(s.e_w) for s in spec.subfaces()])
    np.testing.assert_allclose(es[eg > 1e-8], eg[eg > 1e-8], rtol=1e-6, atol=0)
    assert max(abs(v) for v in spec.energy_error) < 1e-6


def test_3d_selective_epsilon_matches_restatement(hip):
    from rthx.equilibrium import equilibrium_surfaces_spectral_3d, solve_equilibrium

    eps = [np.array([0.3, 0.6, 0.9]), np.array([0.9, 0.5, 0.2]), np.array([0.4, 0.4, 0.8]), np.full(3, 0.9),
           np.full(3, 0.9), np.full(3, 0.9)]
    dom = _cube(eps, limits=LIMITS3)
    assert dom.spectral_mode == "spectral_variable"
    info = {}
    T, j, Abs, r = equilibrium_surfaces_spectral_3d(dom, dom.F_smooth, info=info)
    subs = dom.subfaces()
    e3 = np.array([s.epsilon for s in subs]).T.copy()
    area = np.array([s.area for s in subs])
    T_in = np.array([s.T_in_w for s in subs])
    j_ref, T_ref, e_ref, sweeps = R.reference_solve(dom.F_smooth, np.array(LIMITS3), 1.0 - e3, e3, area, T_in,
                                                    np.zeros(len(subs)))
    print(f"outer {info['outer_iterations']}, gmres {info['gmres_iterations']}, restatement sweeps {sweeps}, "
          f"max |dT| {np.max(np.abs(T - T_ref)):.3e}, max |dj| {np.max(np.abs(j - j_ref)):.3e}")
    assert info["converged"] == 1 and info["outer_iterations"] < 60
    assert np.max(np.abs(T - T_ref)) <= 1e-6
    np.testing.assert_allclose(j, j_ref, rtol=1e-8, atol=1e-8)
    T2, j2, _, _ = solve_equilibrium(dom)
    assert np.array_equal(T2, T) and np.array_equal(j2, j)
