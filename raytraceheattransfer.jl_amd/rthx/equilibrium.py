"""Grey and spectral GERT solves on the MI355X.

Host mirror of equilibriumGrey2D! (src/HeatTransfer/equilibrium/
equilibriumGrey2D.jl:80-211) with populateWorkspace!
(WorkspaceStructs.jl:68-118) and writeResultsToDomainGrey!
(writeResults/writeResultsToDomain3D.jl:112-144).  The linear system
(I - Diagonal(coeff) F') j = h and g = F' j run in librthx (rthx_solve_grey*,
restarted GMRES on the device); element bookkeeping stays on the host as in
the reference.  Spectral domains: equilibrium_spectral and
equilibrium_surfaces_spectral_3d (rthx_solve_spectral: the outer loop on the
emission fractions runs in librthx too).  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np
import scipy.sparse as sp

from . import abi
from ._lib import check, load

STEFAN_BOLTZMANN = 5.670374419e-8  # src/RayTraceHeatTransfer.jl:20


def populate_workspace(dom, spectral_bin: int = 1) -> dict:
    """populateWorkspace! (WorkspaceStructs.jl:68-118): per-element properties in
    global order (surfaces in (coarse, fine, wall) order, then volumes)."""
    b = spectral_bin - 1
    ns = len(dom.surface_mapping)
    nv = 0 if dom.surfaces_only else len(dom.volume_mapping)
    ws = {k: np.zeros(ns) for k in ("Area", "epsw", "Tw", "qw")}
    ws.update({k: np.zeros(nv) for k in ("Volume", "kappa_g", "omega_g", "Tg", "qg")})
    ws["Qw_known"] = np.zeros(ns, dtype=int)
    ws["Qg_known"] = np.zeros(nv, dtype=int)
    for (c, f, w), s in dom.surface_mapping.items():
        face = dom.fine_mesh[c - 1][f - 1]
        i = s - 1
        ws["Area"][i] = face.area[w - 1]
        ws["epsw"][i] = float(np.atleast_1d(face.epsilon[w - 1])[min(b, np.size(face.epsilon[w - 1]) - 1)])
        ws["Tw"][i] = face.T_in_w[w - 1]
        ws["qw"][i] = face.q_in_w[w - 1]
        ws["Qw_known"][i] = 1 if face.T_in_w[w - 1] < 0.0 else 0
    if nv:
        for (c, f), v in dom.volume_mapping.items():
            face = dom.fine_mesh[c - 1][f - 1]
            i = v - 1
            kap = float(np.atleast_1d(face.kappa_g)[min(b, np.size(face.kappa_g) - 1)])
            sig = float(np.atleast_1d(face.sigma_s_g)[min(b, np.size(face.sigma_s_g) - 1)])
            ws["Volume"][i] = face.volume
            ws["kappa_g"][i] = kap
            ws["omega_g"][i] = sig / (kap + sig) if kap + sig > 0.0 else 0.0
            ws["Tg"][i] = face.T_in_g
            ws["qg"][i] = face.q_in_g
            ws["Qg_known"][i] = 1 if face.T_in_g < 0.0 else 0
    return ws


def _solve(F, coeff, h, device, info, rtol=1e-12, atol=math.sqrt(np.finfo(np.float64).eps), memory=50,
           handle=None, result=None):
    """(I - Diagonal(coeff) F') j = h and g = F' j on the device.  F: a
    SmoothHandle (`handle`, dense or sparse, read in place), a trace result's
    device counts (`result`: the leading len(h) block of its F_raw,
    rthx_solve_grey_result), a scipy sparse matrix or a dense array.  `info`
    receives rthx_solve_info and ``F_form``: which of these was passed."""
    lib = load()
    n = len(h)
    a = abi.SolveArgs()
    a.device, a.memory, a.itmax, a.rtol, a.atol = device, memory, 0, rtol, atol
    co = np.ascontiguousarray(coeff, dtype=np.float64)
    hh = np.ascontiguousarray(h, dtype=np.float64)
    j = np.empty(n)
    g = np.empty(n)
    inf = abi.SolveInfo()
    dp = C.c_double
    if handle is not None:
        form = "smoothed_dense" if handle.dense else "smoothed_sparse"
        check(lib.rthx_solve_grey_smoothed(handle.handle, abi.ptr(co, dp), abi.ptr(hh, dp), C.byref(a),
                                           abi.ptr(j, dp), abi.ptr(g, dp), C.byref(inf)))
    elif result is not None:
        form = "result"
        check(lib.rthx_solve_grey_result(result.handle, n, abi.ptr(co, dp), abi.ptr(hh, dp), C.byref(a),
                                         abi.ptr(j, dp), abi.ptr(g, dp), C.byref(inf)))
    elif sp.issparse(F):
        form = "host_csr"
        Fc = F.tocsr()
        rp = np.ascontiguousarray(Fc.indptr, dtype=np.int64)
        ci = np.ascontiguousarray(Fc.indices, dtype=np.int32)
        vv = np.ascontiguousarray(Fc.data, dtype=np.float64)
        check(lib.rthx_solve_grey(abi.ptr(rp, C.c_int64), abi.ptr(ci, C.c_int32), abi.ptr(vv, dp), None, n,
                                  abi.ptr(co, dp), abi.ptr(hh, dp), C.byref(a), abi.ptr(j, dp), abi.ptr(g, dp),
                                  C.byref(inf)))
    else:
        form = "host_dense"
        Fd = np.ascontiguousarray(F, dtype=np.float64)
        check(lib.rthx_solve_grey(None, None, None, abi.ptr(Fd, dp), n, abi.ptr(co, dp), abi.ptr(hh, dp),
                                  C.byref(a), abi.ptr(j, dp), abi.ptr(g, dp), C.byref(inf)))
    if info is not None:
        info.update(inf.as_dict())
        info["F_form"] = form
    return j, g


def equilibrium_grey(dom, F, spectral_bin: int = 1, device: int = 0, verbose: bool = False,
                     info: Optional[dict] = None):
    """equilibriumGrey2D! (equilibriumGrey2D.jl:80-211).  Writes T_w, j_w,
    g_a_w, e_w, r_w, g_w, q_w, i_w (walls) and T_g, j_g, ... (volumes) into the
    fine faces, sets dom.energy_error, and returns (T, j, Abs, r) in global
    element order.  F: None (dom.F_smooth, read in place on the device when it
    lives there, dense or sparse), a DeviceF (the lazy F_raw of
    exchange_ray_tracing: solved from its device counts), a scipy sparse
    matrix or a dense array."""
    from .exchange import DeviceF

    ws = populate_workspace(dom, spectral_bin)
    ns = len(ws["Area"])
    nv = len(ws["Volume"])
    n = ns + nv
    # :4-40 emissive powers / known heat sources
    Q_known = np.concatenate([ws["Qw_known"], ws["Qg_known"]])
    E = np.zeros(n)
    Q = np.zeros(n)
    for i in range(ns):
        if Q_known[i] == 0:
            E[i] = ws["epsw"][i] * STEFAN_BOLTZMANN * ws["Area"][i] * ws["Tw"][i] ** 4
        else:
            Q[i] = ws["qw"][i]
    for v in range(nv):
        i = ns + v
        if Q_known[i] == 0:
            E[i] = 4 * ws["kappa_g"][v] * STEFAN_BOLTZMANN * ws["Volume"][v] * ws["Tg"][v] ** 4
        else:
            Q[i] = ws["qg"][v]
    # :105-127 reflectivity / scattering albedo
    b = np.zeros(n)
    if np.any(ws["omega_g"] > 1e-6) or np.sum(ws["epsw"]) < n:
        b[:ns] = 1.0 - ws["epsw"]
        b[ns:] = ws["omega_g"]
    # :136-156 right-hand side and M = I - Diagonal(coeff) F'
    h = np.where(Q_known == 1, Q, E)
    coeff = np.where(Q_known == 1, 1.0, b)
    Fm = F
    handle = None
    result = None
    dev = getattr(dom, "_F_smooth_device", None)
    if F is None:  # dom.F_smooth: read in place on the device when it lives there
        if dom.F_smooth_handle() is not None:
            handle = dom.F_smooth_handle()
        else:
            F = Fm = dom.F_smooth
    if handle is not None:
        pass
    elif isinstance(F, DeviceF):  # F_raw's counts, where the trace left them
        result, Fm = F.res, None
        device = result.device
    elif dev is not None and dev[0] is F:
        handle = dev[1]
    elif sp.issparse(F):
        Fm = F.tocsr()[:n, :n]
    else:
        Fm = np.asarray(F)[:n, :n]
    solve_info = {} if info is None else info
    j, g = _solve(Fm, coeff, h, device, solve_info, handle=handle, result=result)
    dom.last_solve_info = solve_info  # (F_form: which form of F the solve was handed)
    if verbose:
        print(f"GMRES: {solve_info['iterations']} iterations in {solve_info['cycles']} cycles, "
              f"residual {solve_info['residual']:.3e} (tolerance {solve_info['tolerance']:.3e})")
    # :176-201 reflected / absorbed split of the incident power g = F' j
    r = b * g
    Abs = (1.0 - b) * g
    # computeTemperaturesVariable! (:43-77)
    T = np.zeros(n)
    for i in range(ns):
        e = max(j[i] - r[i], 0.0)
        T[i] = (e / (ws["epsw"][i] * STEFAN_BOLTZMANN * ws["Area"][i])) ** 0.25 \
            if ws["epsw"][i] > 0.0 and ws["Area"][i] > 0.0 else 0.0
    for v in range(nv):
        i = ns + v
        e = max(j[i] - r[i], 0.0)
        T[i] = (e / (4 * ws["kappa_g"][v] * ws["Volume"][v] * STEFAN_BOLTZMANN)) ** 0.25 \
            if ws["kappa_g"][v] > 0.0 and ws["Volume"][v] > 0.0 else 0.0
    T = np.nan_to_num(T, nan=0.0)
    _write_results(dom, T, j, Abs, r)
    dom.energy_error = float(np.sum(j - r - Abs))
    return T, j, Abs, r


def _write_results(dom, T, j, Abs, r):
    """writeResultsToDomainGrey! (writeResultsToDomain3D.jl:112-144)."""
    ns = len(dom.surface_mapping)
    for (c, f, w), s in dom.surface_mapping.items():
        face = dom.fine_mesh[c - 1][f - 1]
        i = s - 1
        for name in ("T_w", "j_w", "g_a_w", "e_w", "r_w", "g_w", "q_w", "i_w"):
            if not isinstance(getattr(face, name, None), list):
                setattr(face, name, [0.0] * len(face.solidWalls))
        e = max(j[i] - r[i], 0.0)
        k = w - 1
        face.T_w[k] = T[i]
        face.j_w[k] = j[i]
        face.g_a_w[k] = Abs[i]
        face.e_w[k] = e
        face.r_w[k] = r[i]
        face.g_w[k] = Abs[i] + r[i]
        face.q_w[k] = e - Abs[i]
        face.i_w[k] = j[i] / (math.pi * face.area[k])
    if not dom.surfaces_only:
        for (c, f), v in dom.volume_mapping.items():
            face = dom.fine_mesh[c - 1][f - 1]
            i = ns + v - 1
            e = max(j[i] - r[i], 0.0)
            face.T_g = T[i]
            face.j_g = j[i]
            face.g_a_g = Abs[i]
            face.e_g = e
            face.r_g = r[i]
            face.g_g = Abs[i] + r[i]
            face.q_g = e - Abs[i]
            face.i_g = j[i] / (4 * math.pi * face.volume)


def solve_equilibrium(dom, F=None, device: int = 0, verbose: bool = False, max_iters: int = 1000,
                      convergence_tol: float = 1e-12):
    """solveEquilibrium! (solveEquilibrium.jl:1-26); F defaults to dom.F_smooth.
    Grey 2D domains and grey 3D surface enclosures take the grey solve (which
    ignores max_iters and convergence_tol, as the reference's does); spectral
    domains take the spectral solve."""
    from .domain3d import ViewFactorDomain3D
    from .gasbox import GasBox3D

    if isinstance(dom, GasBox3D):  # (no counterpart in the reference: DESIGN.md §7l)
        return equilibrium_gasbox(dom, device=dom.device if F is None else device, F=F, verbose=verbose)
    if isinstance(dom, ViewFactorDomain3D):  # solveEquilibrium.jl:13-22
        F3 = dom.F_smooth if F is None else F
        if dom.spectral_mode != "grey":
            return equilibrium_surfaces_spectral_3d(dom, F3, device=device, max_iters=max_iters,
                                                    convergence_tol=convergence_tol, verbose=verbose)
        return equilibrium_surfaces_grey_3d(dom, F3, device=device, verbose=verbose)
    if dom.spectral_mode != "grey":
        return equilibrium_spectral(dom, F, device=device, max_iters=max_iters, convergence_tol=convergence_tol,
                                    verbose=verbose)
    return equilibrium_grey(dom, F, device=device, verbose=verbose)


def equilibrium_gasbox(box, device: int = 0, F=None, verbose: bool = False, info: Optional[dict] = None):
    """The grey GERT solve of a GasBox3D or VoxelGasBox3D (rthx.gasbox): E, b,
    coeff and h assembled as equilibrium_grey assembles them (walls eps sigma
    A T^4, gas 4 kappa sigma V T^4, b = 1 - eps / omega; kappa and omega =
    sigma_s / beta per voxel for a VoxelGasBox3D), the system solved on the device
    from the box's device-resident F_smooth (F: a matrix to use instead).
    Writes T_w, q_w (per surface), T_g, q_g (per volume) and energy_error onto
    the box -- an element with T given keeps it and gets q = emitted -
    absorbed, one in radiative equilibrium keeps q and gets T -- and returns
    (T, j, Abs, r) in element order."""
    ns, nv = box.n_surfaces, box.n_volumes
    n = ns + nv
    area, vol = box.areas(), box.volume()
    eps, kappa = box.epsilon, box.kappa
    if np.ndim(kappa) == 0:
        omega = box.sigma_s / box.beta if box.beta > 0.0 else 0.0
        scatters = omega > 1e-6
    else:  # per voxel (omega = 0 where beta = 0)
        beta = box.beta
        omega = np.divide(box.sigma_s, beta, out=np.zeros(nv), where=beta > 0.0)
        scatters = bool(np.any(omega > 1e-6))
    T_in = np.concatenate([box.T_in_w, box.T_in_g])
    q_in = np.concatenate([box.q_in_w, box.q_in_g])
    Q_known = (T_in < 0.0).astype(int)
    size = np.concatenate([eps * area, np.broadcast_to(4.0 * kappa * vol, (nv,))])  # emission per sigma T^4
    E = np.where(Q_known == 0, size * STEFAN_BOLTZMANN * np.where(Q_known == 0, T_in, 0.0) ** 4, 0.0)
    b = np.zeros(n)
    if scatters or np.sum(eps) < n:
        b[:ns] = 1.0 - eps
        b[ns:] = omega
    h = np.where(Q_known == 1, q_in, E)
    coeff = np.where(Q_known == 1, 1.0, b)
    handle = None
    if F is None:
        handle = box.F_smooth_handle
        if handle is None:
            raise ValueError("the box has no F_smooth yet: call it (box(rays_tot)) before solve_equilibrium")
    elif sp.issparse(F):
        F = F.tocsr()[:n, :n]
    else:
        F = np.asarray(F)[:n, :n]
    solve_info = {} if info is None else info
    j, g = _solve(F, coeff, h, device, solve_info, handle=handle)
    box.last_solve_info = solve_info
    if verbose:
        print(f"GMRES: {solve_info['iterations']} iterations in {solve_info['cycles']} cycles, "
              f"residual {solve_info['residual']:.3e} (tolerance {solve_info['tolerance']:.3e})")
    r = b * g
    Abs = (1.0 - b) * g
    e = np.maximum(j - r, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        T = np.where(size > 0.0, (e / (size * STEFAN_BOLTZMANN)) ** 0.25, 0.0)
    T = np.nan_to_num(T, nan=0.0)
    T_out = np.where(Q_known == 1, T, T_in)
    q_out = np.where(Q_known == 1, q_in, e - Abs)
    box.T_w, box.q_w = T_out[:ns].copy(), q_out[:ns].copy()
    box.T_g, box.q_g = T_out[ns:].copy(), q_out[ns:].copy()
    box.energy_error = float(np.sum(j - r - Abs))
    return T_out, j, Abs, r


def equilibrium_surfaces_grey_3d(domain, F, spectral_bin: int = 1, device: int = 0, verbose: bool = False,
                                 info: Optional[dict] = None):
    """equilibriumSurfacesGrey3D! (equilibriumSurfacesGrey3D.jl:40-132) with
    populateWorkspace!(::SurfaceOnlyWorkspace, ::ViewFactorDomain3D)
    (WorkspaceStructs.jl:120-141) and writeResultsToDomainGrey3D!
    (writeResultsToDomain3D.jl:54-83).  The system (I - diag(coeff) F') j = h
    runs on the device (rthx_solve_grey; the reference's dense `\\` is met
    within the solver tolerance).  Returns (T, j, Abs, r)."""
    subs = domain.subfaces()
    n = len(subs)
    b = spectral_bin - 1
    area = np.array([s.area for s in subs])
    eps = np.array([float(np.atleast_1d(s.epsilon)[min(b, np.size(s.epsilon) - 1)]) for s in subs])
    Tw = np.array([s.T_in_w for s in subs])
    qw = np.array([s.q_in_w for s in subs])
    Q_known = (Tw < 0.0).astype(int)
    E = np.where(Q_known == 0, eps * STEFAN_BOLTZMANN * area * Tw ** 4, 0.0)  # computeEmissivePowers! (:3-16)
    h = np.where(Q_known == 1, qw, E)
    coeff = np.where(Q_known == 1, 1.0, 1.0 - eps)
    solve_info = {} if info is None else info
    j, g = _solve(np.asarray(F)[:n, :n], coeff, h, device, solve_info)
    if verbose:
        print(f"GMRES: {solve_info['iterations']} iterations, residual {solve_info['residual']:.3e}")
    Bv = 1.0 - eps  # getValueB(::SurfaceOnlyWorkspace) (WorkspaceStructs.jl:173-175)
    Abs = (1.0 - Bv) * g
    r = Bv * g
    T = np.zeros(n)
    for i in range(n):  # computeTemperatures! (:18-34)
        e = max(j[i] - r[i], 0.0)
        T[i] = (e / (eps[i] * STEFAN_BOLTZMANN * area[i])) ** 0.25 if eps[i] > 0.0 and area[i] > 0.0 else 0.0
    T = np.nan_to_num(T, nan=0.0)
    for i, s in enumerate(subs):  # writeResultsToDomainGrey3D!
        e = max(j[i] - r[i], 0.0)
        s.j_w, s.g_a_w, s.e_w, s.r_w = j[i], Abs[i], e, r[i]
        s.g_w = Abs[i] + r[i]
        s.i_w = j[i] / (math.pi * s.area)
        if s.T_in_w < -0.1:
            s.q_w = s.q_in_w
            s.T_w = T[i]
        else:
            s.T_w = s.T_in_w
            s.q_w = e - Abs[i]
    domain.energy_error = float(np.sum(j - r - Abs))
    return T, j, Abs, r


# --------------------------------------------------------------------------
# spectral GERT solve
# --------------------------------------------------------------------------
def _check_band_limits(limits, n_bins: int) -> np.ndarray:
    """The checks of equilibriumSpectral2D! (equilibriumSpectral2D.jl:58-79)."""
    if limits is None:
        raise ValueError("Spectral solve requires wavelength band limits to be set (dom.wavelength_band_limits)")
    lim = np.ascontiguousarray(limits, dtype=np.float64)
    if lim.ndim != 1 or len(lim) < 4:
        raise ValueError("wavelength_band_limits must have at least 4 values (defining 3 bins)")
    if np.any(lim <= 0):
        raise ValueError("wavelength_band_limits must all be positive (wavelengths > 0)")
    if np.any(np.diff(lim) <= 0):
        raise ValueError("wavelength_band_limits must be strictly increasing (no duplicates)")
    if len(lim) != n_bins + 1:
        raise ValueError(f"{len(lim)} wavelength_band_limits for {n_bins} spectral bins (n_bins + 1 expected)")
    return lim


def _band_struct(F, n: int, handle, keep: list) -> abi.SpectralBand:
    """One rthx_spectral_band from a SmoothHandle (dense or sparse), a scipy
    sparse matrix or a dense array (its leading n x n block); `keep` holds
    the arrays alive."""
    band = abi.SpectralBand()
    if handle is not None:
        band.smoothed = handle.handle
        keep.append(handle)
    elif sp.issparse(F):
        Fc = F.tocsr()[:n, :n]
        rp = np.ascontiguousarray(Fc.indptr, dtype=np.int64)
        ci = np.ascontiguousarray(Fc.indices, dtype=np.int32)
        vv = np.ascontiguousarray(Fc.data, dtype=np.float64)
        keep += [rp, ci, vv]
        band.row_ptr, band.cols, band.vals = abi.ptr(rp, C.c_int64), abi.ptr(ci, C.c_int32), abi.ptr(vv, C.c_double)
    else:
        Fd = np.ascontiguousarray(np.asarray(F)[:n, :n], dtype=np.float64)
        keep.append(Fd)
        band.dense = abi.ptr(Fd, C.c_double)
    return band


def solve_spectral(F, limits, b, prop, size, T_in, q_in, device: int = 0, max_iters: int = 1000,
                   convergence_tol: float = 1e-12, handles=None, rtol: float = 1e-12,
                   atol: float = math.sqrt(np.finfo(np.float64).eps), memory: int = 50):
    """rthx_solve_spectral.  F: one matrix (shared by every band) or a list of
    K, each dense, scipy sparse, or None with a SmoothHandle in `handles` at
    that place; b, prop: [K, n]; size, T_in, q_in: [n].  Returns
    (j[K, n], g[K, n], T[n], e[n], info)."""
    lib = load()
    b = np.ascontiguousarray(b, dtype=np.float64)
    prop = np.ascontiguousarray(prop, dtype=np.float64)
    K, n = b.shape
    mats = list(F) if isinstance(F, (list, tuple)) else [F]
    hs = list(handles) if handles is not None else [None] * len(mats)
    if len(mats) > 1 and all(m is mats[0] for m in mats) and all(h is hs[0] for h in hs):
        mats, hs = mats[:1], hs[:1]  # grouped bins share one matrix: one pass over it
    keep: list = []
    bands = (abi.SpectralBand * len(mats))(*[_band_struct(m, n, h, keep) for m, h in zip(mats, hs)])
    lim = np.ascontiguousarray(limits, dtype=np.float64)
    size = np.ascontiguousarray(size, dtype=np.float64)
    T_in = np.ascontiguousarray(T_in, dtype=np.float64)
    q_in = np.ascontiguousarray(q_in, dtype=np.float64)
    a = abi.SpectralArgs()
    a.device, a.memory, a.itmax, a.max_outer = device, memory, 0, int(max_iters)
    a.rtol, a.atol, a.convergence_tol = rtol, atol, convergence_tol
    j = np.empty((K, n))
    g = np.empty((K, n))
    T = np.empty(n)
    e = np.empty(n)
    inf = abi.SpectralInfo()
    dp = C.c_double
    check(lib.rthx_solve_spectral(bands, len(mats), n, K, abi.ptr(lim, dp), abi.ptr(b, dp), abi.ptr(prop, dp),
                                  abi.ptr(size, dp), abi.ptr(T_in, dp), abi.ptr(q_in, dp), C.byref(a),
                                  abi.ptr(j, dp), abi.ptr(g, dp), abi.ptr(T, dp), abi.ptr(e, dp), C.byref(inf)))
    del keep
    return j, g, T, e, inf.as_dict()


def _report(si: dict, info: Optional[dict], verbose: bool) -> None:
    if info is not None:
        info.update(si)
    if verbose:
        print(f"spectral solve: {si['outer_iterations']} outer iterations, {si['gmres_iterations']} GMRES steps, "
              f"change {si['change']:.3e}, residual {si['residual']:.3e} (tolerance {si['tolerance']:.3e})")
    if not si["converged"]:
        import warnings

        warnings.warn(f"spectral solve not converged after {si['outer_iterations']} outer iterations "
                      f"(change {si['change']:.3e})")


def equilibrium_spectral(dom, F=None, device: int = 0, max_iters: int = 1000, convergence_tol: float = 1e-12,
                         verbose: bool = False, info: Optional[dict] = None):
    """equilibriumSpectral2D! (equilibriumSpectral2D.jl) for both spectral
    modes, solved on the device (rthx_solve_spectral).  F: one
    matrix or a list of one per band (default dom.F_smooth, read in place on
    the device when it lives there).  Writes per band j, g_a, e, r, g (and i)
    into the per-bin vectors of every face (writeResultsToDomainSpectralBin!),
    T and q (writeTemperaturesHeatSources!) and dom.energy_error (one value
    per band); returns (T, j[K, n], Abs[K, n], r[K, n])."""
    from .direct import _ensure_result_fields

    K = dom.n_spectral_bins
    lim = _check_band_limits(dom.wavelength_band_limits, K)
    wss = [populate_workspace(dom, k) for k in range(1, K + 1)]
    ns, nv = len(wss[0]["Area"]), len(wss[0]["Volume"])
    n = ns + nv
    b = np.array([np.concatenate([1.0 - ws["epsw"], ws["omega_g"]]) for ws in wss])
    prop = np.array([np.concatenate([ws["epsw"], ws["kappa_g"]]) for ws in wss])
    size = np.concatenate([wss[0]["Area"], 4.0 * wss[0]["Volume"]])
    T_in = np.concatenate([wss[0]["Tw"], wss[0]["Tg"]])
    q_in = np.concatenate([wss[0]["qw"], wss[0]["qg"]])
    handles = None
    if F is None:
        if dom.F_smooth_handle() is not None:
            handles = [dom.F_smooth_handle()]
        else:
            F = dom.F_smooth
    else:
        dev = getattr(dom, "_F_smooth_device", None)
        if dev is not None and dev[0] is F:
            handles = [dev[1]]
    if handles is not None:
        F = [None]
    j, g, T, e, si = solve_spectral(F, lim, b, prop, size, T_in, q_in, device=device, max_iters=max_iters,
                                    convergence_tol=convergence_tol, handles=handles)
    _report(si, info, verbose)
    r = b * g
    Abs = (1.0 - b) * g
    em = np.maximum(j - r, 0.0)
    _ensure_result_fields(dom)
    for (c, f, w), s in dom.surface_mapping.items():  # writeResultsToDomainSpectralBin!
        face = dom.fine_mesh[c - 1][f - 1]
        i, k = s - 1, w - 1
        if not isinstance(getattr(face, "i_w", None), list) or len(face.i_w) != len(face.solidWalls):
            face.i_w = [0.0] * len(face.solidWalls)
        face.j_w[k] = j[:, i].copy()
        face.g_a_w[k] = Abs[:, i].copy()
        face.e_w[k] = em[:, i].copy()
        face.r_w[k] = r[:, i].copy()
        face.g_w[k] = Abs[:, i] + r[:, i]
        face.i_w[k] = j[:, i] / (math.pi * face.area[k])
        if face.T_in_w[k] > -0.1:  # writeTemperaturesHeatSources!
            face.T_w[k] = face.T_in_w[k]
            face.q_w[k] = float(np.sum(em[:, i]) - np.sum(Abs[:, i]))
        else:
            face.T_w[k] = T[i]
            face.q_w[k] = face.q_in_w[k]
    if nv:
        for (c, f), v in dom.volume_mapping.items():
            face = dom.fine_mesh[c - 1][f - 1]
            i = ns + v - 1
            face.j_g = j[:, i].copy()
            face.g_a_g = Abs[:, i].copy()
            face.e_g = em[:, i].copy()
            face.r_g = r[:, i].copy()
            face.g_g = Abs[:, i] + r[:, i]
            face.i_g = j[:, i] / (4 * math.pi * face.volume)
            if face.T_in_g > -0.1:
                face.T_g = face.T_in_g
                face.q_g = float(np.sum(em[:, i]) - np.sum(Abs[:, i]))
            else:
                face.T_g = T[i]
                face.q_g = face.q_in_g
    dom.energy_error = [float(np.sum(j[k] - g[k])) for k in range(K)]  # sum((I - F_k') j_k)
    return T, j, Abs, r


def equilibrium_surfaces_spectral_3d(domain, F, device: int = 0, max_iters: int = 1000,
                                     convergence_tol: float = 1e-12, verbose: bool = False,
                                     info: Optional[dict] = None):
    """equilibriumSurfacesSpectral3D! (equilibriumSurfacesSpectral3D.jl): the
    spectral solve with one shared F, then writeResultsToDomainSpectralBin3D!
    and writeTemperaturesHeatSources!.  Returns (T, j[K, n], Abs[K, n], r[K, n])."""
    K = domain.n_spectral_bins
    lim = _check_band_limits(domain.wavelength_band_limits, K)
    subs = domain.subfaces()
    n = len(subs)
    eps = np.array([np.broadcast_to(np.asarray(s.epsilon, dtype=np.float64), (K,)) for s in subs]).T.copy()
    area = np.array([s.area for s in subs])
    T_in = np.array([s.T_in_w for s in subs])
    q_in = np.array([s.q_in_w for s in subs])
    Fm = F if sp.issparse(F) else np.asarray(F)[:n, :n]
    j, g, T, e, si = solve_spectral(Fm, lim, 1.0 - eps, eps, area, T_in, q_in, device=device, max_iters=max_iters,
                                    convergence_tol=convergence_tol)
    _report(si, info, verbose)
    b = 1.0 - eps
    r = b * g
    Abs = (1.0 - b) * g
    em = np.maximum(j - r, 0.0)
    for i, s in enumerate(subs):
        s.j_w, s.g_a_w, s.e_w, s.r_w = j[:, i].copy(), Abs[:, i].copy(), em[:, i].copy(), r[:, i].copy()
        s.g_w = Abs[:, i] + r[:, i]
        s.i_w = j[:, i] / (math.pi * s.area)
        if s.T_in_w > -0.1:
            s.T_w = s.T_in_w
            s.q_w = float(np.sum(em[:, i]) - np.sum(Abs[:, i]))
        else:
            s.T_w = T[i]
            s.q_w = s.q_in_w
    domain.energy_error = [float(np.sum(j[k] - g[k])) for k in range(K)]
    return T, j, Abs, r
