"""Grey GERT solve (rthx_solve_grey, rthx_solve_grey_smoothed) through
abi.SolveArgs on synthetic systems (tests/solver_ref.py): the operator F' x at
the chunk and wave-stride edges of its kernels, and the control flow of the
GMRES driver (csrc/rthx_solve.cpp) that the traced N = 165 cases never reach:
restarts, memory other than 50, an exhausted itmax, a breakdown step, h = 0
and n below memory.

Every bound follows from the code (solver_ref.ftx_chain, dot_chain) or from
the system itself; none is fitted:
  g_out      |g_i - (F' j_out)_i| <= m_i eps sum_k |F_ki j_k|, the exact product
             taken in extended precision and m_i the longest addition chain of
             the kernel plus one: 128 + ceil(n / 128) + 1 (k_ftx_part +
             k_ftx_reduce), ceil(len_i / 64) + 6 + 1 (k_spmv).
  residual   info.residual against |h - M j_out| in extended precision: they
             differ by the rounding of the device's M j_out (the product's
             bound times |c_i|, one rounding each for c y, j - c y and h - w)
             and of the norm (k_multidot's chain).
  j_out      |j - j*|_2 <= |M^-1|_2 info.residual + cond_2(M) n eps |j*|_2 with
             j* from numpy.linalg.solve and the norms from an SVD.
Step counts are not compared with the restatement: the device orthogonalises
by classical Gram-Schmidt twice, the restatement by modified Gram-Schmidt.
"""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.sparse as sp

import solver_ref as R

pytestmark = pytest.mark.gpu

DP = C.c_double
EPS = R.EPS
LD = R.LD


def solve(lib, co, h, dense=None, csr=None, handle=None, memory=50, itmax=0, rtol=1e-12, atol=math.sqrt(EPS)):
    """One rthx_solve_grey* call; (j, g, info).  The outputs start as NaN."""
    from rthx import abi

    n = len(h)
    a = abi.SolveArgs()
    a.device, a.memory, a.itmax, a.rtol, a.atol = 0, memory, itmax, rtol, atol
    co = np.ascontiguousarray(co, dtype=np.float64)
    h = np.ascontiguousarray(h, dtype=np.float64)
    j, g = np.full(n, np.nan), np.full(n, np.nan)
    info = abi.SolveInfo()
    tail = (abi.ptr(co, DP), abi.ptr(h, DP), C.byref(a), abi.ptr(j, DP), abi.ptr(g, DP), C.byref(info))
    if handle is not None:
        rc = lib.rthx_solve_grey_smoothed(handle.handle, *tail)
    elif csr is not None:
        rp = np.ascontiguousarray(csr.indptr, dtype=np.int64)
        ci = np.ascontiguousarray(csr.indices, dtype=np.int32)
        v = np.ascontiguousarray(csr.data, dtype=np.float64)
        rc = lib.rthx_solve_grey(abi.ptr(rp, C.c_int64), abi.ptr(ci, C.c_int32), abi.ptr(v, DP), None, n, *tail)
    else:
        Fd = np.ascontiguousarray(dense, dtype=np.float64)
        rc = lib.rthx_solve_grey(None, None, None, abi.ptr(Fd, DP), n, *tail)
    assert rc == abi.RTHX_OK, lib.rthx_last_error()
    assert info.n == n and np.all(np.isfinite(j)) and np.all(np.isfinite(g))
    return j, g, info


def check_g(F, form, j, g, what):
    exact, mag = R.ftx_exact(F, j)
    bound = R.ftx_chain(F, form) * EPS * mag
    err = np.abs(g.astype(LD) - exact)
    worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0.0)))
    print(f"{what}: g within {worst:.3f} of its bound")
    assert np.all(err <= bound)
    assert not g[np.asarray(mag == 0)].any()  # an empty column of F gives exactly 0


def check_residual(F, form, co, h, j, info, what, rtol=1e-12, atol=math.sqrt(EPS)):
    n = len(h)
    y, mag = R.ftx_exact(F, j)
    col, jl, hl = co.astype(LD), j.astype(LD), h.astype(LD)
    r = hl - (jl - col * y)
    delta = EPS * (np.abs(col) * R.ftx_chain(F, form) * mag + np.abs(col * y) + np.abs(jl - col * y) + np.abs(r))
    rn = float(np.sqrt(np.sum(r * r)))
    allowed = float(np.sqrt(np.sum(delta * delta))) + R.dot_chain(n) * EPS * rn
    print(f"{what}: residual {info.residual:.6e}, recomputed {rn:.6e}, difference {abs(info.residual - rn):.2e} "
          f"of {allowed:.2e} allowed; tolerance {info.tolerance:.3e}")
    assert abs(info.residual - rn) <= allowed
    hn = float(np.sqrt(np.sum(hl * hl)))
    assert abs(info.tolerance - (atol + rtol * hn)) <= rtol * R.dot_chain(n) * EPS * hn


def check_solution(M, h, j, info, what):
    n = len(h)
    js = np.linalg.solve(M, h)
    s = np.linalg.svd(M, compute_uv=False)
    bound = info.residual / s[-1] + (s[0] / s[-1]) * n * EPS * np.linalg.norm(js)
    err = np.linalg.norm(j - js)
    print(f"{what}: |j - j*| {err:.3e} of {bound:.3e}")
    assert err <= bound


def check_all(F, form, co, h, j, g, info, what, **tols):
    check_g(F, form, j, g, what)
    check_residual(F, form, co, h, j, info, what, **tols)
    check_solution(np.eye(len(h)) - co[:, None] * R.dense(F).T, h, j, info, what)
    assert (info.converged == 1) == (info.residual <= info.tolerance)


# ---------------------------------------------------------------------------
# the operator alone: coeff = 0, the system is j = h
# ---------------------------------------------------------------------------
def operator_alone(lib, F, form, what, **route):
    n = F.shape[0]
    h = np.random.default_rng(1000 + n).standard_normal(n)
    j, g, info = solve(lib, np.zeros(n), h, **route)
    print(f"{what}: {info.iterations} step, {info.cycles} cycle, residual {info.residual:.3e}, "
          f"max |j - h| / |h| {np.max(np.abs(j - h) / np.abs(h)) / EPS:.2f} eps")
    assert info.converged == 1 and info.iterations == 1
    # j = v (beta / (v . v)) with v = h / beta: two dot products of k_multidot's chain and 5 roundings
    assert np.all(np.abs(j - h) <= (-(-n // 256) + 16) * EPS * np.abs(h))
    check_all(F, form, np.zeros(n), h, j, g, info, what)


@pytest.mark.parametrize("n", [1, 127, 128, 129, 255, 256, 257, 513])
def test_operator_host_dense(hip, n):
    F = np.random.default_rng(n).standard_normal((n, n))
    operator_alone(hip.load(), F, "dense", f"host dense n {n}", dense=F)


@pytest.mark.parametrize("n", [5, 259])
def test_operator_host_csr(hip, n):
    F = R.synth_columns(n, n, [0, 1, 63, 64, 65, 129])
    pops = np.diff(F.tocsc().indptr)
    assert set(pops) == {min(p, n - 1) for p in (0, 1, 63, 64, 65, 129)}  # the row lengths of F'
    assert F.indptr[n] == F.indptr[n - 1]  # an empty row beside the empty columns
    operator_alone(hip.load(), F, "sparse", f"host CSR n {n}", csr=F)


def test_operator_dense_smoothing_handle(hip):
    from rthx.smoothing import smooth_F

    n = 257
    F, w = R.synth_dense(n, n)
    Fs, handle = smooth_F(F, w, 0, max_iters=3, verbose=False, keep_device=True)
    try:
        assert handle.dense and Fs.shape == (n, n)
        operator_alone(hip.load(), Fs, "dense", f"dense smoothing handle n {n}", handle=handle)
    finally:
        handle.close()


def test_operator_sparse_smoothing_handle(hip):
    from rthx.smoothing import smooth_F

    n = 515
    F, w = R.synth_sparse(n, n, [1, 2, 63, 64, 65, 127, 128, 129])
    Fs, handle = smooth_F(F, w, 0, max_iters=3, verbose=False, keep_device=True)
    try:
        assert not handle.dense and sp.issparse(Fs)
        lens = np.diff(Fs.tocsc().indptr)
        print(f"rows of F': {lens.min()} to {lens.max()} entries")
        assert lens.min() <= 64 < 128 < lens.max()  # one, two and more wave strides
        operator_alone(hip.load(), Fs, "sparse", f"sparse smoothing handle n {n}", handle=handle)
    finally:
        handle.close()


# ---------------------------------------------------------------------------
# GMRES control flow on the random-walk chain: M = I - c F'
# ---------------------------------------------------------------------------
ROUTES = [("dense", 129), ("csr", 257)]  # 129 crosses a 128-row chunk


def chain(form, n, c):
    F, co, h, M = R.chain_system(n, c)
    if form == "csr":
        Fs = sp.csr_matrix(F)
        return Fs, "sparse", co, h, dict(csr=Fs)
    return F, "dense", co, h, dict(dense=F)


@pytest.mark.parametrize("form,n", ROUTES)
@pytest.mark.parametrize("name,c,memory,tols", R.GMRES_RESTARTING, ids=[x[0] for x in R.GMRES_RESTARTING])
def test_gmres_restarts(hip, name, c, memory, tols, form, n):
    F, kind, co, h, route = chain(form, n, c)
    j, g, info = solve(hip.load(), co, h, memory=memory, **tols, **route)
    what = f"{name} {form} n {n}"
    print(f"{what}: {info.iterations} steps in {info.cycles} cycles")
    assert info.converged == 1 and info.cycles >= 2 and info.iterations <= 2 * n
    assert info.iterations <= memory * info.cycles
    if memory == 1:
        assert info.iterations == info.cycles
    check_all(F, kind, co, h, j, g, info, what, **tols)


@pytest.mark.parametrize("form,n", ROUTES)
def test_gmres_exhausts_itmax(hip, form, n):
    """c = 0.99 with memory 5 stalls (solver_ref.GMRES_STALLING): the default
    itmax = 2 n runs out with the residual above the tolerance."""
    F, kind, co, h, route = chain(form, n, 0.99)
    tols = R.GMRES_STALLING[n]
    j, g, info = solve(hip.load(), co, h, memory=5, **tols, **route)
    what = f"stalling {form} n {n}"
    print(f"{what}: {info.iterations} steps in {info.cycles} cycles, residual {info.residual / info.tolerance:.3g} "
          f"of the tolerance")
    assert info.converged == 0 and info.iterations == 2 * n and info.residual > info.tolerance
    assert info.cycles == -(-2 * n // 5)
    check_all(F, kind, co, h, j, g, info, what, **tols)
    j, g, info = solve(hip.load(), co, h, memory=5, itmax=3, **tols, **route)
    assert info.iterations == 3 and info.cycles == 1 and info.converged == 0
    check_all(F, kind, co, h, j, g, info, what + " itmax 3", **tols)


def test_gmres_stall_meets_the_default_tolerance_at_257(hip):
    """The stalling system at n = 257 with the default atol (solver_ref.
    GMRES_STALLING): solved within 2 n steps after many five-step cycles."""
    F, kind, co, h, route = chain("csr", 257, 0.99)
    j, g, info = solve(hip.load(), co, h, memory=5, **route)
    print(f"{info.iterations} steps in {info.cycles} cycles")
    assert info.converged == 1 and info.cycles >= 2 and info.iterations <= 2 * 257
    check_all(F, kind, co, h, j, g, info, "stalling csr n 257, default tolerances")


@pytest.mark.parametrize("form,n", ROUTES)
def test_zero_right_hand_side(hip, form, n):
    F, kind, co, h, route = chain(form, n, 0.9)
    j, g, info = solve(hip.load(), co, np.zeros(n), **route)
    assert not j.any() and not g.any()
    assert info.iterations == 0 and info.cycles == 0 and info.converged == 1 and info.residual == 0.0


def test_n_below_memory(hip):
    F, kind, co, h, route = chain("dense", 3, 0.9)
    j, g, info = solve(hip.load(), co, h, memory=50, **route)
    print(f"n 3, memory 50: {info.iterations} steps in {info.cycles} cycles")
    assert info.converged == 1 and 1 <= info.iterations <= 3
    check_all(F, kind, co, h, j, g, info, "n 3 memory 50")
