"""tests/solver_ref.py pinned on the CPU: the generators give what their
docstrings say, the extended-precision fixed-pass smoothing agrees with the
numpy restatement (oracle/smooth_oracle.py) to rounding, the restatement
converges on every case tests/test_gpu_smooth_edges.py runs to convergence,
and the GMRES restatement restarts, stalls and stops where
tests/test_gpu_solve_edges.py expects the device to.  CPU only.

Bound of the fixed-pass agreement (fixed_pass_bound): an entry of F_smooth
passes through 3 + 2 k rounded operations (w F, the halved sum, k products
with the rounded (u_i + u_j) / 2, the final division), and k + 1 row sums
enter it, each through one division.  Every summand is positive, so a row
sum's relative error is at most its longest addition chain: numpy adds blocks
of at most 128 entries on 8 accumulators (16 additions, 3 to combine) and
pairs the blocks (ceil(log2(n / 128)) more).  To first order the distance is
below (3 + 2 k + (k + 1) (2 + chain)) u, u = eps / 2; the measured distances
are printed and are 10 times smaller.
"""
import math

import numpy as np
import pytest
import scipy.sparse as sp

import solver_ref as R
from oracle import smooth_oracle as so

EPS = R.EPS
DENSE_N = [1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513, 575, 577, 1023, 1024, 1025, 1087, 1088, 1089]
SPARSE = {9: [1, 2], 515: [1, 2, 63, 64, 65, 127, 128, 129]}


def fixed_pass_bound(n, k):
    chain = 19 + max(0, math.ceil(math.log2(max(n, 1) / 128.0)))
    return (3 + 2 * k + (k + 1) * (2 + chain)) / 2.0  # in eps


def props(Fs, w):
    """check_props of tests/test_gpu_smooth.py."""
    Fd = R.dense(Fs)
    W = np.asarray(w) / np.min(w)
    assert np.abs(Fd.sum(axis=1) - 1).max() < 1e-12
    X = W[:, None] * Fd
    assert np.abs(X - X.T).max() <= 8 * EPS * np.abs(X).max() * 4
    assert Fd.min() >= 0.0


# ---------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------
def test_synth_dense():
    F, w = R.synth_dense(65, 3)
    assert F.shape == (65, 65) and np.count_nonzero(F) == 65 * 65
    assert np.abs(F.sum(axis=1) - 1).max() <= 4 * EPS
    assert w.min() >= 1.0 and w.max() <= 50.0 and len(np.unique(w)) == 65
    F2, w2 = R.synth_dense(65, 3)
    assert np.array_equal(F, F2) and np.array_equal(w, w2)


@pytest.mark.parametrize("n", sorted(SPARSE))
def test_synth_sparse(n):
    lens = SPARSE[n]
    F, w = R.synth_sparse(n, n, lens)
    assert sp.isspmatrix_csr(F) and F.has_sorted_indices
    assert np.array_equal(np.diff(F.indptr), [lens[i % len(lens)] for i in range(n)])
    assert np.all(F.diagonal() > 0)
    assert np.abs(np.asarray(F.sum(axis=1)).ravel() - 1).max() <= 4 * EPS
    for i in range(n):
        assert len(set(F.indices[F.indptr[i]:F.indptr[i + 1]])) == F.indptr[i + 1] - F.indptr[i]
    density = F.nnz / n ** 2
    print(f"n {n}: density {density:.3f}")
    assert density < 0.25  # the sparse route
    # reversed rows hold the same matrix
    rp, ci, v = R.reverse_rows(F)
    G = sp.csr_matrix((v, ci, rp), shape=(n, n))
    assert not G.has_sorted_indices or max(lens) == 1
    assert np.array_equal(G.toarray(), F.toarray())


def test_chain_F():
    assert np.array_equal(R.chain_F(1), [[1.0]])
    assert np.array_equal(R.chain_F(3), [[0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])
    F = R.chain_F(129)
    assert np.array_equal(F, F.T) and np.all(F.sum(axis=1) == 1.0) and np.count_nonzero(F) == 2 * 129
    ev = np.linalg.eigvalsh(F)
    assert np.allclose(ev, np.sort(np.cos(np.arange(129) * np.pi / 129)), atol=1e-12)


# ---------------------------------------------------------------------------
# fixed passes: extended precision against the float64 restatement
# ---------------------------------------------------------------------------
def fixed_case(n, lens=None):
    F, w = R.synth_sparse(n, n, lens) if lens else R.synth_dense(n, n)
    log = []
    Fo = so.smooth_F(F, w, 0, max_iters=3, k_dykstra=0, log=log)
    done = [x for x in log if x[0] == "ap_done"][0]
    k = done[1]
    assert k == (3 if n > 1 else 0)  # no convergence branch is taken: three scale passes (none at n = 1)
    assert log[0][1] == ("sparse" if lens else "dense") and sp.issparse(Fo) == bool(lens)
    W = w / w.min()  # smooth_F's renorm, in float64 as there
    # the restatement's own defects lie within the bound the device is held to
    X = so.build_X(F, W)
    seen = [(0, so.delta_R_X(X, W, so.hunger(X, W)[1]))] + [(x[1], x[2]) for x in log if x[0] == "ap"]
    assert len(seen) == (2 if n > 1 else 1)  # with max_iters = 3 the schedule evaluates the defect once more, after pass 1
    for p, d in seen:
        d_ld, s_norm = R.defect_ld(F, W, p)
        assert abs(d - d_ld) <= R.defect_bound(n, p, d_ld, s_norm)
        assert d_ld == 0 or R.defect_bound(n, p, d_ld, s_norm) < 1e-3 * d_ld / n  # far below one missing row
    return F, W, Fo, R.smooth_fixed_ld(F, W, k)


@pytest.mark.parametrize("n", DENSE_N)
def test_fixed_passes_dense(n):
    F, W, Fo, Fl = fixed_case(n)
    d = R.rel_distance(Fo, Fl)
    print(f"dense n {n}: restatement within {d:.2f} eps of extended precision (bound {fixed_pass_bound(n, 3):.0f})")
    assert d <= fixed_pass_bound(n, 3)
    assert float(np.abs(Fl.sum(axis=1) - 1).max()) <= np.finfo(R.LD).eps * 8


@pytest.mark.parametrize("n", sorted(SPARSE))
def test_fixed_passes_sparse(n):
    F, W, Fo, Fl = fixed_case(n, SPARSE[n])
    patt = ((F + F.T) != 0).toarray()
    assert np.array_equal(Fo.toarray() != 0, patt) and np.array_equal(Fl != 0, patt)
    d = R.rel_distance(Fo, Fl)
    print(f"sparse n {n}: restatement within {d:.2f} eps of extended precision (bound {fixed_pass_bound(n, 3):.0f})")
    assert d <= fixed_pass_bound(n, 3)


def test_fixed_ld_notices_one_entry():
    """A row sum that misses one entry moves F by about 1 / n relative in that
    row, far above the rounding bound."""
    n = 257
    F, w = R.synth_dense(n, n)
    Fl = R.smooth_fixed_ld(F, w, 3)
    G = F.copy()
    G[100, 200] = 0.0
    assert R.rel_distance(R.smooth_fixed_ld(G, w, 3).astype(np.float64), Fl) > 1e4 * fixed_pass_bound(n, 3)


# ---------------------------------------------------------------------------
# the restatement converges where the device is run to convergence
# ---------------------------------------------------------------------------
def run_oracle(F, w, **kw):
    log = []
    Fo = so.smooth_F(F, w, 0, log=log, **kw)
    done = [x for x in log if x[0] == "ap_done"][0]
    dyk = [x for x in log if x[0] == "dykstra"]
    return Fo, done, dyk


@pytest.mark.parametrize("n", [65, 513, 1089])
def test_full_ap_dense_converges(n):
    F, w = R.synth_dense(n, n)
    Fo, done, _ = run_oracle(F, w)
    print(f"dense n {n}: AP converged {done[3]} in {done[1]} iterations, delta {done[2]:.3g}")
    assert done[3] and not done[4] and done[1] < 1000
    props(Fo, w)


@pytest.mark.parametrize("n", sorted(SPARSE))
def test_full_ap_sparse_converges(n):
    F, w = R.synth_sparse(n, n, SPARSE[n])
    Fo, done, _ = run_oracle(F, w)
    print(f"sparse n {n}: AP converged {done[3]} in {done[1]} iterations, delta {done[2]:.3g}")
    assert sp.issparse(Fo) and done[3] and not done[4] and done[1] < 1000
    props(Fo, w)


@pytest.mark.parametrize("n,k", [(2, 1), (33, 1), (257, 1), (1025, 1), (33, 6)])
def test_dykstra_then_ap_converges(n, k):
    F, w = R.synth_dense(n, n)
    Fo, done, dyk = run_oracle(F, w, k_dykstra=k)
    print(f"n {n}, k_dykstra {k}: PCG {[x[2] for x in dyk]}, AP converged {done[3]} in {done[1]} iterations")
    assert dyk and all(x[2] < 200 for x in dyk)  # the PCG cap is not reached
    assert done[3] and done[1] < 1000
    props(Fo, w)


# ---------------------------------------------------------------------------
# GMRES restatement: the control flow the device tests rely on
# ---------------------------------------------------------------------------
def tol_of(h, rtol, atol):
    return atol + rtol * np.linalg.norm(h)


# steps and cycles of the restatement at n = 129 / 257
RESTART_FACTS = {"short_memory": {129: (55, 11), 257: (56, 12)},
                 "reference_memory": {129: (190, 4), 257: (194, 4)},
                 "memory_1": {129: (186, 186), 257: (192, 192)}}


@pytest.mark.parametrize("n", [129, 257])
@pytest.mark.parametrize("name,c,memory,tols", R.GMRES_RESTARTING, ids=[x[0] for x in R.GMRES_RESTARTING])
def test_gmres_restarts(name, c, memory, tols, n):
    F, co, h, M = R.chain_system(n, c)
    x, it, cyc = R.gmres_restarted(M, h, memory=memory, **tols)
    print(f"n {n}, c {c}, memory {memory}: {it} steps in {cyc} cycles")
    assert np.linalg.norm(h - M @ x) <= tol_of(h, **tols)
    assert cyc >= 2 and it <= 2 * n and it > memory * (cyc - 1)
    # the recorded facts, to within one cycle (the last bits of a BLAS product may move a step)
    it0, cyc0 = RESTART_FACTS[name][n]
    assert abs(it - it0) <= memory and abs(cyc - cyc0) <= 1
    if memory == 1:
        assert it == cyc


@pytest.mark.parametrize("n", sorted(R.GMRES_STALLING))
def test_gmres_exhausts_itmax(n):
    tols = R.GMRES_STALLING[n]
    F, co, h, M = R.chain_system(n, 0.99)
    x, it, cyc = R.gmres_restarted(M, h, memory=5, **tols)
    ratio = np.linalg.norm(h - M @ x) / tol_of(h, **tols)
    print(f"n {n}, c 0.99, memory 5, atol {tols['atol']:.3g}: residual {ratio:.3g} of the tolerance after {it} steps")
    assert it == 2 * n and ratio > 4.0  # far enough that another rounding cannot decide it
    x, it, cyc = R.gmres_restarted(M, h, memory=5, itmax=3, **tols)
    assert it == 3 and cyc == 1


def test_gmres_stall_meets_default_tolerance_at_257():
    """Why GMRES_STALLING runs n = 257 with atol = 0: with the default atol the
    stalling system is solved in 410 of 514 steps, by a hair."""
    F, co, h, M = R.chain_system(257, 0.99)
    x, it, cyc = R.gmres_restarted(M, h, memory=5, **R.DEFAULT_TOL)
    ratio = np.linalg.norm(h - M @ x) / tol_of(h, **R.DEFAULT_TOL)
    print(f"n 257, c 0.99, memory 5, default tolerances: {it} steps in {cyc} cycles, residual {ratio:.3g} of the tolerance")
    assert 5 * 50 < it < 2 * 257 and it > 5 * (cyc - 1) and 0.5 < ratio <= 1.0


def test_gmres_trivial_cases():
    F, co, h, M = R.chain_system(3, 0.9)
    x, it, cyc = R.gmres_restarted(M, h, memory=50)
    assert it <= 3 and np.linalg.norm(h - M @ x) <= tol_of(h, **R.DEFAULT_TOL)
    x, it, cyc = R.gmres_restarted(M, np.zeros(3), memory=50)
    assert it == 0 and cyc == 0 and not x.any()
    # M = I: one step, left by the breakdown or the estimate, and x = h
    h = np.random.default_rng(5).standard_normal(129)
    x, it, cyc = R.gmres_restarted(np.eye(129), h, memory=50)
    assert it == 1 and cyc == 1 and np.abs(x - h).max() <= 16 * EPS * np.abs(h).max()
    # against a direct solve
    F, co, h, M = R.chain_system(129, 0.9)
    x, it, cyc = R.gmres_restarted(M, h, memory=50, atol=0.0)
    assert np.linalg.norm(x - np.linalg.solve(M, h)) <= np.linalg.cond(M) * 1e-12 * np.linalg.norm(h)
