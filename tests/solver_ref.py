"""Synthetic inputs and high-precision references for the device smoothing
(rthx_smooth_F) and the grey GERT solve (rthx_solve_grey*), for
tests/test_gpu_smooth_edges.py and tests/test_gpu_solve_edges.py.  Test
infrastructure only; pinned on the CPU by tests/test_solver_ref.py.

Both stages take plain matrices through the C ABI, so inputs of any size are
generated here instead of traced: sizes on and beside the kernels' tile
boundaries, weights spread over 50 : 1, sparse rows shorter than, equal to and
longer than one and two wave strides.
"""
import math

import numpy as np
import scipy.sparse as sp

EPS = np.finfo(np.float64).eps
LD = np.longdouble


def weights(n, rng):
    """w = exp(U(0, ln 50)): continuous weights over 50 : 1."""
    return np.exp(rng.uniform(0.0, math.log(50.0), n))


def synth_dense(n, seed):
    """(F, w): F = A / rowsum with A = U(0, 1) + 0.05 (density 1, the dense
    route), w as weights()."""
    rng = np.random.default_rng(seed)
    w = weights(n, rng)
    A = rng.random((n, n)) + 0.05
    return A / A.sum(axis=1, keepdims=True), w


def synth_sparse(n, seed, lens):
    """(F as CSR with ascending columns, w): row i holds lens[i % len(lens)]
    distinct random columns, always including i; values U + 0.05,
    row-normalised."""
    rng = np.random.default_rng(seed)
    w = weights(n, rng)
    indptr, indices, data = [0], [], []
    for i in range(n):
        L = min(lens[i % len(lens)], n)
        others = np.delete(np.arange(n), i)
        cols = np.sort(np.concatenate([[i], rng.choice(others, L - 1, replace=False)]))
        v = rng.random(L) + 0.05
        indices.append(cols)
        data.append(v / v.sum())
        indptr.append(indptr[-1] + L)
    F = sp.csr_matrix((np.concatenate(data), np.concatenate(indices).astype(np.int32), np.array(indptr, dtype=np.int64)),
                      shape=(n, n))
    return F, w


def synth_columns(n, seed, pops):
    """CSR F with signed normal entries whose column j holds
    min(pops[j % len(pops)], n - 1) entries in random rows below n - 1: the
    column populations are the row lengths of F', a column with population 0 is
    empty, and the last row is empty."""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for j in range(n):
        p = min(pops[j % len(pops)], n - 1)
        rows.append(rng.choice(n - 1, p, replace=False))
        cols.append(np.full(p, j))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    F = sp.csr_matrix((rng.standard_normal(len(rows)), (rows, cols)), shape=(n, n))
    F.sort_indices()
    return F


def reverse_rows(F):
    """The CSR arrays of F with the columns of every row in descending order."""
    rp = F.indptr.astype(np.int64)
    ci = F.indices.astype(np.int32).copy()
    v = F.data.astype(np.float64).copy()
    for i in range(F.shape[0]):
        ci[rp[i]:rp[i + 1]] = ci[rp[i]:rp[i + 1]][::-1]
        v[rp[i]:rp[i + 1]] = v[rp[i]:rp[i + 1]][::-1]
    return rp, ci, v


def chain_F(n):
    """The 1-D random walk: F[i, i +- 1] = 1/2, the ends reflecting onto
    themselves.  Symmetric, rows sum to 1, eigenvalues cos(k pi / n) spread
    over (-1, 1]."""
    F = np.zeros((n, n))
    for i in range(n):
        F[i, i - 1 if i > 0 else i] += 0.5
        F[i, i + 1 if i < n - 1 else i] += 0.5
    return F


def dense(F):
    return F.toarray() if sp.issparse(F) else np.asarray(F)


def smooth_fixed_ld(F, w, k):
    """build_X, hunger, k x (scale, hunger), recover_F of
    oracle/smooth_oracle.py in extended precision (64-bit significand): dense
    longdouble F_smooth.  Its own rounding is 2^-11 of float64's, so at the
    float64 level it does not depend on a summation order."""
    assert np.finfo(LD).eps <= 2.0 ** -63, "np.longdouble carries no extended precision on this platform"
    wl = np.asarray(w, dtype=np.float64).astype(LD)
    A = wl[:, None] * dense(F).astype(LD)
    X = (A + A.T) / LD(2)
    for _ in range(k):
        u = wl / X.sum(axis=1)
        X = X * ((u[:, None] + u[None, :]) / LD(2))
    return X / X.sum(axis=1)[:, None]


def defect_ld(F, w, p):
    """The reciprocity defect delta_R_X after build_X, hunger and p x (scale,
    hunger), in extended precision:
        delta = |t|_2,  t_ij = X_ij (u_i - u_j) / sqrt(w_i^2 + w_j^2),  i < j,
    and |s|_2 with s_ij = |X_ij| (|u_i| + |u_j|) / sqrt(w_i^2 + w_j^2), which
    measures how far rounding errors of u move delta (defect_bound)."""
    wl = np.asarray(w, dtype=np.float64).astype(LD)
    A = wl[:, None] * dense(F).astype(LD)
    X = (A + A.T) / LD(2)
    u = wl / X.sum(axis=1)
    for _ in range(p):
        X = X * ((u[:, None] + u[None, :]) / LD(2))
        u = wl / X.sum(axis=1)
    i, j = np.triu_indices(len(wl), 1)
    den = np.sqrt(wl[i] ** 2 + wl[j] ** 2)
    t = X[i, j] * (u[i] - u[j]) / den
    s = np.abs(X[i, j]) * (np.abs(u[i]) + np.abs(u[j])) / den
    return float(np.sqrt(np.sum(t * t))), float(np.sqrt(np.sum(s * s)))


def defect_bound(n, p, delta, s_norm):
    """First-order bound on |delta_device - delta| from the device code
    (csrc/rthx_smooth_kernels.hip), every count in units of eps = 2 u, so with
    a factor 2 in hand.
      a_p  roundings an entry of X has been through: 2 after build_X (w F, the
           halved sum), and per scale pass 2 more (u_i + u_j, the product;
           the halving is exact) plus the error b of the u's
      b_p  of u = w / r: the row sum's longest addition chain -- ap_sym_tile 1
           (the lane's pair) + 6 (wave_sum8) + 4 (wave totals), k_ap_sym_reduce
           at most 3 partials a slice + 8 slices: 22; the sparse k_sp_step's
           is shorter -- one division, and the entries' own a_p
      5    the roundings of t_ij itself (u_i - u_j, the product, w_i^2 + w_j^2,
           the quotient, the square)
      c    the sum over pairs: k_delta_rows ceil(n / 256) + 6 + 4, k_dot
           ceil(n / 1024) + 6 + 16
    |delta_device - delta| <= eps ((a_p + 5 + c) delta + b_p |s|_2)."""
    a = 2
    b = 22 + 1 + a
    for _ in range(p):
        a = a + 2 + b
        b = 22 + 1 + a
    c = -(-n // 256) + 10 + -(-n // 1024) + 22
    return EPS * ((a + 5 + c) * delta + b * s_norm)


def rel_distance(F, F_ld):
    """Largest entrywise |F - F_ld| / |F_ld| in units of eps (entries that are
    0 in both count 0; an entry that is 0 in one only counts inf)."""
    F = dense(F).astype(LD)
    d = np.abs(F - F_ld)
    nz = F_ld != 0
    out = float(np.max(d[nz] / np.abs(F_ld[nz]), initial=0.0)) / EPS
    return math.inf if np.any(d[~nz] != 0) else out


def gmres_restarted(M, h, memory=50, rtol=1e-12, atol=math.sqrt(EPS), itmax=0):
    """Plain numpy GMRES(memory) from a zero guess with the stopping rule of
    csrc/rthx_solve.cpp gmres(): tol = atol + rtol |h|; a cycle ends after
    `memory` steps, at itmax (0: 2n), when the Givens estimate of the residual
    is <= tol, or at a breakdown; cycles repeat while the true residual
    |h - M x| > tol.  Modified Gram-Schmidt.  Returns (x, iterations, cycles)."""
    M = np.asarray(M, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    n = len(h)
    m = max(1, memory)
    itmax = itmax if itmax > 0 else 2 * n
    tol = atol + rtol * np.linalg.norm(h)
    x = np.zeros(n)
    r = h.copy()
    beta = np.linalg.norm(r)
    iters = cycles = 0
    while beta > tol and iters < itmax:
        cycles += 1
        V = np.zeros((m + 1, n))
        H = np.zeros((m + 1, m))
        cs, sn, g = np.zeros(m), np.zeros(m), np.zeros(m + 1)
        V[0] = r / beta
        g[0] = beta
        k = 0
        while k < m and iters < itmax:
            w = M @ V[k]
            for i in range(k + 1):
                H[i, k] = V[i] @ w
                w = w - H[i, k] * V[i]
            hn = np.linalg.norm(w)
            H[k + 1, k] = hn
            if hn > 0:
                V[k + 1] = w / hn
            for i in range(k):
                t = cs[i] * H[i, k] + sn[i] * H[i + 1, k]
                H[i + 1, k] = -sn[i] * H[i, k] + cs[i] * H[i + 1, k]
                H[i, k] = t
            den = math.hypot(H[k, k], H[k + 1, k])
            cs[k], sn[k] = (H[k, k] / den, H[k + 1, k] / den) if den > 0 else (1.0, 0.0)
            H[k, k], H[k + 1, k] = den, 0.0
            g[k + 1] = -sn[k] * g[k]
            g[k] = cs[k] * g[k]
            iters += 1
            k += 1
            if abs(g[k]) <= tol or hn == 0.0:
                break
        y = np.linalg.solve(np.triu(H[:k, :k]), g[:k])
        x = x + V[:k].T @ y
        r = h - M @ x
        beta = np.linalg.norm(r)
    return x, iters, cycles


def chain_system(n, c):
    """(F, coeff, h, M) of the GMRES control-flow cases: F = chain_F(n),
    coeff = c, h = U(0, 1) + 0.1, M = I - c F'."""
    F = chain_F(n)
    h = np.random.default_rng(n).random(n) + 0.1
    return F, np.full(n, float(c)), h, np.eye(n) - c * F.T


DEFAULT_TOL = dict(rtol=1e-12, atol=math.sqrt(EPS))  # the reference's GMRES call
RTOL_ONLY = dict(rtol=1e-12, atol=0.0)
# (name, c, memory, tolerances): cases that converge after at least one restart
GMRES_RESTARTING = [
    ("short_memory", 0.9, 5, DEFAULT_TOL),
    ("reference_memory", 0.99, 50, RTOL_ONLY),
    ("memory_1", 0.9, 1, DEFAULT_TOL),
]
# c = 0.99 with memory 5 stalls: n -> tolerances under which 2 n steps do not
# reach the tolerance.  At n = 129 the residual after 258 steps is 960 times
# the default tolerance.  At n = 257 the default atol = sqrt(eps) is reached at
# step 410 of 514 (0.97 of the tolerance; that run is kept as a converging
# case), so the exhausted cap is run with atol = 0, where the residual after
# 514 steps is 8.5 times the tolerance.
GMRES_STALLING = {129: DEFAULT_TOL, 257: RTOL_ONLY}


# ---------------------------------------------------------------------------
# exact products and the rounding bounds of the device operator F' x
# ---------------------------------------------------------------------------
def ftx_exact(F, x):
    """(F' x, sum_k |F_ki x_k|) in extended precision, both length n."""
    Fd = dense(F).astype(LD)
    xl = np.asarray(x, dtype=np.float64).astype(LD)
    P = Fd * xl[:, None]
    return P.sum(axis=0), np.abs(P).sum(axis=0)


def ftx_chain(F, form):
    """Per output i, the longest addition chain of the device's F' x plus one
    (the product's own rounding), from csrc/rthx_solve_kernels.hip:
      dense   k_ftx_part adds 128 rows in sequence, k_ftx_reduce the
              ceil(n / 128) chunk sums:                  128 + ceil(n / 128)
      sparse  k_spmv: each lane adds ceil(len / 64) products of the row of F'
              (len = entries in column i of F), then a 6-step butterfly:
                                                         ceil(len / 64) + 6
    With m such additions the computed sum differs from the exact one by at
    most gamma_m sum |terms| < m eps sum |terms| (eps = 2 u: a factor 2 in hand)."""
    n = F.shape[0]
    if form == "dense":
        return np.full(n, 128 + -(-n // 128) + 1)
    pop = np.diff(sp.csc_matrix(F).indptr)
    return -(-pop // 64) + 6 + 1


def dot_chain(n):
    """k_multidot: ceil(n / 256) products per lane, 6 butterfly steps, 3
    additions of the wave totals, plus one for the product."""
    return -(-n // 256) + 6 + 3 + 1
