"""Dense numpy restatement of the reference's spectral GERT solve
(equilibriumSpectral2D.jl, equilibriumSurfacesSpectral3D.jl), for the tests
of rthx_solve_spectral.  Test infrastructure only.

The reference's algorithm, as restated here: a Picard iteration on the
emitted power e.  Each sweep solves, in the least-squares sense and by one QR
of the fixed (K + 1) n x K n matrix,

    top stripe      sum_k M_k j_k = h,       M_k = I - diag(coeff_k) F_k'
                                             (coeff = 1 where the heat is
                                             prescribed, b_k elsewhere;
                                             buildSystemMatrix.jl),
                                             h = e_i or q_i
    bottom stripes  D_k j_k = e .* f_k(T),   D_k = I - diag(b_k) F_k'

with the weighted fractions f of the current temperatures on the right, then
e = max(sum_k D_k j_k, 10 eps) (updateSpectralEmission.jl), then the
temperatures of the radiative-equilibrium elements from e with the plain
fractions of the previous temperatures (updateTemperaturesSpectral.jl), until
||j - j_prev|| / ||j|| < 1e-14.
"""
import numpy as np

from rthx import PolyVolume2D, RayTracingDomain2D
from rthx.direct import bins_emission_fractions
from rthx.equilibrium import STEFAN_BOLTZMANN, populate_workspace


def plain_fractions(limits, T):
    """w[K, n]: getBinsEmissionFractions, band-major."""
    return bins_emission_fractions(limits, len(limits) - 1, T).T.copy()


def weighted_fractions(limits, T, prop):
    """f[K, n] = prop .* w / sum_k(prop .* w) (getWeightedEmissionFractions;
    left as prop .* w where the sum is 0)."""
    out = prop * plain_fractions(limits, T)
    s = out.sum(axis=0)
    pos = s > 0
    out[:, pos] /= s[pos]
    return out


def dense(F):
    return np.asarray(F.toarray() if hasattr(F, "toarray") else F, dtype=np.float64)


def reference_solve(F, limits, b, prop, size, T_in, q_in, tol=1e-14, max_sweeps=20000):
    """The restatement.  F: one matrix or a list of K; b, prop: [K, n].
    Returns (j[K, n], T[n], e[n], sweeps)."""
    K, n = b.shape
    Fs = [dense(m)[:n, :n] for m in (F if isinstance(F, (list, tuple)) else [F] * K)]
    P = T_in > -0.1
    T = np.where(P, T_in, np.max(T_in[P]))
    w = plain_fractions(limits, T)
    e = size * STEFAN_BOLTZMANN * T ** 4 * np.sum(prop * w, axis=0)  # setupBoundaryConditions.jl:31-54
    h = np.where(P, e, q_in)
    A = np.zeros(((K + 1) * n, K * n))
    for k in range(K):
        coeff = np.where(P, b[k], 1.0)
        A[:n, k * n:(k + 1) * n] = np.eye(n) - coeff[:, None] * Fs[k].T
        A[(k + 1) * n:(k + 2) * n, k * n:(k + 1) * n] = np.eye(n) - b[k][:, None] * Fs[k].T
    Q, R = np.linalg.qr(A)
    j_prev = np.zeros(K * n)
    for sweep in range(1, max_sweeps + 1):
        f = weighted_fractions(limits, T, prop)
        rhs = np.concatenate([h, (e[None, :] * f).ravel()])
        j = np.linalg.solve(R, Q.T @ rhs)
        jk = j.reshape(K, n)
        g = np.array([Fs[k].T @ jk[k] for k in range(K)])
        e = np.maximum(np.sum(jk - b * g, axis=0), 10 * np.finfo(np.float64).eps)
        w = plain_fractions(limits, T)  # of the previous temperatures
        den = size * STEFAN_BOLTZMANN * np.sum(prop * w, axis=0)
        T = np.where(P, T_in, (e / np.where(den > 0, den, 1.0)) ** 0.25)
        if np.linalg.norm(j - j_prev) < tol * np.linalg.norm(j):
            return jk, T, e, sweep
        j_prev = j
    raise RuntimeError(f"restatement not converged in {max_sweeps} sweeps")


def reciprocal_F(weights, rng):
    """A synthetic exchange-factor matrix: rows sum to 1 and weights_i F_ij is
    symmetric (a symmetric random matrix Sinkhorn-scaled to row sums
    `weights`)."""
    n = len(weights)
    S = rng.random((n, n)) + 0.1
    S = S + S.T
    d = np.ones(n)
    for _ in range(5000):
        d_new = np.sqrt(d * weights / (S @ d))
        if np.max(np.abs(d_new - d)) < 1e-16 * np.max(d):
            d = d_new
            break
        d = d_new
    X = d[:, None] * S * d[None, :]
    X = 0.5 * (X + X.T)
    return X / X.sum(axis=1, keepdims=True)


def spectral_square(ndim, n_bins, kappa, epsilon, T_walls=(1000.0, 0.0, 0.0, 0.0), q_walls=(0.0,) * 4, T_in_g=-1.0,
                    q_in_g=0.0, sigma_s=0.0, limits=None):
    """A unit square cut ndim x ndim with n_bins bands: kappa, sigma_s scalars
    or per-band; epsilon a scalar, a per-band vector, or four of either."""
    per_band = lambda v: np.broadcast_to(np.asarray(v, dtype=np.float64), (n_bins,)).copy()
    face = PolyVolume2D([(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)], [True] * 4, n_bins, per_band(kappa),
                        per_band(sigma_s))
    eps = epsilon if (isinstance(epsilon, (list, tuple)) and len(epsilon) == 4 and n_bins != 4) else [epsilon] * 4
    face.epsilon = [per_band(e) for e in eps]
    face.T_in_w = list(T_walls)
    face.q_in_w = list(q_walls)
    face.T_in_g = T_in_g
    face.q_in_g = q_in_g
    dom = RayTracingDomain2D([face], [(ndim, ndim)])
    if limits is not None:
        dom.wavelength_band_limits = np.asarray(limits, dtype=np.float64)
    return dom


def domain_arrays(dom):
    """(b, prop [K, n], size, T_in, q_in [n]) of a 2D domain in global element
    order, from populateWorkspace! per band."""
    K = dom.n_spectral_bins
    wss = [populate_workspace(dom, k) for k in range(1, K + 1)]
    b = np.array([np.concatenate([1.0 - ws["epsw"], ws["omega_g"]]) for ws in wss])
    prop = np.array([np.concatenate([ws["epsw"], ws["kappa_g"]]) for ws in wss])
    size = np.concatenate([wss[0]["Area"], 4.0 * wss[0]["Volume"]])
    T_in = np.concatenate([wss[0]["Tw"], wss[0]["Tg"]])
    q_in = np.concatenate([wss[0]["qw"], wss[0]["qg"]])
    return b, prop, size, T_in, q_in
