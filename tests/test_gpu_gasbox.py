"""The 3D gas-box exchange tracer on the GPU (rthx_gasbox_trace, rthx.gasbox;
DESIGN.md §7l).  The CPU oracle has no gas in 3D, so the tracer is pinned

* statistically to the independent numpy restatement (tests/gasbox_ref.py):
  the two-sample homogeneity statistic of tests/helpers.py summed over all
  rows against ``chi2.isf(1e-7, dof)``, the mirror tests' bound, with a
  negative control (the GPU trace at 1.03 beta must exceed it);
* to Gauss-Legendre quadrature of the four kinds of exchange integral;
* to analytic limits: a transparent medium gives the 3D view factors, the
  isothermal enclosure stays isothermal, and an optically thin gas takes
  (T_g / T_wall)^4 = F(voxel -> hot face);

and exactly only to itself: emitter ranges, strides, ray ranges, the row split
and the three row-count forms change no count.
"""
import math

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.stats

import gasbox_ref as G
import helpers as H
from rthx import GasBox3D
from rthx.equilibrium import solve_equilibrium

pytestmark = pytest.mark.gpu

P_BOUND = 1e-7
LO, HI, N3 = (0.0, 0.0, 0.0), (1.0, 0.9, 0.5), (4, 3, 2)  # unequal n and L: an axis or face mix-up shows
BETA, R_DIST = 2.0, 200_000


def dense(res):
    rp, cols, cnt = res.csr()
    n = len(rp) - 1
    return sp.csr_matrix((cnt.astype(np.int64), cols, rp), shape=(n, n)).toarray()


def traced(box, R, **kw):
    res = box.trace(R, **kw)
    try:
        return dense(res), res.info()
    finally:
        res.close()


@pytest.fixture(scope="module")
def first_box(hip):
    box = GasBox3D(LO, HI, N3, kappa=1.5, sigma_s=0.5)
    assert box.beta == BETA and box.num_elements == 76
    yield box
    box.close()


@pytest.fixture(scope="module")
def reference_counts():
    """The numpy restatement's 76 rows of 2e5 rays, traced once."""
    ref = G.Box(LO, HI, N3)
    return ref.trace(range(ref.N), R_DIST, BETA, seed=4242)


@pytest.fixture(scope="module")
def gpu_counts(first_box):
    return {f: traced(first_box, R_DIST, seed=11, faithful=f) for f in (False, True)}


@pytest.mark.parametrize("faithful", [False, True])
def test_distribution_matches_the_restatement(gpu_counts, reference_counts, faithful):
    """Two independent restatements against each other (CPU): X2 5153, bound
    5760 (dof 5212)."""
    A, info = gpu_counts[faithful]
    assert info["lost_total"] == 0 and np.all(A.sum(axis=1) == R_DIST)
    x2, dof = H.homogeneity(A, reference_counts)
    bound = scipy.stats.chi2.isf(P_BOUND, dof)
    print(f"faithful={faithful}: X2 {x2:.1f} dof {dof} z {(x2 - dof) / math.sqrt(2 * dof):+.2f} bound {bound:.1f}")
    assert x2 <= bound, (x2, dof, bound)


def test_distribution_negative_control(first_box, reference_counts):
    """The same statistic must reject a 3 % error in beta (CPU against CPU: 8568)."""
    A, _ = traced(first_box, R_DIST, seed=11, beta=1.03 * BETA)
    x2, dof = H.homogeneity(A, reference_counts)
    bound = scipy.stats.chi2.isf(P_BOUND, dof)
    print(f"1.03 beta: X2 {x2:.1f} dof {dof} bound {bound:.1f}")
    assert x2 > bound, (x2, dof, bound)


def test_quadrature(hip):
    """3 x 3 x 3 unit cube, beta = 1.5, 4e6 rays from voxel (0, 0, 0) and from
    wall cell z-(0, 0): every column at least one cell away within 5 sigma
    (binomial) of the Gauss-Legendre value of its pair integral."""
    ref = G.Box((0, 0, 0), (1, 1, 1), (3, 3, 3))
    box = GasBox3D((0, 0, 0), (1, 1, 1), (3, 3, 3), kappa=1.5)
    R = 4_000_000
    worst, kinds = 0.0, set()
    try:
        for i in (ref.volume_index(0, 0, 0), ref.wall_index(4, 0, 0)):
            A, info = traced(box, R, seed=5, emitter_begin=i, emitter_end=i + 1)
            assert info["rows_traced"] == 1 and A[i].sum() == R and A.sum() == R
            for j in range(ref.N):
                if not ref.separated(i, j):
                    continue
                q = ref.pair_integral(i, j, 1.5)
                if q == 0.0:  # (coplanar wall cells)
                    assert A[i, j] == 0
                    continue
                z = (A[i, j] / R - q) / math.sqrt(q * (1.0 - q) / R)
                worst = max(worst, abs(z))
                kinds.add((ref.element(i)[0], ref.element(j)[0]))
                assert abs(z) <= 5.0, (i, j, A[i, j] / R, q, z)
    finally:
        box.close()
    print(f"worst |z| against quadrature {worst:.2f}")
    assert len(kinds) == 4


def test_transparent_limit(hip):
    """beta = 0: no ray ends in the gas, wall rows are the analytic 3D view
    factors of the wall quads (coplanar pairs exactly 0) within 5 sigma, and
    volume rows hit walls only."""
    from rthx.domain3d import view_factors_3d

    box = GasBox3D(LO, HI, N3, kappa=0.0)
    R = 100_000
    try:
        A, info = traced(box, R, seed=3)
        xyz, nv, _normals = box.polygon_arrays()
        F, area, _ = view_factors_3d(xyz, nv)
    finally:
        box.close()
    ns = box.n_surfaces
    assert info["lost_total"] == 0 and np.all(A.sum(axis=1) == R)
    assert not A[:, ns:].any()  # every gas column is zero, volume rows included
    assert np.allclose(area, box.areas(), rtol=1e-12)
    ref = G.Box(LO, HI, N3)
    face = np.array([ref.element(g)[1] for g in range(ns)])
    coplanar = face[:, None] == face[None, :]
    assert not A[:ns, :ns][coplanar].any()
    p = F[~coplanar]
    z = (A[:ns, :ns][~coplanar] / R - p) / np.sqrt(p * (1.0 - p) / R)
    print(f"worst |z| against the analytic view factors {np.abs(z).max():.2f} over {z.size} pairs")
    assert np.abs(z).max() <= 5.0


def test_exact(first_box, monkeypatch):
    """What must hold to the count: closure, repeatability, independence of
    the emitter range and stride, of the row split and of the row-count form
    (u16 and u32 LDS histograms, the global form), ray ranges folded with
    accumulate, and sampling_error on the result."""
    box = first_box
    N, R = box.num_elements, 5000
    for faithful in (False, True):
        res = box.trace(R, seed=9, faithful=faithful)
        A, info = dense(res), res.info()
        rms, mx = res.sampling_error()
        assert 0.0 < rms < mx < 1.0 / math.sqrt(R)
        assert info["lost_total"] == 0 and info["lost_max_row"] == 0 and info["rays_traced"] == N * R
        assert info["n_emitters"] == N and info["rows_traced"] == N and info["nnz"] == np.count_nonzero(A)
        assert np.all(A.sum(axis=1) == R)
        res2 = box.trace(R, seed=9, faithful=faithful)
        for x, y in zip(res.csr(), res2.csr()):  # the same call twice: the same CSR
            assert np.array_equal(x, y)
        res2.close()
        # emitter range and stride
        S, sinfo = traced(box, R, seed=9, faithful=faithful, emitter_begin=3, emitter_end=70, emitter_stride=7)
        full = np.zeros_like(A)
        full[3:70:7] = A[3:70:7]
        assert np.array_equal(S, full) and sinfo["rows_traced"] == len(range(3, 70, 7))
        # row split (the natural split of R = 5000 over 76 rows is 4), unsplit, and a split that leaves parts of 1 and 2 rays
        for split in ("1", "3", "2500"):
            monkeypatch.setenv("RTHX_GASBOX_SPLIT", split)
            assert np.array_equal(traced(box, R, seed=9, faithful=faithful)[0], A), split
        monkeypatch.delenv("RTHX_GASBOX_SPLIT")
        # the global form, and the LDS histogram where the plan would not take it (2-ray parts)
        monkeypatch.setenv("RTHX_GASBOX_GHIST", "1")
        assert np.array_equal(traced(box, R, seed=9, faithful=faithful)[0], A)
        monkeypatch.setenv("RTHX_GASBOX_GHIST", "0")
        monkeypatch.setenv("RTHX_GASBOX_SPLIT", "2500")
        assert np.array_equal(traced(box, R, seed=9, faithful=faithful)[0], A)
        monkeypatch.delenv("RTHX_GASBOX_SPLIT")
        monkeypatch.delenv("RTHX_GASBOX_GHIST")
        # three ray ranges cut off multiples of four, folded on the device
        acc = box.trace(1001, seed=9, faithful=faithful)
        for b, e in ((1001, 2503), (2503, R)):
            part = box.trace(e - b, seed=9, faithful=faithful, ray_begin=b)
            acc.accumulate(part)
            part.close()
        assert acc.info()["rays_per_emitter"] == R and acc.info()["lost_total"] == 0
        for x, y in zip(res.csr(), acc.csr()):
            assert np.array_equal(x, y)
        acc.close()
        res.close()


def test_u32_and_u16_histograms_agree(first_box, monkeypatch):
    """R >= 65536 on two rows (a wall cell and a voxel): unsplit, a workgroup
    counts in u32; split as planned its parts count in u16; the global form
    counts in the dense row.  Identical counts."""
    box = first_box
    R = 70_000
    rows = dict(emitter_begin=51, emitter_end=53)  # the last wall cell and the first voxel
    A, info = traced(box, R, seed=2, **rows)
    assert info["rows_traced"] == 2 and np.all(A[51:53].sum(axis=1) == R) and A.sum() == 2 * R
    monkeypatch.setenv("RTHX_GASBOX_SPLIT", "1")
    assert np.array_equal(traced(box, R, seed=2, **rows)[0], A)
    monkeypatch.setenv("RTHX_GASBOX_GHIST", "1")
    assert np.array_equal(traced(box, R, seed=2, **rows)[0], A)


def test_reciprocity(first_box, gpu_counts):
    """w_i F_ij = w_j F_ji with w = weights() (wall areas, 4 beta V): z-scores
    of the count pairs over pairs whose counts sum to at least 50."""
    A, _ = gpu_counts[False]
    w = first_box.weights()
    # (counts of R rays a row: under reciprocity w_i c_ij - w_j c_ji has mean 0 and, Poisson, variance w_i^2 c_ij + w_j^2 c_ji)
    i, j = np.triu_indices(len(w), 1)
    cij, cji = A[i, j].astype(float), A[j, i].astype(float)
    keep = cij + cji >= 50
    num = w[i] * cij - w[j] * cji
    var = w[i] ** 2 * cij + w[j] ** 2 * cji
    z = num[keep] / np.sqrt(var[keep])
    print(f"reciprocity: worst |z| {np.abs(z).max():.2f} over {keep.sum()} pairs")
    assert keep.any() and np.abs(z).max() <= 5.0


def test_isothermal_enclosure(hip):
    """Grey walls (eps = 0.7) at 1000 K, a scattering gas in radiative
    equilibrium with q = 0: every voxel sits at 1000 K.  Exact for any
    reciprocal, conservative F; the slack covers the smoothing's 8 eps defect
    and GMRES's 1e-12."""
    box = GasBox3D(LO, HI, N3, kappa=1.0, sigma_s=0.5, epsilon=0.7, T_in_w=1000.0, T_in_g=-1.0, q_in_g=0.0)
    try:
        box(76 * 20_000, seed=1)
        assert box.last_smooth_info["converged"]
        solve_equilibrium(box)
        assert box.last_solve_info["converged"] and box.last_solve_info["F_form"].startswith("smoothed")
        Fs = box.F_smooth
        Fs = Fs.toarray() if sp.issparse(Fs) else Fs
        Fr = box.F_raw  # (counts / R from the device, as every other tracer's result gives it)
    finally:
        box.close()
    assert Fr.shape == (76, 76) and np.allclose(Fr.sum(axis=1), 1.0, atol=1e-12) and Fr.nnz == box.last_trace_info["nnz"]
    assert np.allclose(Fs.sum(axis=1), 1.0, atol=1e-12)
    w = box.weights()
    assert np.allclose(w[:, None] * Fs, (w[:, None] * Fs).T, atol=1e-12)
    sigma = 5.670374419e-8
    emission = 0.7 * sigma * box.areas().sum() * 1000.0 ** 4
    dev = np.abs(box.T_g / 1000.0 - 1.0).max()
    print(f"isothermal: max |T_g / 1000 - 1| {dev:.3e}, energy error / emission {box.energy_error / emission:.3e}")
    assert dev <= 1e-6
    assert abs(box.energy_error) <= 1e-6 * emission
    assert np.all(box.T_w == 1000.0) and np.allclose(box.q_g, 0.0)
    assert np.abs(box.q_w).max() <= 1e-6 * emission  # nothing flows between equal temperatures


def test_optically_thin_gas(hip):
    """Unit cube 3 x 3 x 3, kappa = 1e-3, black walls, z- at 1000 K and the
    rest at 0 K, gas in radiative equilibrium, R = 1e5: each voxel's
    (T_g / 1000)^4 is the quadrature value of F(voxel -> z- face) within
    5 sigma (binomial at R) + 2e-3, the latter bounding the neglected gas-gas
    exchange, 1 - exp(-kappa * diagonal) <= 1.8e-3.

    The box smooths with one Dykstra round (GasBox3D.__call__ says why): a wall
    row sends about 30 of its 1e5 rays into so thin a gas, and smooth_F's
    plain alternating projection, which starts from the equal-weight mean of
    the two directions' estimates, keeps half of that noise and misses this
    bound about 4-fold (tests/test_gasbox_host.py shows both on the CPU)."""
    n = (3, 3, 3)
    Tw = [0.0, 0.0, 0.0, 0.0, 1000.0, 0.0]
    box = GasBox3D((0, 0, 0), (1, 1, 1), n, kappa=1e-3, epsilon=1.0, T_in_w=Tw, T_in_g=-1.0, q_in_g=0.0)
    R = 100_000
    try:
        box(box.num_elements * R, seed=1)
        solve_equilibrium(box)
    finally:
        box.close()
    assert box.last_smooth_info["k_dykstra"] == 1 and box.last_smooth_info["converged"]
    ref = G.Box((0, 0, 0), (1, 1, 1), n)
    worst = 0.0
    bad = []
    for v in range(ref.Nv):
        q = ref.volume_to_face(ref.Ns + v, 4, 1e-3)
        got = (box.T_g[v] / 1000.0) ** 4
        tol = 5.0 * math.sqrt(q * (1.0 - q) / R) + 2e-3
        worst = max(worst, abs(got - q) / tol)
        print(f"voxel {ref.element(ref.Ns + v)[2]}: (T_g/1000)^4 {got:.5f} quadrature {q:.5f} diff {got - q:+.2e} tol {tol:.2e}")
        if abs(got - q) > tol:
            bad.append((v, got, q, tol))
    print(f"optically thin: worst |deviation| / tolerance {worst:.3f}")
    assert not bad, bad
