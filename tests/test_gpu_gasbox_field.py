"""The gas box with one extinction coefficient per voxel on the GPU
(rthx_gasbox_trace_field, rthx.gasbox.VoxelGasBox3D).  The
lattice walk is pinned

* statistically to the delta-tracking restatement (tests/gasbox_field_ref.py),
  which never looks at a cell boundary: the two-sample homogeneity statistic of
  tests/helpers.py summed over all rows against ``chi2.isf(1e-7, dof)``, with
  three negative controls that must exceed it (the field reversed along x,
  the field times 1.03, and the uniform kernel at the field's mean beta);
* to the uniform kernel, whose rays a uniform field must send one for one;
* to Gauss-Legendre quadrature with the closed-form optical depth of a layered
  field, to reciprocity, to the isothermal enclosure and to the optically thin
  limit with kappa differing fourfold between neighbours;

and exactly only to itself: emitter ranges, strides, ray ranges, the row split
and the three row-count forms change no count, and a voxel with beta = 0
absorbs nothing.
"""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.stats

import gasbox_field_ref as GF
import gasbox_ref as G
import helpers as H
from rthx import GasBox3D, VoxelGasBox3D, _lib, abi
from rthx.equilibrium import solve_equilibrium

pytestmark = pytest.mark.gpu

P_BOUND = 1e-7
LO, HI, N3 = (0.0, 0.0, 0.0), (1.0, 0.9, 0.5), (4, 3, 2)  # unequal n and L: an axis or face mix-up shows
R_DIST = 200_000
# beta[c_x, c_y, c_z]: one x-slab transparent, a 12-fold contrast along x, gradients along y and z
FIELD = (np.array([0.0, 0.5, 2.0, 6.0])[:, None, None] * (1.0 + 0.5 * np.arange(3))[None, :, None]
         * np.array([1.0, 0.6])[None, None, :])


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
def field_box(hip):
    box = VoxelGasBox3D(LO, HI, N3, kappa=0.75 * FIELD, sigma_s=0.25 * FIELD)
    assert box.num_elements == 76 and np.array_equal(box.beta, GF.FieldBox(LO, HI, N3, FIELD).beta_elements())
    yield box
    box.close()


@pytest.fixture(scope="module")
def reference_counts():
    """The delta-tracking restatement's 76 rows of 2e5 rays, traced once."""
    ref = GF.FieldBox(LO, HI, N3, FIELD)
    return ref.trace(range(ref.N), R_DIST, seed=4243)


@pytest.fixture(scope="module")
def gpu_counts(field_box):
    return {f: traced(field_box, R_DIST, seed=11, faithful=f) for f in (False, True)}


def statistic(A, reference, what):
    x2, dof = H.homogeneity(A, reference)
    bound = scipy.stats.chi2.isf(P_BOUND, dof)
    print(f"{what}: X2 {x2:.1f} dof {dof} z {(x2 - dof) / math.sqrt(2 * dof):+.2f} bound {bound:.1f}")
    return x2, bound


@pytest.mark.parametrize("faithful", [False, True])
def test_distribution_matches_the_restatement(gpu_counts, reference_counts, faithful):
    """A numpy lattice walk against the restatement (CPU): X2 4682, bound 5186
    (dof 4666)."""
    A, info = gpu_counts[faithful]
    assert info["lost_total"] == 0 and np.all(A.sum(axis=1) == R_DIST)
    x2, bound = statistic(A, reference_counts, f"faithful={faithful}")
    assert x2 <= bound, (x2, bound)


def test_negative_control_reversed_field(field_box, reference_counts):
    """The field reversed along x (CPU against CPU: 1.5e7)."""
    A, _ = traced(field_box, R_DIST, seed=11, beta=FIELD[::-1])
    x2, bound = statistic(A, reference_counts, "reversed along x")
    assert x2 > bound, (x2, bound)


def test_negative_control_scaled_field(field_box, reference_counts):
    """The field times 1.03 (CPU against CPU: 6840 against 5176)."""
    A, _ = traced(field_box, R_DIST, seed=11, beta=1.03 * FIELD)
    x2, bound = statistic(A, reference_counts, "1.03 beta")
    assert x2 > bound, (x2, bound)


def test_negative_control_uniform_kernel(hip, reference_counts):
    """The uniform kernel at the field's mean beta (CPU against CPU: 5.8e6):
    what the box could do before it took a field."""
    box = GasBox3D(LO, HI, N3, kappa=float(FIELD.mean()))
    try:
        A, _ = traced(box, R_DIST, seed=11)
    finally:
        box.close()
    x2, bound = statistic(A, reference_counts, "uniform kernel at the mean beta")
    assert x2 > bound, (x2, bound)


def test_uniform_field_sends_the_uniform_kernels_rays(hip):
    """A uniform field of beta = 2 and the uniform kernel at beta = 2 with one
    seed trace the same rays; a ray's column may differ only where rounding
    decides (the walk sums beta seg cell by cell and divides by d per plane,
    the uniform ray multiplies one free path by 1 / beta): at most 1e-6 of all
    rays.  A numpy walk against the numpy uniform ray: 0 of 1.52e7.  Measured
    on the MI355X: 0 of 1.52e7 in both sampling modes."""
    uni = GasBox3D(LO, HI, N3, kappa=1.5, sigma_s=0.5)
    vox = VoxelGasBox3D(LO, HI, N3, kappa=np.full(N3, 1.5), sigma_s=0.5)
    try:
        for faithful in (False, True):
            A, _ = traced(uni, R_DIST, seed=11, faithful=faithful)
            Bc, info = traced(vox, R_DIST, seed=11, faithful=faithful)
            moved = int(np.abs(A - Bc).sum()) // 2
            print(f"faithful={faithful}: {moved} of {A.sum()} rays end in another column")
            assert info["lost_total"] == 0 and A.sum() == Bc.sum() == 76 * R_DIST
            assert moved <= 1e-6 * A.sum()
    finally:
        uni.close()
        vox.close()


def test_transparent_voxels_absorb_nothing(field_box, gpu_counts):
    ns = field_box.n_surfaces
    clear = np.flatnonzero(field_box.beta == 0.0)
    assert clear.size == 6  # the slab c_x = 0
    for faithful in (False, True):
        A, info = gpu_counts[faithful]
        assert info["lost_total"] == 0 and info["lost_max_row"] == 0 and np.all(A.sum(axis=1) == R_DIST)
        assert not A[:, ns + clear].any()
        assert np.all(A[:, ns + np.flatnonzero(field_box.beta > 0.0)].sum(axis=0) > 0)
    # an all-zero field is the transparent box: no gas column at all, and the uniform kernel's counts at beta = 0
    Z, info = traced(field_box, 20_000, seed=3, beta=0.0)
    assert info["lost_total"] == 0 and np.all(Z.sum(axis=1) == 20_000) and not Z[:, ns:].any()
    uni = GasBox3D(LO, HI, N3, kappa=0.0)
    try:
        U, _ = traced(uni, 20_000, seed=3)
    finally:
        uni.close()
    assert int(np.abs(Z - U).sum()) // 2 <= 1e-6 * Z.sum()  # (exit planes lo + n h against hi: rounding only)


def test_layered_quadrature(hip):
    """3 x 3 x 3 unit cube, beta_z = (0.5, 3, 1), 4e6 rays from voxel (0, 0, 0),
    wall cell z-(0, 0) and wall cell x-(1, 1): every column at least one cell
    away within 5 sigma (binomial) of the quadrature with the layered field's
    closed-form optical depth."""
    ref = GF.layered_box()
    rows = GF.layered_rows(ref)
    box = VoxelGasBox3D((0, 0, 0), (1, 1, 1), (3, 3, 3), kappa=ref.beta)
    R = 4_000_000
    counts = []
    try:
        for i in rows:
            A, info = traced(box, R, seed=5, emitter_begin=i, emitter_end=i + 1)
            assert info["rows_traced"] == 1 and A[i].sum() == R and A.sum() == R
            counts.append(A[i])
    finally:
        box.close()
    worst, pairs = GF.check_rows_against_layered_quadrature(ref, rows, np.array(counts), R)
    print(f"worst |z| against the layered quadrature {worst:.2f} over {pairs} pairs")


def test_reciprocity(field_box, gpu_counts):
    """w_i F_ij = w_j F_ji with w = wall areas, 4 beta_v V, over pairs with at
    least 50 counts and w > 0 (a numpy walk: worst |z| 4.07 over 2128 pairs)."""
    A, _ = gpu_counts[False]
    w = np.concatenate([field_box.areas(), 4.0 * field_box.beta * field_box.volume()])
    i, j = np.triu_indices(len(w), 1)
    cij, cji = A[i, j].astype(float), A[j, i].astype(float)
    keep = (cij + cji >= 50) & (w[i] > 0.0) & (w[j] > 0.0)
    num = w[i] * cij - w[j] * cji
    var = w[i] ** 2 * cij + w[j] ** 2 * cji
    z = num[keep] / np.sqrt(var[keep])
    print(f"reciprocity: worst |z| {np.abs(z).max():.2f} over {keep.sum()} pairs")
    assert keep.sum() > 1000 and np.abs(z).max() <= 5.0


def test_exact(field_box, monkeypatch):
    """What must hold to the count: closure, repeatability, independence of
    the emitter range and stride, of the row split and of the row-count form
    (u16 and u32 LDS histograms, the global form), ray ranges folded with
    accumulate, and sampling_error on the result."""
    box = field_box
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
    # the field is read at every call: another field, then the first again
    A1, _ = traced(box, R, seed=9)
    A2, _ = traced(box, R, seed=9, beta=2.0 * FIELD)
    assert not np.array_equal(A1, A2) and np.array_equal(traced(box, R, seed=9)[0], A1)


def test_u32_and_u16_histograms_agree(field_box, monkeypatch):
    """R >= 65536 on two rows (a wall cell and a voxel): unsplit, a workgroup
    counts in u32; split as planned its parts count in u16; the global form
    counts in the dense row.  Identical counts."""
    box = field_box
    R = 70_000
    rows = dict(emitter_begin=51, emitter_end=53)  # the last wall cell and the first voxel
    A, info = traced(box, R, seed=2, **rows)
    assert info["rows_traced"] == 2 and np.all(A[51:53].sum(axis=1) == R) and A.sum() == 2 * R
    monkeypatch.setenv("RTHX_GASBOX_SPLIT", "1")
    assert np.array_equal(traced(box, R, seed=2, **rows)[0], A)
    monkeypatch.setenv("RTHX_GASBOX_GHIST", "1")
    assert np.array_equal(traced(box, R, seed=2, **rows)[0], A)


def test_field_length_is_checked(field_box):
    """n_beta != Nv needs the box, so it is checked here: RTHX_EINVAL, and the
    result stays unused."""
    lib = _lib.load()
    args, _keep = _lib.make_args(0, 100, 0.0, 1, 0, 76, 1, 0, abi.RTHX_FLAG_DEVICE_ONLY)
    res = _lib.DeviceResult()
    try:
        for n_beta in (23, 25, 76):
            f = np.ones(n_beta)
            rc = lib.rthx_gasbox_trace_field(field_box._handle(0), C.byref(args), abi.ptr(f, C.c_double), n_beta, 0,
                                             res.handle)
            assert rc == abi.RTHX_EINVAL and "n_beta" in lib.rthx_last_error().decode()
        f = np.ones(24)
        assert lib.rthx_gasbox_trace_field(field_box._handle(0), C.byref(args), abi.ptr(f, C.c_double), 24, 0,
                                           res.handle) == 0
        assert res.info()["rays_traced"] == 7600
    finally:
        res.close()


def test_isothermal_enclosure(hip):
    """Grey walls (eps = 0.7) at 1000 K, a gas whose kappa and sigma_s both
    differ from voxel to voxel, in radiative equilibrium with q = 0: every
    voxel sits at 1000 K.  Exact for any reciprocal, conservative F; the slack
    covers the smoothing's 8 eps defect and GMRES's 1e-12."""
    kappa = 0.2 + 0.5 * FIELD          # 0.2 ... 9.2
    sigma_s = 0.1 + 0.25 * FIELD[::-1]  # (runs against kappa: omega from 0.01 to 0.94)
    box = VoxelGasBox3D(LO, HI, N3, kappa=kappa, sigma_s=sigma_s, epsilon=0.7, T_in_w=1000.0, T_in_g=-1.0, q_in_g=0.0)
    try:
        box(76 * 20_000, seed=1)
        assert box.last_smooth_info["converged"]
        solve_equilibrium(box)
        assert box.last_solve_info["converged"] and box.last_solve_info["F_form"].startswith("smoothed")
        Fs = box.F_smooth
        Fs = Fs.toarray() if sp.issparse(Fs) else Fs
    finally:
        box.close()
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


def test_optically_thin_heterogeneous_gas(hip):
    """Unit cube 3 x 3 x 3, kappa_v = 1e-3 (0.5, 1, 2)[(c_x + c_y + c_z) mod 3],
    black walls, z- at 1000 K and the rest at 0 K, gas in radiative
    equilibrium, R = 1e5: each voxel's (T_g / 1000)^4 is the quadrature value
    of F(voxel -> z- face) within 5 sigma (binomial at R) + 2e-3
    (tests/gasbox_field_ref.py thin_reference says what the 2e-3 covers;
    on the CPU the restatement's counts land at 0.25 of the tolerance, the
    device's at 0.41)."""
    n = (3, 3, 3)
    Tw = [0.0, 0.0, 0.0, 0.0, 1000.0, 0.0]
    box = VoxelGasBox3D((0, 0, 0), (1, 1, 1), n, kappa=GF.thin_field(), epsilon=1.0, T_in_w=Tw, T_in_g=-1.0, q_in_g=0.0)
    R = 100_000
    try:
        box(box.num_elements * R, seed=1)
        solve_equilibrium(box)
    finally:
        box.close()
    assert box.last_smooth_info["k_dykstra"] == 1 and box.last_smooth_info["converged"]
    ref = G.Box((0, 0, 0), (1, 1, 1), n)
    q, tol = GF.thin_reference(ref, R)
    got = (box.T_g / 1000.0) ** 4
    ratio = np.abs(got - q) / tol
    print(f"optically thin, heterogeneous: worst |deviation| / tolerance {ratio.max():.3f}")
    assert np.all(ratio <= 1.0), list(zip(got, q, tol))
