"""The per-voxel gas box's host side (include/rthx.h rthx_gasbox_trace_field,
rthx.gasbox.VoxelGasBox3D), without a GPU: the delta-tracking
restatement (tests/gasbox_field_ref.py) against quadrature of a layered
field's exchange integrals, the ray's lattice walk (csrc/rthx_gasbox_walk.h,
the function the kernel calls) in tests/gasbox_walk_host_check.cpp, built for
the host with AddressSanitizer and UBSan and run, every argument check of the
new call, VoxelGasBox3D's broadcasting, weights and element order, the
per-voxel grey solve's assembly, and the optically thin heterogeneous gas on
the smoothing oracle."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import gasbox_field_ref as GF
import gasbox_ref as G
from rthx import GasBox3D, VoxelGasBox3D, _lib, abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-s", "-C", os.path.dirname(os.path.dirname(_lib.LIB_PATH))], check=True)
    return _lib.load()


def test_restatement_matches_layered_quadrature():
    """3 x 3 x 3 unit cube, beta_z = (0.5, 3, 1), 2e6 rays from voxel (0, 0, 0),
    wall cell z-(0, 0) and wall cell x-(1, 1): the delta-tracking restatement
    against the closed-form optical depth of a layered field in the four
    exchange kernels, 5 sigma.  (A numpy lattice walk: worst |z| 3.87 over 188
    pairs; this restatement: 2.92 over 188.)"""
    box = GF.layered_box()
    rows = GF.layered_rows(box)
    R = 2_000_000
    worst, pairs = GF.check_rows_against_layered_quadrature(box, rows, box.trace(rows, R, seed=20261), R)
    print(f"worst |z| {worst:.2f} over {pairs} separated pairs")
    assert pairs == 188


def test_layered_quadrature_reduces_to_the_uniform_one():
    box = GF.FieldBox([0, 0, 0], [1, 0.9, 0.5], (4, 3, 2), np.full((4, 3, 2), 2.0))
    for i, j in ((box.volume_index(0, 0, 0), box.volume_index(3, 2, 1)), (box.wall_index(1, 2, 1), box.volume_index(0, 0, 0)),
                 (box.volume_index(1, 1, 0), box.wall_index(5, 3, 2)), (box.wall_index(0, 0, 0), box.wall_index(3, 3, 1))):
        assert box.pair_integral_layered(i, j) == pytest.approx(box.pair_integral(i, j, 2.0), rel=1e-12)


def test_restatement_with_a_uniform_field_is_the_uniform_law():
    """Delta tracking at beta = beta_max accepts every collision: the counts
    of a uniform field follow the uniform restatement's law (two-sample
    homogeneity at 1e-7, as the GPU tests)."""
    import scipy.stats

    import helpers as H

    lo, hi, n = (0.0, 0.0, 0.0), (1.0, 0.9, 0.5), (4, 3, 2)
    fb = GF.FieldBox(lo, hi, n, np.full(n, 2.0))
    rows = [0, 30, 52, 75]
    A = fb.trace(rows, 100_000, seed=5)
    Bc = G.Box(lo, hi, n).trace(rows, 100_000, 2.0, seed=6)
    x2, dof = H.homogeneity(A, Bc)
    assert x2 <= scipy.stats.chi2.isf(1e-7, dof), (x2, dof)


def test_walk_stays_in_range(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "gasbox_walk_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "raytraceheattransfer.jl_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "gasbox_walk_host_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"gasbox walk rays (\d+), near a crossing (\d+)", out.stdout)
    assert m and int(m.group(1)) >= 3_000_000 and int(m.group(2)) < 1e-6 * int(m.group(1)), out.stdout
    assert "gasbox walk check ok" in out.stdout
    print(out.stdout.strip())


def test_validation_without_gpu(lib):
    """Every argument error of rthx_gasbox_trace_field that needs no handle is
    reported before the first device call (a box cannot be made without a
    GPU, so n_beta != Nv is checked on the GPU, tests/test_gpu_gasbox_field.py)."""
    EINVAL, ERANGE = abi.RTHX_EINVAL, abi.RTHX_ERANGE
    r = C.c_void_p()
    assert lib.rthx_result_create(C.byref(r)) == 0
    field = np.array([0.0, 1.0, 2.5, 0.0, 1e-300, 7.0, 0.25, 3.0])

    def trace(args, beta=field, n_beta=None, ray_begin=0, box=None, res=r):
        b = None if beta is None else np.ascontiguousarray(beta, dtype=np.float64)
        rc = lib.rthx_gasbox_trace_field(box, None if args is None else C.byref(args), abi.ptr(b, C.c_double),
                                         (0 if b is None else b.size) if n_beta is None else n_beta, ray_begin, res)
        return rc, lib.rthx_last_error().decode()

    good, _ = _lib.make_args(0, 100, 0.0, 1, 0, 8)
    assert trace(None)[0] == EINVAL
    rc, msg = trace(good)  # everything but the box is fine (zeros in the field included)
    assert rc == EINVAL and "null box" in msg
    rc, msg = trace(good, beta=np.zeros(8))  # an all-zero field is legal
    assert rc == EINVAL and "null box" in msg
    rc, msg = trace(good, beta=None, n_beta=8)
    assert rc == EINVAL and "null beta" in msg
    for n_beta in (0, -1, 2 ** 31):
        rc, msg = trace(good, n_beta=n_beta)
        assert rc == EINVAL and "n_beta" in msg
    for bad in (-1.0, -1e-300, np.nan, np.inf, -np.inf):
        for at in (0, 5, 7):
            f = field.copy()
            f[at] = bad
            rc, msg = trace(good, beta=f)
            assert rc == EINVAL and "beta" in msg and "finite" in msg, (bad, at, rc, msg)
    # the checks rthx_gasbox_trace makes
    rc, msg = trace(good, ray_begin=-1)
    assert rc == EINVAL and "ray_begin" in msg
    rc, msg = trace(good, ray_begin=2 ** 32 - 100)
    assert rc == ERANGE and "2^32" in msg
    assert trace(good, ray_begin=2 ** 62)[0] == ERANGE
    a, _ = _lib.make_args(1, 100, 0.0, 1, 0, 8)
    rc, msg = trace(a)
    assert rc == EINVAL and "bin" in msg
    a, keep = _lib.make_args(0, 100, 0.0, 1, 0, 8, record_ids=[0])
    rc, msg = trace(a)
    assert rc == EINVAL and "recording" in msg
    a, _ = _lib.make_args(0, 100, 0.0, 1, 0, 8, flags=abi.RTHX_FLAG_ASYNC)
    rc, msg = trace(a)
    assert rc == EINVAL and "RTHX_FLAG" in msg
    a, _ = _lib.make_args(0, 100, 0.0, 1, 0, 8, flags=0x10)
    assert trace(a)[0] == EINVAL
    a, _ = _lib.make_args(0, 2 ** 32, 0.0, 1, 0, 8)
    assert trace(a)[0] == ERANGE
    a, _ = _lib.make_args(0, 100, 0.0, 1, 0, 8, emitter_stride=0)
    assert trace(a)[0] == EINVAL
    a, _ = _lib.make_args(0, 100, 0.0, 1, -1, 8)
    assert trace(a)[0] == EINVAL
    assert trace(good, res=None)[0] == EINVAL
    lib.rthx_result_destroy(r)


def test_header_documents_the_field_trace():
    txt = open(os.path.join(ROOT, "include", "rthx.h")).read()
    body = txt[txt.index("int rthx_gasbox_trace("):]
    assert "int rthx_gasbox_trace_field(" in body  # (documented after rthx_gasbox_trace)
    for phrase in ("lo_a + (c_a + (d_a > 0)) h_a", "tau < tau_acc + beta_c seg", "2 a + (d_a > 0)", "n_beta != Nv",
                   "absorbs nothing"):
        assert phrase in body, phrase
    assert re.search(r"#define RTHX_ABI_VERSION 5\b", txt)
    assert "rthx_gasbox_trace_field" in abi.EXPORTED_SYMBOLS


def test_voxel_box_fields_and_weights():
    lo, hi, n = np.array([-0.25, 0.5, 0.0]), np.array([0.75, 1.4, 0.5]), (4, 3, 2)
    ref = G.Box(lo, hi, n)
    kap = np.arange(24.0).reshape(n) + 1.0  # [c_x, c_y, c_z]
    box = VoxelGasBox3D(lo, hi, n, kappa=kap, sigma_s=0.5)
    assert box.n_volumes == ref.Nv and box.num_elements == ref.N
    for v in range(ref.Nv):  # element order: c_x fastest
        cx, cy, cz = ref.element(ref.Ns + v)[2]
        assert box.kappa[v] == kap[cx, cy, cz] and box.sigma_s[v] == 0.5
    fb = GF.FieldBox(lo, hi, n, kap + 0.5)
    assert np.array_equal(box.beta, fb.beta_elements())
    # the same field given in element order, and a scalar
    flat = VoxelGasBox3D(lo, hi, n, kappa=box.kappa, sigma_s=np.full(24, 0.5))
    assert np.array_equal(flat.kappa, box.kappa) and np.array_equal(flat.beta, box.beta)
    uni = VoxelGasBox3D(lo, hi, n, kappa=2.0, sigma_s=0.5)
    assert uni.beta.shape == (24,) and np.all(uni.beta == 2.5)
    assert np.array_equal(uni.weights(), GasBox3D(lo, hi, n, kappa=2.0, sigma_s=0.5).weights())
    # weights: wall areas, then max(1e-6, 4 beta_v V)
    w = box.weights()
    assert len(w) == ref.N and np.allclose(w[:ref.Ns], [ref.size(g) for g in range(ref.Ns)], rtol=1e-13)
    assert np.allclose(w[ref.Ns:], 4.0 * fb.beta_elements() * np.prod(ref.h), rtol=1e-13)
    thin = kap * 0.0
    thin[1, 2, 1] = 3.0
    tw = VoxelGasBox3D(lo, hi, n, kappa=thin).weights()[ref.Ns:]
    v = ref.volume_index(1, 2, 1) - ref.Ns
    assert tw[v] == pytest.approx(12.0 * np.prod(ref.h)) and np.all(np.delete(tw, v) == 1e-6)  # get_w's floor
    # refused
    for bad in (np.ones((3, 4, 2)), np.ones(23), np.ones((2, 12)), -kap, np.where(kap == 5.0, np.nan, kap),
                np.where(kap == 5.0, np.inf, kap)):
        with pytest.raises(ValueError):
            VoxelGasBox3D(lo, hi, n, kappa=bad)
        with pytest.raises(ValueError):
            VoxelGasBox3D(lo, hi, n, kappa=1.0, sigma_s=bad)
    with pytest.raises(ValueError):
        GasBox3D(lo, hi, n, kappa=kap)  # the uniform box goes on refusing a field
    # a transparent voxel: legal to hold and to trace, refused by the smoothing and the solve
    with pytest.raises(ValueError, match="beta = 0"):
        VoxelGasBox3D(lo, hi, n, kappa=thin)(1000)


def test_grey_solve_assembly_per_voxel():
    """equilibrium_gasbox with per-voxel kappa and omega on a made-up F: the
    uniform field through VoxelGasBox3D assembles bit for bit what GasBox3D
    assembles, and a heterogeneous field gives size 4 kappa_v V and b =
    sigma_s,v / beta_v -- read back through the system the solver is handed."""
    from rthx import equilibrium as EQ

    lo, hi, n = (0, 0, 0), (1, 1, 1), (2, 1, 2)
    seen = []

    def fake_solve(F, coeff, h, device, info, handle=None):
        seen.append((np.array(coeff), np.array(h)))
        info.update(iterations=0, cycles=0, residual=0.0, tolerance=0.0, converged=True)
        return np.array(h), np.array(h)

    real = EQ._solve
    EQ._solve = fake_solve
    try:
        kw = dict(epsilon=0.7, T_in_w=1000.0, T_in_g=[-1.0, 500.0, -1.0, 800.0], q_in_g=[3.0, 0.0, 0.0, 0.0])
        a = GasBox3D(lo, hi, n, kappa=1.5, sigma_s=0.5, **kw)
        b = VoxelGasBox3D(lo, hi, n, kappa=1.5, sigma_s=0.5, **kw)
        F = np.eye(a.num_elements)
        ra = EQ.equilibrium_gasbox(a, F=F)
        rb = EQ.equilibrium_gasbox(b, F=F)
        for x, y in zip(seen[0] + ra, seen[1] + rb):
            assert np.array_equal(x, y)
        kap, sig = np.array([1.0, 0.0, 2.0, 4.0]), np.array([1.0, 0.5, 0.0, 4.0])
        c = VoxelGasBox3D(lo, hi, n, kappa=kap, sigma_s=sig, **kw)
        EQ.equilibrium_gasbox(c, F=F)
    finally:
        EQ._solve = real
    coeff, h = seen[2]
    ns = c.n_surfaces
    assert np.allclose(coeff[:ns], 0.3)
    assert np.array_equal(coeff[ns:], [1.0, 1.0, 1.0, 0.5])  # (q known: 1; T known: omega_v = sigma_s / beta)
    sb = EQ.STEFAN_BOLTZMANN
    V = c.volume()
    assert h[ns + 0] == 3.0 and h[ns + 2] == 0.0
    assert h[ns + 1] == pytest.approx(4.0 * 0.0 * V * sb * 500.0 ** 4) and h[ns + 3] == pytest.approx(4.0 * 4.0 * V * sb * 800.0 ** 4)


def test_thin_heterogeneous_gas_needs_the_orthogonal_projection():
    """tests/test_gasbox_host.py's thin-gas case with kappa differing fourfold
    between neighbouring voxels: the delta-tracking restatement's counts (1e5
    rays a row), weights 4 kappa_v V, smoothed by the smoothing oracle.  One
    Dykstra round puts every voxel's (T_g / T)^4 inside 5 sigma + 2e-3; the
    alternating projection alone misses it several-fold."""
    from oracle import smooth_oracle as SO

    fb = GF.FieldBox([0, 0, 0], [1, 1, 1], (3, 3, 3), GF.thin_field())
    R = 100_000
    F = fb.trace(range(fb.N), R, seed=1) / R
    V = fb.size(fb.Ns)
    w = np.concatenate([[fb.size(g) for g in range(fb.Ns)], np.maximum(1e-6, 4 * fb.beta_elements() * V)])
    q, tol = GF.thin_reference(fb, R)
    hot = slice(fb.face_offset[4], fb.face_offset[5])
    worst = {}
    for k in (0, 1):
        Fs = np.asarray(SO.smooth_F(F, w, fb.Ns, k_dykstra=k))
        got = (w[hot, None] * Fs[hot, fb.Ns:]).sum(axis=0) / w[fb.Ns:]
        worst[k] = float((np.abs(got - q) / tol).max())
    print(f"worst deviation / tolerance: alternating projection alone {worst[0]:.2f}, one Dykstra round {worst[1]:.2f}")
    assert worst[1] <= 1.0 < worst[0]
