"""The 3D gas-box tracer's host side (include/rthx.h rthx_gasbox_*, rthx.gasbox;
DESIGN.md §7l), without a GPU: the element layout against the independent
restatement (tests/gasbox_ref.py), the wall quads, every argument check of the
C ABI, the restatement itself against quadrature of the exchange integrals, and
the ray's classification function (csrc/rthx_gasbox.h, the one the kernel
calls) in tests/gasbox_host_check.cpp, built for the host with
AddressSanitizer and UBSan and run."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import gasbox_ref as G
import helpers as H
from rthx import GasBox3D, _lib, abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-s", "-C", os.path.dirname(os.path.dirname(_lib.LIB_PATH))], check=True)
    return _lib.load()


@pytest.mark.parametrize("n", [(4, 3, 2), (1, 1, 1), (1, 5, 2)])
def test_layout_matches_the_restatement(lib, n):
    ref = G.Box([0, 0, 0], [1, 1, 1], n)
    nn = np.array(n, dtype=np.int32)
    ns, nv = C.c_int64(-1), C.c_int64(-1)
    off = np.full(7, -1, dtype=np.int64)
    assert lib.rthx_gasbox_layout(abi.ptr(nn, C.c_int32), C.byref(ns), C.byref(nv), abi.ptr(off, C.c_int64)) == 0
    assert (ns.value, nv.value) == (ref.Ns, ref.Nv)
    assert np.array_equal(off, ref.face_offset)
    assert ns.value == 2 * (n[1] * n[2] + n[0] * n[2] + n[0] * n[1]) and nv.value == n[0] * n[1] * n[2]
    box = GasBox3D([0, 0, 0], [1, 1, 1], n, kappa=1.0)
    lay = box.layout()
    assert lay["n_elements"] == ref.N and np.array_equal(lay["face_offset"], ref.face_offset)
    # outputs are optional
    assert lib.rthx_gasbox_layout(abi.ptr(nn, C.c_int32), None, None, None) == 0


def test_polygons_lie_on_their_faces():
    lo, hi, n = np.array([-0.25, 0.5, 0.0]), np.array([0.75, 1.4, 0.5]), (4, 3, 2)
    box = GasBox3D(lo, hi, n, kappa=2.0, sigma_s=0.5)
    ref = G.Box(lo, hi, n)
    xyz, nv, normals = box.polygon_arrays()
    assert xyz.shape == (ref.Ns, 4, 3) and np.all(nv == 4) and normals.shape == (ref.Ns, 3)
    centre = 0.5 * (lo + hi)
    for g in range(ref.Ns):
        kind, f, _c = ref.element(g)
        a, side = f >> 1, f & 1
        assert kind == "wall"
        assert np.all(xyz[g, :, a] == (hi[a] if side else lo[a]))  # on its face's plane
        blo, bhi = ref.bounds(g)  # ... and exactly its cell of the face
        assert np.allclose(xyz[g].min(axis=0), blo, atol=1e-15) and np.allclose(xyz[g].max(axis=0), bhi, atol=1e-15)
        e1, e2 = xyz[g, 1] - xyz[g, 0], xyz[g, 3] - xyz[g, 0]
        cr = np.cross(e1, e2)
        assert np.linalg.norm(cr) == pytest.approx(ref.size(g), rel=1e-13)  # area h_p h_q
        assert np.allclose(xyz[g, 2] - xyz[g, 0], e1 + e2, atol=1e-15)      # a rectangle, corners in order
        assert np.array_equal(normals[g], ref.inward_normal(f))
        assert normals[g] @ (centre - xyz[g].mean(axis=0)) > 0.0             # inward
        assert cr @ normals[g] > 0.0                                        # counter-clockwise about it
    assert box.areas() == pytest.approx([ref.size(g) for g in range(ref.Ns)], rel=1e-13)
    w = box.weights()
    assert len(w) == ref.N and np.allclose(w[:ref.Ns], box.areas())
    assert np.allclose(w[ref.Ns:], 4.0 * 2.5 * np.prod(ref.h))
    thin = GasBox3D(lo, hi, n, kappa=1e-9)  # get_w's floor
    assert np.all(thin.weights()[ref.Ns:] == 1e-6)


def test_properties_broadcast():
    box = GasBox3D([0, 0, 0], [1, 1, 1], (2, 3, 4), kappa=1.0, epsilon=[0.1, 0.2, 0.3, 0.4, 0.5, 0.6], T_in_w=300.0,
                   T_in_g=np.arange(24.0))
    ref = G.Box([0, 0, 0], [1, 1, 1], (2, 3, 4))
    for g in range(ref.Ns):
        assert box.epsilon[g] == pytest.approx(0.1 * (ref.element(g)[1] + 1))
    assert np.all(box.T_in_w == 300.0) and np.array_equal(box.T_in_g, np.arange(24.0))
    with pytest.raises(ValueError):
        GasBox3D([0, 0, 0], [1, 1, 1], (2, 3, 4), kappa=1.0, epsilon=[0.5] * 5)
    with pytest.raises(ValueError):
        GasBox3D([0, 0, 0], [1, 1, 1], (2, 3, 4), kappa=[1.0] * 24)  # per-voxel kappa: out of scope
    with pytest.raises(_lib.RthxError):
        GasBox3D([0, 0, 0], [1, 1, 1], (2, 0, 4), kappa=1.0)


def _create(lib, lo, hi, n, out=True):
    h = C.c_void_p()
    a = [None if v is None else np.ascontiguousarray(v, dtype=t) for v, t in ((lo, np.float64), (hi, np.float64), (n, np.int32))]
    rc = lib.rthx_gasbox_create(abi.ptr(a[0], C.c_double), abi.ptr(a[1], C.c_double), abi.ptr(a[2], C.c_int32), 0,
                                C.byref(h) if out else None)
    if rc == 0:
        lib.rthx_gasbox_destroy(h)
    return rc, lib.rthx_last_error().decode()


def test_validation_without_gpu(lib):
    """Every argument error is reported before the first device call: on a
    machine without a GPU a valid call fails with RTHX_EDEVICE, an invalid one
    with its own code."""
    lo, hi, n = [0.0, 0.0, 0.0], [1.0, 2.0, 3.0], [2, 2, 2]
    ok_rc, _ = _create(lib, lo, hi, n)
    assert ok_rc in (0, abi.RTHX_EDEVICE)
    EINVAL, ERANGE = abi.RTHX_EINVAL, abi.RTHX_ERANGE
    assert _create(lib, lo, hi, n, out=False)[0] == EINVAL
    assert _create(lib, None, hi, n)[0] == EINVAL
    assert _create(lib, lo, None, n)[0] == EINVAL
    assert _create(lib, lo, hi, None)[0] == EINVAL
    for bad_n in ([0, 2, 2], [2, -1, 2], [2, 2, 0]):
        rc, msg = _create(lib, lo, hi, bad_n)
        assert rc == EINVAL and ">= 1" in msg
    for bad_hi in ([0.0, 2.0, 3.0], [1.0, -2.0, 3.0], [1.0, 2.0, 0.0]):
        rc, msg = _create(lib, lo, bad_hi, n)
        assert rc == EINVAL and "above lo" in msg
    for bad in (np.nan, np.inf, -np.inf):
        assert _create(lib, [bad, 0.0, 0.0], hi, n) == (EINVAL, "non-finite box corner")
        assert _create(lib, lo, [1.0, bad, 3.0], n)[0] == EINVAL
    assert _create(lib, [-1e308] * 3, [1e308] * 3, n)[0] == EINVAL  # (the extent overflows)
    rc, msg = _create(lib, lo, hi, [2048, 1024, 1024])  # Nv = 2^31
    assert rc == ERANGE and "2^31" in msg
    assert _create(lib, lo, hi, [1290, 1290, 1290])[0] == ERANGE  # Nv < 2^31 <= N
    assert _create(lib, lo, hi, [2 ** 31 - 1] * 3)[0] == ERANGE
    # layout
    nn = np.array([1, 0, 1], dtype=np.int32)
    assert lib.rthx_gasbox_layout(abi.ptr(nn, C.c_int32), None, None, None) == EINVAL
    assert lib.rthx_gasbox_layout(None, None, None, None) == EINVAL
    # trace: the checks of the arguments come before the handles are touched
    r = C.c_void_p()
    assert lib.rthx_result_create(C.byref(r)) == 0

    def trace(args, beta=1.0, ray_begin=0, box=None, res=r):
        rc = lib.rthx_gasbox_trace(box, None if args is None else C.byref(args), beta, ray_begin, res)
        return rc, lib.rthx_last_error().decode()

    good, _ = _lib.make_args(0, 100, 0.0, 1, 0, 8)
    assert trace(None)[0] == EINVAL
    rc, msg = trace(good)  # everything but the box is fine
    assert rc == EINVAL and "null box" in msg
    for beta in (-1.0, -1e-300, np.nan, np.inf):
        rc, msg = trace(good, beta=beta)
        assert rc == EINVAL and "beta" in msg
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


def test_header_documents_the_contract():
    txt = open(os.path.join(ROOT, "include", "rthx.h")).read()
    body = txt[txt.index("typedef struct rthx_gasbox rthx_gasbox;") - 3000:]
    for phrase in ("f = 2 axis + side", "face_offset[f] + c_p + n_p c_q", "Ns + c_x + n_x (c_y + n_y c_z)",
                   "lost_total is always 0", "emitter ranges"):
        assert phrase in body, phrase
    assert re.search(r"#define RTHX_ABI_VERSION 5\b", txt)


@pytest.fixture(scope="module")
def reference_rows():
    """2e6 rays from one voxel and one wall cell of the 3 x 3 x 3 unit cube at
    beta = 1.5, traced once by the numpy restatement."""
    box = G.Box([0, 0, 0], [1, 1, 1], (3, 3, 3))
    rows = [box.volume_index(0, 0, 0), box.wall_index(4, 0, 0)]
    R = 2_000_000
    return box, rows, R, box.trace(rows, R, 1.5, seed=20260)


def test_reference_matches_quadrature(reference_rows):
    """The restatement's four kinds of pair against Gauss-Legendre quadrature
    (8 points a dimension), every column at least one cell away: 5 sigma
    (binomial)."""
    box, rows, R, counts = reference_rows
    kinds = set()
    worst = 0.0
    for k, i in enumerate(rows):
        assert counts[k].sum() == R
        for j in range(box.N):
            if not box.separated(i, j):
                continue
            q = box.pair_integral(i, j, 1.5)
            if q == 0.0:  # (coplanar wall cells never see each other)
                assert counts[k, j] == 0, (i, j)
                continue
            z =(counts[k, j] / R - q) / np.sqrt(q * (1.0 - q) / R)
            worst = max(worst, abs(z))
            kinds.add((box.element(i)[0], box.element(j)[0]))
            assert abs(z) <= 5.0, (i, j, counts[k, j] / R, q, z)
    print(f"worst |z| {worst:.2f} over the separated pairs")
    assert kinds == {("vol", "vol"), ("vol", "wall"), ("wall", "vol"), ("wall", "wall")}


def test_quadrature_reciprocity_and_closure():
    """The integrals themselves: A_i F_ij = 4 beta V_j F_ji between a wall cell
    and a voxel, w_i F_ij = w_j F_ji within a kind, and a voxel's factors to
    the six faces (touching ones included) leave the gas's own share,
    1 - sum = the voxel's self- and gas-absorption, small in a thin medium."""
    box = G.Box([0, 0, 0], [1, 0.9, 0.5], (4, 3, 2))
    beta = 2.0
    v, w_ = box.volume_index(0, 0, 0), box.wall_index(1, 2, 1)
    assert box.size(w_) * box.pair_integral(w_, v, beta) == pytest.approx(
        4 * beta * box.size(v) * box.pair_integral(v, w_, beta), rel=1e-12)
    v2 = box.volume_index(3, 2, 1)
    assert box.pair_integral(v, v2, beta) == pytest.approx(box.pair_integral(v2, v, beta), rel=1e-12)
    cube = G.Box([0, 0, 0], [1, 1, 1], (3, 3, 3))
    for c in ((0, 0, 0), (1, 1, 0), (1, 1, 1)):
        s = sum(cube.volume_to_face(cube.volume_index(*c), f, 1e-3) for f in range(6))
        assert 1.0 - 1.8e-3 <= s < 1.0, (c, s)


def test_thin_gas_needs_the_orthogonal_projection():
    """Why GasBox3D smooths with one Dykstra round.  The optically thin case of
    tests/test_gpu_gasbox.py on the CPU: the numpy restatement's counts (3 x 3
    x 3 unit cube, kappa = 1e-3, 1e5 rays a row), smoothed by the smoothing
    oracle, and (T_g / T)^4 = sum over the hot face of A_i F_iv / (4 kappa V)
    against the quadrature value of F(voxel -> face), tolerance 5 sigma + 2e-3.
    With smooth_F's automatic choice (chi = 0.33 < 0.4: alternating projection
    alone, from the equal-weight mean of the two directions) the few wall rays
    absorbed in the gas put the worst voxel several tolerances out; with one
    round of the orthogonal projection, which weights a pair by w_j^2 : w_i^2,
    every voxel is inside."""
    from oracle import smooth_oracle as SO

    ref = G.Box([0, 0, 0], [1, 1, 1], (3, 3, 3))
    kappa, R = 1e-3, 100_000
    F = ref.trace(range(ref.N), R, kappa, seed=1) / R
    w = np.array([ref.size(g) for g in range(ref.Ns)] + [max(1e-6, 4 * kappa * ref.size(ref.Ns))] * ref.Nv)
    q = np.array([ref.volume_to_face(ref.Ns + v, 4, kappa) for v in range(ref.Nv)])
    tol = 5.0 * np.sqrt(q * (1.0 - q) / R) + 2e-3
    hot = slice(ref.face_offset[4], ref.face_offset[5])
    assert SO.cross_coupling_chi(F, ref.Ns)[0] < 0.4
    worst = {}
    for k in (0, 1):
        Fs = np.asarray(SO.smooth_F(F, w, ref.Ns, k_dykstra=k))
        got = (w[hot, None] * Fs[hot, ref.Ns:]).sum(axis=0) / w[ref.Ns:]
        worst[k] = float((np.abs(got - q) / tol).max())
    print(f"worst deviation / tolerance: alternating projection alone {worst[0]:.2f}, one Dykstra round {worst[1]:.2f}")
    assert worst[1] <= 1.0 < worst[0]
    # the pair variance of the orthogonal projection over the plain mean's, 4 t (1 - t), t = w_i w_j / (w_i^2 + w_j^2)
    rho = np.logspace(-4, 4, 161)
    op = (rho ** 4 * 1.0 + 1.0 * rho) / (rho ** 2 + 1.0) ** 2  # w_j = 1, w_i = rho: (w_j^4 w_i + w_i^4 w_j) / (w_i^2 + w_j^2)^2
    mean = (rho + 1.0) / 4.0
    t = rho / (rho ** 2 + 1.0)
    assert np.allclose(op / mean, 4 * t * (1 - t), rtol=1e-12) and np.all(op <= mean * (1 + 1e-15))


def test_classification_stays_in_range(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "gasbox_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "raytraceheattransfer.jl_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "gasbox_host_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"gasbox rays (\d+), near a cell boundary (\d+)", out.stdout)
    assert m and int(m.group(1)) == 3_000_000 and int(m.group(2)) < 1e-6 * int(m.group(1)), out.stdout
    assert "gasbox check ok" in out.stdout
    print(out.stdout.strip())
