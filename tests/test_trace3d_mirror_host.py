"""Specular symmetry planes of the 3D tracer without a GPU:
the scene builders and fold maps the GPU tests rely on, the argument checks of
``Scene3D`` / ``ViewFactorDomain3D`` and of rthx_scene3d_create_mirrored that
come before any device call, and the two symbols' presence.  The traces are
tests/test_gpu_trace3d_mirror.py.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import mirror3d_scenes as M
from oracle import oracle
from rthx import abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytraceheattransfer.jl_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-s", "-C", CSRC], check=True)
    return _lib.load()


@pytest.mark.parametrize("axes,n_part,n_cube,n_box", [((0,), 60, 48, 12), ((0, 1, 2), 15, 12, 3)],
                         ids=["half", "octant"])
def test_boxed_scene_and_fold_maps(axes, n_part, n_cube, n_box):
    sc = M.boxed(axes)
    xyz, nrm, n = sc["xyz"], sc["normals"], sc["n_part"]
    assert xyz.shape == (120, 4, 3) and n == n_part and np.all(sc["nv"] == 4)
    on_cube = np.array([np.any(np.all(np.isin(q, (0.0, 1.0)), axis=0)) for q in xyz])
    assert on_cube.sum() == 96 and on_cube[:n].sum() == n_cube and (~on_cube[:n]).sum() == n_box
    # the part lies at x_k <= 0.5 on every folded axis, the rest does not
    assert np.all(xyz[:n][:, :, list(axes)] <= 0.5 + 1e-12)
    assert np.all(np.any(xyz[n:].mean(axis=1)[:, list(axes)] > 0.5, axis=1))
    # cube rays leave inward, box rays outward
    cen = xyz.mean(axis=1)
    toward = np.einsum("ij,ij->i", nrm, 0.5 - cen)
    assert np.all(toward[on_cube] > 0) and np.all(toward[~on_cube] < 0)
    # fold: onto the part, every part column the image of 2^len(axes) full columns; identity on the part
    col_of, row_of = sc["col_of"], sc["row_of"]
    assert col_of.min() == 0 and col_of.max() == n - 1
    assert np.all(np.bincount(col_of, minlength=n) == 2 ** len(axes))
    assert np.array_equal(col_of[row_of], np.arange(n))
    # a folded polygon is the mirror image of its part polygon: same plane distance from the centre, same area
    for j in (n, 77, 119):
        f = M.fold_point(xyz[j], axes)
        assert np.allclose(np.sort(f.reshape(-1)), np.sort(xyz[col_of[j]].reshape(-1)), atol=1e-12)
    C_ = np.arange(n * 120).reshape(n, 120)
    B = M.fold_counts(C_, col_of, n)
    assert B.shape == (n, n) and np.array_equal(B.sum(axis=1), C_.sum(axis=1))
    mxyz, mnv = sc["mirrors"]
    assert mxyz.shape == (len(axes), 4, 3) and np.all(mnv == 4)
    for m, k in enumerate(axes):
        assert np.all(mxyz[m][:, k] == 0.5)
        others = np.delete(mxyz[m], k, axis=1)
        assert others.min() == -0.25 and others.max() == 1.25


def test_folded_oracle_is_closed_and_symmetric():
    """The restatement on the full scene loses nothing, and folding keeps
    every ray: what the GPU tests compare against (a short trace)."""
    sc = M.boxed((0,))
    n = sc["n_part"]
    Cf, lost = oracle.trace_exchange_3d(sc["xyz"], sc["nv"], sc["normals"], 500, seed=3, begin=0, end=n, nthreads=4)
    assert lost == 0 and Cf.shape == (n, 120)
    B = M.fold_counts(Cf.astype(np.int64), sc["col_of"], n)
    assert np.all(B.sum(axis=1) == 500)
    # self-return: an x = 0 cube element reaches its image on x = 1, which folds onto itself
    on_x0 = np.flatnonzero(np.all(sc["xyz"][:n, :, 0] == 0.0, axis=1))
    assert len(on_x0) == 16 and np.diag(B)[on_x0].sum() > 0


def test_small_scene_builders():
    xyz, nv, nrm, (mxyz, mnv) = M.octant_cube()
    assert xyz.shape == (3, 4, 3) and len(mnv) == 3
    for k in range(3):
        assert np.all(xyz[k][:, k] == 0.0) and nrm[k][k] == 1.0
    xyz, nv, nrm, (mxyz, mnv) = M.mirror_box()
    assert xyz.shape == (1, 4, 3) and np.all(xyz[0][:, 2] == 0.0) and len(mnv) == 5
    planes = sorted((int(np.flatnonzero(np.ptp(q, axis=0) == 0)[0]), float(q[0][np.ptp(q, axis=0) == 0][0])) for q in mxyz)
    assert planes == [(0, 0.0), (0, 1.0), (1, 0.0), (1, 1.0), (2, 1.0)]
    pts, faces, mirror_faces = M.octant_domain_inputs()
    for k in range(3):
        assert np.all(pts[np.array(faces[k]) - 1][:, k] == 0.0)
        assert np.all(pts[np.array(mirror_faces[k]) - 1][:, k] == 0.5)


def test_scene3d_mirror_arguments_checked_before_the_library():
    from rthx.trace3d import Scene3D, mirror_arrays

    xyz, nv, nrm, (mxyz, mnv) = M.octant_cube()
    mx, mk = mirror_arrays((mxyz, mnv))
    assert mx.shape == (3, 12) and mx.dtype == np.float64 and mk.dtype == np.int32 and mx.flags["C_CONTIGUOUS"]
    mx, mk = mirror_arrays((np.zeros((0, 4, 3)), []))
    assert mx.shape == (0, 12) and len(mk) == 0
    with pytest.raises(ValueError, match="pair"):
        Scene3D(xyz, nv, nrm, mirrors=mxyz)
    with pytest.raises(ValueError, match="need 36"):
        Scene3D(xyz, nv, nrm, mirrors=(mxyz[:2], mnv))
    with pytest.raises(ValueError, match="3 or 4 vertices"):
        Scene3D(xyz, nv, nrm, mirrors=(mxyz, [4, 5, 4]))


def test_view_factor_domain_mirror_faces_without_a_device():
    from rthx.domain3d import ViewFactorDomain3D

    pts, faces, mirror_faces = M.octant_domain_inputs()
    args = (2, [0.0] * 3, [1000.0, 0.0, 0.0], [1.0] * 3)
    dom = ViewFactorDomain3D(pts, faces, *args, mirror_faces=mirror_faces)
    # not meshed, no elements
    assert dom.num_elements == 12 and len(dom.facesMesh) == 3
    mxyz, mnv = dom.mirror_arrays()
    assert mxyz.shape == (3, 4, 3) and np.all(mnv == 4)
    for k in range(3):
        assert np.all(mxyz[k][:, k] == 0.5)
    with pytest.raises(ValueError, match="montecarlo"):
        dom(method="analytic")
    plain = ViewFactorDomain3D(pts, faces, *args)
    assert plain.mirror_faces == [] and plain.mirror_arrays() is None
    with pytest.raises(ValueError, match="3 or 4"):
        ViewFactorDomain3D(pts, faces, *args, mirror_faces=[[1, 2]])
    with pytest.raises(ValueError, match="out of range"):
        ViewFactorDomain3D(pts, faces, *args, mirror_faces=[[1, 2, 3, 9]])
    with pytest.raises(ValueError, match="out of range"):
        ViewFactorDomain3D(pts, faces, *args, mirror_faces=[[0, 1, 2, 3]])
    # a triangular mirror face keeps its three vertices
    tri = ViewFactorDomain3D(pts, faces, *args, mirror_faces=[[2, 4, 8]])
    mxyz, mnv = tri.mirror_arrays()
    assert mnv.tolist() == [3] and np.array_equal(mxyz[0, :3], pts[[1, 3, 7]])


def _create(lib, xyz, nv, nrm, mxyz, mnv, n_mirror):
    h = C.c_void_p()
    x = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 12)
    k = np.ascontiguousarray(nv, dtype=np.int32)
    nr = np.ascontiguousarray(nrm, dtype=np.float64)
    mx = None if mxyz is None else np.ascontiguousarray(mxyz, dtype=np.float64).reshape(-1, 12)
    mk = None if mnv is None else np.ascontiguousarray(mnv, dtype=np.int32)
    rc = lib.rthx_scene3d_create_mirrored(abi.ptr(x, C.c_double), abi.ptr(k, C.c_int32), abi.ptr(nr, C.c_double), None,
                                          len(k), None if mx is None else abi.ptr(mx, C.c_double),
                                          None if mk is None else abi.ptr(mk, C.c_int32), n_mirror, 0, C.byref(h))
    return rc, h, lib.rthx_last_error().decode()


def test_bad_mirror_input_is_refused_before_any_device_call(lib):
    xyz, nv, nrm, (mxyz, mnv) = M.octant_cube()
    bent = mxyz.copy()
    bent[0, 3, 0] += 0.1
    inf = mxyz.copy()
    inf[2, 0, 2] = np.inf
    for what, (mx, mk, nm) in {
        "nv 5": (mxyz, [4, 5, 4], 3), "nv 0": (mxyz, [4, 4, 0], 3), "non-planar": (bent, mnv, 3),
        "non-finite": (inf, mnv, 3), "negative count": (mxyz, mnv, -2), "null xyz": (None, mnv, 3),
        "null nv": (mxyz, None, 3),
    }.items():
        rc, h, msg = _create(lib, xyz, nv, nrm, mx, mk, nm)
        assert rc == abi.RTHX_EINVAL and "mirror" in msg and not h.value, (what, rc, msg)
    # the real polygons are checked as in rthx_scene3d_create_grouped: one polygon needs a mirror
    rc, h, msg = _create(lib, xyz[:1], nv[:1], nrm[:1], None, None, 0)
    assert rc == abi.RTHX_EINVAL and "fewer than 2" in msg and not h.value
    n1, n2 = C.c_int64(-7), C.c_int64(-7)
    assert lib.rthx_scene3d_mirrors(None, C.byref(n1), C.byref(n2)) == abi.RTHX_EINVAL
    assert n1.value == -7 and n2.value == -7


def test_symbols_declared_and_exported(lib):
    for s in ("rthx_scene3d_create_mirrored", "rthx_scene3d_mirrors"):
        assert s in abi.EXPORTED_SYMBOLS
        getattr(lib, s)
    hdr = open(os.path.join(ROOT, "include", "rthx.h")).read()
    assert "int rthx_scene3d_mirrors(const rthx_scene3d* scene, int64_t* n_mirror, int64_t* n_mirror_tris);" in hdr
    assert "int rthx_scene3d_create_mirrored(const double* xyz, const int32_t* nv, const double* normal," in hdr
    assert "#define RTHX_ABI_VERSION 5 " in hdr
    jl = open(os.path.join(ROOT, "raytraceheattransfer.jl_amd", "julia", "RTHX.jl")).read()
    assert "ccall((:rthx_scene3d_create_mirrored" in jl
