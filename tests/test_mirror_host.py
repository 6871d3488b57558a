"""Specular symmetry walls without a GPU: the geometry flag
(``PolyVolume2D(mirror_walls=...)`` -> ``mirrorWalls``), its flattening
(``FlatDomain.coarse_mirror``) and the argument checks of
rthx_domain_set_mirror_walls / rthx_domain_get_mirror_walls that come before
any device call.  The traces are tests/test_gpu_mirror.py.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers as H
from rthx import PolyVolume2D, RayTracingDomain2D, abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytraceheattransfer.jl_amd", "csrc")

SQUARE = [(0.0, 0.0), (0.5, 0.0), (0.5, 1.0), (0.0, 1.0)]
TRIANGLE = [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0)]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-s", "-C", CSRC], check=True)
    return _lib.load()


def test_mirror_walls_default_to_none():
    quad = PolyVolume2D(SQUARE, [True] * 4, 1, 1.0, 0.0)
    tri = PolyVolume2D(TRIANGLE, [True, False, True])
    assert quad.mirrorWalls == [False] * 4 and tri.mirrorWalls == [False] * 3
    assert H.square_face().mirrorWalls == [False] * 4
    flat = H.square_domain(3).flat()
    assert flat.coarse_mirror.dtype == np.uint8 and flat.coarse_mirror.shape == (1, 4) and not flat.coarse_mirror.any()


def test_mirror_walls_attribute_and_length():
    f = PolyVolume2D(SQUARE, [True, False, True, True], 1, 1.0, 0.0, mirror_walls=[False, True, False, False])
    assert f.mirrorWalls == [False, True, False, False] and f.solidWalls == [True, False, True, True]
    f = PolyVolume2D(SQUARE, [True, False, True, True], mirror_walls=(0, 1, 0, 0))
    assert f.mirrorWalls == [False, True, False, False]
    with pytest.raises(ValueError, match="one entry per wall"):
        PolyVolume2D(SQUARE, [True, False, True, True], mirror_walls=[False, True, False])
    with pytest.raises(ValueError, match="one entry per wall"):
        PolyVolume2D(TRIANGLE, [True, False, True], mirror_walls=[False, True, False, False])


@pytest.mark.parametrize("verts,solid,mirror", [
    (SQUARE, [True, True, True, True], [False, True, False, False]),
    (SQUARE, [False, False, False, True], [False, False, True, True]),
    (TRIANGLE, [True, False, True], [True, True, False]),
])
def test_solid_and_mirror_is_refused(verts, solid, mirror):
    with pytest.raises(ValueError, match="both solid and a mirror"):
        PolyVolume2D(verts, solid, 1, 1.0, 0.0, mirror_walls=mirror)


def test_sub_volumes_do_not_inherit_the_flag():
    f = PolyVolume2D(SQUARE, [True, False, True, True], 1, 1.0, 0.0, mirror_walls=[False, True, False, False])
    dom = RayTracingDomain2D([f], [(3, 4)])
    assert all(sub.mirrorWalls == [False] * 4 for sub in dom.fine_mesh[0])
    # a mirror wall is no surface: bottom 3 + top 3 + left 4 wall elements, none on the right
    assert dom.num_surfaces == 3 + 3 + 4 and dom.num_volumes == 12


def test_coarse_mirror_content_and_padding():
    quad = PolyVolume2D(SQUARE, [True, False, True, True], 1, 1.0, 0.0, mirror_walls=[False, True, False, False])
    quad2 = PolyVolume2D([(0.5, 0.0), (1.0, 0.0), (1.0, 1.0), (0.5, 1.0)], [True, True, True, False], 1, 1.0, 0.0)
    flat = RayTracingDomain2D([quad, quad2], [(2, 2), (2, 2)]).flat()
    assert flat.coarse_mirror.dtype == np.uint8 and flat.coarse_mirror.flags["C_CONTIGUOUS"]
    assert flat.coarse_mirror.tolist() == [[0, 1, 0, 0], [0, 0, 0, 0]]
    # a triangle face (ndim 3): three flags and a zero in the padding slot, like coarse_solid
    tri = PolyVolume2D(TRIANGLE, [True, True, False], 1, 1.0, 0.0, mirror_walls=[False, False, True])
    flat = RayTracingDomain2D([tri], [(3, 3)]).flat()
    assert flat.coarse_nv.tolist() == [3]
    assert flat.coarse_mirror.tolist() == [[0, 0, 1, 0]]
    assert flat.coarse_solid.reshape(-1, 4).tolist() == [[1, 1, 0, 0]]


def test_setter_and_getter_refuse_null_without_a_device(lib):
    assert lib.rthx_abi_version() == 5
    mask = np.zeros(4, dtype=np.uint8)
    assert lib.rthx_domain_set_mirror_walls(None, abi.ptr(mask, C.c_uint8)) == abi.RTHX_EINVAL
    assert b"null domain" in lib.rthx_last_error()
    assert lib.rthx_domain_set_mirror_walls(None, None) == abi.RTHX_EINVAL
    n = C.c_int64(-7)
    assert lib.rthx_domain_get_mirror_walls(None, C.byref(n)) == abi.RTHX_EINVAL
    assert n.value == -7
    assert b"null" in lib.rthx_last_error()


def test_symbols_declared_and_exported(lib):
    for s in ("rthx_domain_set_mirror_walls", "rthx_domain_get_mirror_walls"):
        assert s in abi.EXPORTED_SYMBOLS
        getattr(lib, s)
    hdr = open(os.path.join(ROOT, "include", "rthx.h")).read()
    assert "int rthx_domain_set_mirror_walls(rthx_domain* dom, const uint8_t* mirror);" in hdr
    assert "int rthx_domain_get_mirror_walls(const rthx_domain* dom, int64_t* n_mirror);" in hdr
    assert "#define RTHX_ABI_VERSION 5 " in hdr


def test_several_devices_refuse_a_mirror_domain():
    """rthx_multi has no mirror setter: the Python wrapper raises before it
    uploads anything."""
    f = PolyVolume2D(SQUARE, [True, False, True, True], 1, 1.0, 0.0, mirror_walls=[False, True, False, False])
    flat = RayTracingDomain2D([f], [(2, 2)]).flat()
    with pytest.raises(_lib.RthxError, match="mirror walls"):
        _lib.MultiDeviceDomain(flat, [0, 1])
