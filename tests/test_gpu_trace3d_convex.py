"""The 3D tracer's exit-direction map (rthx_scene3d_hull = 3: a convex
enclosure seen from inside, rthx_trace3d.h CvxPlane, Walk::convex_exit)
beyond the unit icosphere: stretched, sheared, far and rescaled spheres,
boxes, prisms, the tetrahedron, the cube map at both ends of its resolution,
row forms and shards, grouped scenes and the product entry.

Every case: the map is on (hull_mode 3) and off under RTHX_T3_NO_CVX=1
(hull_mode 0); all rows equal the plain BVH walk's bit for bit, lost rays
too; sampled rows equal the brute-force CPU restatement's.  Tolerance: exact
equality, as tests/test_gpu_trace3d.py.  tests/test_convex_scenes_host.py
shows for every (scene, R) here that at least 1e5 rays, and 2 % of all, pass
the map's geometric gate, so equality with the walk is not vacuous.
"""
import time

import numpy as np
import pytest

import convex_scenes as S
import helpers as H
from oracle import oracle
from test_gpu_trace3d import gpu_dense

pytestmark = pytest.mark.gpu


def _trace(xyz, nv, nrm, R, seed, faithful=False, groups=None):
    """(counts as CSR matrix, info, stats, seconds to build the scene)."""
    from rthx.trace3d import Scene3D

    t0 = time.perf_counter()
    s = Scene3D(xyz, nv, nrm, groups=groups)
    t_scene = time.perf_counter() - t0
    try:
        st = s.stats()
        rp, cols, cnt, info = s.trace(R, seed=seed, faithful=faithful)
    finally:
        s.close()
    return H.counts_matrix(rp, cols, cnt, len(nv)), info, st, t_scene


def _sample_rows(n, k=5):
    return [int(g) for g in np.unique(np.linspace(0, n - 1, k).astype(int))]


def _map_equals_walk_and_restatement(monkeypatch, scene, R, seed, faithful=False, rows=None, mode=3):
    """The core assertion.  `rows`: the rows compared with the restatement
    (default: up to 5 spread over the scene).  Returns the map's counts."""
    xyz, nv, nrm = scene[:3]
    groups = scene[3] if len(scene) > 3 else None
    n = len(nv)
    monkeypatch.delenv("RTHX_T3_NO_CVX", raising=False)
    D, info, st, t_scene = _trace(xyz, nv, nrm, R, seed, faithful, groups)
    assert st["hull_mode"] == mode, st["hull_mode"]
    monkeypatch.setenv("RTHX_T3_NO_CVX", "1")
    W, winfo, wst, _ = _trace(xyz, nv, nrm, R, seed, faithful, groups)
    monkeypatch.delenv("RTHX_T3_NO_CVX")
    assert wst["hull_mode"] == 0
    assert info["rays_traced"] == n * R and winfo["rays_traced"] == n * R
    bad = (D != W).nnz
    print(f"n {n}, R {R}: {bad} counts differ from the walk, lost {info['lost_total']} / {winfo['lost_total']}, "
          f"scene built in {t_scene:.3f} s")
    assert bad == 0, f"{bad} counts differ from the plain walk"
    assert info["lost_total"] == winfo["lost_total"]
    for g in _sample_rows(n) if rows is None else rows:
        C, _lost = oracle.trace_exchange_3d(xyz, nv, nrm, R, seed=seed, begin=g, end=g + 1, nthreads=16, groups=groups)
        assert np.array_equal(D.getrow(g).toarray()[0], C[0]), f"row {g}"
    return D, info, t_scene


SHAPES = ["ico2_z1.5", "ico2_0.6_1_1.6", "ico2_shear", "ico2_z3", "cube_1", "cube_3", "cube_8_8_1", "box_1_1_4",
          "prism_6", "prism_12", "tetrahedron"]


@pytest.mark.parametrize("name,faithful", [(k, False) for k in SHAPES] + [("ico2_shear", True), ("prism_12", True)])
def test_shapes(hip, monkeypatch, name, faithful):
    """Convex bodies that are no sphere: r_in / r_out down to 1/3, so the arc
    bound sits at kCvxArcMax, most rays walk and the two paths
    interleave within a wave; quads (two coplanar triangles with one t);
    coplanar fans of triangles; the cube map's lowest resolution (the
    tetrahedron, the 6-quad cube).  The scenes of few rows trace R >= 65536
    rays a row: split rows and u32 counters on this path."""
    scene, R = S.case(name)
    _D, info, _t = _map_equals_walk_and_restatement(monkeypatch, scene, R, seed=31, faithful=faithful)
    assert info["lost_total"] == 0


@pytest.mark.parametrize("name", ["ico2_shear_far", "ico2_shear_far_1e-3", "ico2_shear_far_1e3"])
def test_placement_and_scale(hip, monkeypatch, name):
    """The sheared sphere 2300 radii from the origin, and that scene scaled
    by 1e-3 and 1e3 about the origin: the detection tolerances and the
    plane-distance window's absolute part (cvx_tpad) follow the scene scale."""
    scene, R = S.case(name)
    _D, info, _t = _map_equals_walk_and_restatement(monkeypatch, scene, R, seed=32)
    assert info["lost_total"] == 0


def test_resolution_clamped_high(hip, monkeypatch):
    """Icosphere level 4: 5120 triangles, the cube map clamped to 96 cells a
    face edge (reached from 3456 triangles), three restatement rows.
    Building the scene (host: vertex test, BVH and the map's lists, then the
    upload) took 0.34 s on the MI355X's host, the whole test 0.76 s, so the
    level 4 sphere stays (profiles/round25/INDEX.md)."""
    scene, R = S.case("ico4")
    n = len(scene[1])
    _D, info, _t = _map_equals_walk_and_restatement(monkeypatch, scene, R, seed=33, rows=_sample_rows(n, 3))
    assert info["lost_total"] == 0


def test_row_forms_and_shards(hip, monkeypatch):
    """The row-count forms and emitter shards on a convex scene (the sphere
    stretched 1.5 along z): the LDS row histogram (RTHX_T3_GHIST=0) and
    counts straight to the dense rows (=1) agree; a strided shard equals its
    rows of the full trace; a 3-row shard of 200 000 rays a row (rows split
    over workgroups, u16 pairs within each) equals the restatement."""
    from rthx.trace3d import Scene3D

    (xyz, nv, nrm), R = S.case("ico2_z1.5")
    n = len(nv)
    s = Scene3D(xyz, nv, nrm)
    try:
        assert s.stats()["hull_mode"] == 3
    finally:
        s.close()
    monkeypatch.setenv("RTHX_T3_GHIST", "0")
    D0, info0 = gpu_dense(xyz, nv, nrm, R, seed=34)
    monkeypatch.setenv("RTHX_T3_GHIST", "1")
    D1, info1 = gpu_dense(xyz, nv, nrm, R, seed=34)
    monkeypatch.delenv("RTHX_T3_GHIST")
    D, info = gpu_dense(xyz, nv, nrm, R, seed=34)
    assert np.array_equal(D0, D1) and np.array_equal(D0, D)
    assert info0["lost_total"] == info1["lost_total"] == info["lost_total"] == 0
    assert int(D.sum()) == n * R
    Sh, _ = gpu_dense(xyz, nv, nrm, R, seed=34, begin=2, stride=5)
    full = np.zeros_like(D)
    full[2::5] = D[2::5]
    assert np.array_equal(Sh, full)
    stride, R3 = S.SHARD_STRIDE, S.SHARD_R
    D3, info3 = gpu_dense(xyz, nv, nrm, R3, seed=35, begin=0, end=3 * stride, stride=stride)
    assert info3["rays_traced"] == 3 * R3
    C3, lost3 = oracle.trace_exchange_3d(xyz, nv, nrm, R3, seed=35, begin=0, end=3 * stride, stride=stride, nthreads=16)
    assert lost3 == 0 and info3["lost_total"] == 0
    assert np.array_equal(D3[0:3 * stride:stride], C3)
    assert int(D3.sum()) == 3 * R3


def test_coplanar_groups(hip, monkeypatch):
    """A cube turned off the axes, its six faces the groups: no box hull
    (no face lies on the bounding box), so the grouped scene takes the exit
    map.  The emitter's group is its own plane, which the map never tests
    (n . d > 0 there); counts equal the walk's and the restatement's with the
    same groups, and no ray lands on its emitter's face."""
    scene, R = S.case("cube_3_rotated_grouped")
    D, info, _t = _map_equals_walk_and_restatement(monkeypatch, scene, R, seed=36)
    g = scene[3]
    assert info["lost_total"] == 0
    assert np.all(D.toarray()[g[:, None] == g[None, :]] == 0)


@pytest.mark.parametrize("level", [1, 2])
def test_noncoplanar_groups(hip, monkeypatch, level):
    """Groups that are not coplanar (four adjacent icosphere triangles each):
    a ray leaving through another polygon of its emitter's group is lost, in
    the walk (Walk::leaf) and the restatement alike.  The exit map tests no
    group, so such a scene does not take it (rthx_scene3d_create_grouped:
    hull_mode 0), and its counts are the restatement's -- all 80 rows at
    level 1, sampled rows at level 2.  Before that rule the scene took the
    map, which counted 1359 (level 2: 1628) of the 11 642 (13 688) rays the
    others lose: 216 (641) counts differed (profiles/round25/INDEX.md)."""
    scene = S.noncoplanar_grouped_icosphere(level)
    xyz, nv, nrm, g = scene
    n, R = len(nv), 5000
    rows = list(range(n)) if level == 1 else None
    D, info, _t = _map_equals_walk_and_restatement(monkeypatch, scene, R, seed=3, rows=rows, mode=0)
    C, lost = oracle.trace_exchange_3d(xyz, nv, nrm, R, seed=3, nthreads=16, groups=g)
    assert info["lost_total"] == lost and lost > S.NONCOPLANAR_MIN_LOST[level] * n * R
    assert np.array_equal(D.toarray(), C)


def test_product_entry(hip, monkeypatch):
    """ViewFactorDomain3D(...)(method="montecarlo") on the readme's icosphere
    at level 1 with every face meshed 2 x 2: the sub-faces as polygon_arrays()
    and their inwardNormal hand them to the tracer -- coplanar neighbours,
    ungrouped."""
    scene = S.domain_icosphere()
    _D, info, _t = _map_equals_walk_and_restatement(monkeypatch, scene, 5000, seed=37)
    assert info["lost_total"] == 0
