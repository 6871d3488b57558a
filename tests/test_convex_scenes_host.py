"""The scenes of the exit-direction-map tests (tests/convex_scenes.py,
tests/test_gpu_trace3d_convex.py) checked without a device: each is closed
and oriented, convex by detect_convex_enclosure's own vertex test, and sends
enough rays through the map's geometric gate for "the map equals the walk"
to say something; and the non-coplanar grouping loses enough rays in the CPU
restatement to tell a tracer that skips the emitter's group from one that
does not.
"""
import numpy as np
import pytest

import convex_scenes as S
from oracle import oracle

CLOSURE_R = 400  # rays per emitter of the closure check (brute force on the CPU)


def _scene(name):
    if name == "domain_icosphere":
        return S.domain_icosphere(), 5000
    if name.startswith("noncoplanar"):
        return S.noncoplanar_grouped_icosphere(int(name[-1])), 5000
    return S.case(name)


ALL = list(S.CASES) + ["domain_icosphere", "noncoplanar1", "noncoplanar2"]


@pytest.mark.parametrize("name", ALL)
def test_scene_passes_the_vertex_test(name):
    """rthx_scene3d_build.cpp detect_convex_enclosure: every vertex on or in front
    of every emitting plane within 1e-12 of the scene scale (the largest
    |coordinate| or extent), the centroid more than 1e-6 of it inside, and
    no triangle wider than 1.4 rad from its centre direction to a corner."""
    (xyz, nv, nrm, *_), _R = _scene(name)
    verts = np.unique(np.concatenate([xyz[k, :nv[k]] for k in range(len(nv))]), axis=0)
    scale = max(np.abs(verts).max(), (verts.max(axis=0) - verts.min(axis=0)).max())
    unit = nrm / np.linalg.norm(nrm, axis=1)[:, None]
    h = np.einsum("ik,ik->i", unit, xyz[:, 0])
    assert (verts @ unit.T - h[None, :]).min() >= -1e-12 * scale
    c = verts.mean(axis=0)
    assert (unit @ c - h).min() > 1e-6 * scale
    tris = np.concatenate([xyz[:, [0, 1, 2]], xyz[nv == 4][:, [2, 3, 0]]])
    w = tris - c
    w /= np.linalg.norm(w, axis=2)[:, :, None]
    m = w.sum(axis=1)
    m /= np.linalg.norm(m, axis=1)[:, None]
    assert np.arccos(np.clip(np.einsum("tik,tk->ti", w, m), -1.0, 1.0)).max() < 1.4


@pytest.mark.parametrize("name", [k for k in ALL if k != "ico4" and not k.startswith("noncoplanar")])
def test_scene_is_closed_and_oriented(name):
    """No ray of the brute-force restatement is lost, every row holds all its
    rays, and none lands on its own emitter (or, grouped, its own group)."""
    (xyz, nv, nrm, *g), _R = _scene(name)
    g = g[0] if g else None
    C, lost = oracle.trace_exchange_3d(xyz, nv, nrm, CLOSURE_R, seed=2, nthreads=16, groups=g)
    assert lost == 0
    assert np.all(C.sum(axis=1) == CLOSURE_R)
    same = np.eye(len(nv), dtype=bool) if g is None else g[:, None] == g[None, :]
    assert np.all(C[same] == 0)


def test_level4_icosphere_sampled_rows_closed():
    """The 5120-triangle icosphere: three sampled rows (brute force over all
    rows would take seconds)."""
    (xyz, nv, nrm), _R = S.case("ico4")
    n = len(nv)
    C, lost = oracle.trace_exchange_3d(xyz, nv, nrm, CLOSURE_R, seed=2, begin=0, end=n, stride=n // 3 + 1, nthreads=16)
    assert lost == 0 and np.all(C.sum(axis=1) == CLOSURE_R)


@pytest.mark.parametrize("name", [k for k in ALL if not k.startswith("noncoplanar")])
def test_scene_reaches_the_exit_map(name):
    """The guard (convex_scenes.cvx_take_share, 20 000 rays of its own: a
    standard error of 0.0035 at most): a share of at least MIN_SHARE of the
    rays passes the gate, and n R share >= MIN_TAKEN rays at the R the device
    test traces."""
    (xyz, nv, nrm, *_), R = _scene(name)
    share = S.cvx_take_share(xyz, nv, nrm, 20_000, seed=1)
    assert share >= S.MIN_SHARE, share
    assert len(nv) * R * share >= S.MIN_TAKEN, (share, len(nv) * R * share)


def test_shard_reaches_the_exit_map():
    """The 3-row shard of 200 000 rays a row: the gate restated on rays of
    those three rows only."""
    (xyz, nv, nrm), _R = S.case("ico2_z1.5")
    rows = np.arange(0, 3 * S.SHARD_STRIDE, S.SHARD_STRIDE)
    assert len(rows) == 3 and rows[-1] < len(nv)
    # (the three polygons as a scene of their own would have another centre: keep the scene, draw from the rows)
    share = S.cvx_take_share(xyz, nv, nrm, 20_000, seed=1, rows=rows)
    assert share >= S.MIN_SHARE and 3 * S.SHARD_R * share >= S.MIN_TAKEN, share


@pytest.mark.parametrize("level", [1, 2])
def test_noncoplanar_groups_lose_rays(level):
    """Groups of four adjacent icosphere triangles: more than 1 % of the
    restatement's rays (level 2: 0.5 %, convex_scenes.NONCOPLANAR_MIN_LOST)
    leave through their emitter's group and are lost, so counts that include
    them differ visibly from counts that skip them."""
    xyz, nv, nrm, g = S.noncoplanar_grouped_icosphere(level)
    R = 5000
    C, lost = oracle.trace_exchange_3d(xyz, nv, nrm, R, seed=3, nthreads=16, groups=g)
    assert lost > S.NONCOPLANAR_MIN_LOST[level] * len(nv) * R, lost
    assert int(C.sum()) + lost == len(nv) * R
    assert np.all(C[g[:, None] == g[None, :]] == 0)
