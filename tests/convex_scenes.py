"""Convex enclosures seen from inside, for the tests of the 3D tracer's
exit-direction map (rthx_trace3d.h CvxPlane), built without a
device: affine images of the icosphere, boxes, prisms and the regular
tetrahedron; a numpy restatement of the geometric gate that decides which
rays the map takes (cvx_take_share), so that a test of "the map equals the
walk" can show that the map was used; and the (scene, rays per emitter)
pairs the device tests trace (CASES), shared with the host test that checks
them.

Every builder returns (xyz[n][4][3], nv[n], normals[n][3]) or that plus
groups[n]; normals point into the enclosure, and a triangle's fourth vertex
repeats its third.
"""
import numpy as np

import helpers as H

# rthx_trace3d.h kCvxArcMin, kCvxArcMax: the bounds of the largest half-arc
# the exit map takes
K_CVX_ARC_MIN, K_CVX_ARC_MAX = 0.005, 0.1


def rodrigues(axis=(1.0, 2.0, 3.0), angle=0.5):
    """Rotation by `angle` about `axis` (default: 0.5 rad about (1, 2, 3) / sqrt(14))."""
    k = np.asarray(axis, dtype=np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def vertex_centroid(xyz, nv):
    """Mean of the distinct vertices (detect_convex_enclosure's centre)."""
    v = np.concatenate([xyz[k, :nv[k]] for k in range(len(nv))])
    return np.unique(v, axis=0).mean(axis=0)


def _finish(polys):
    """(xyz, nv, normals) of a list of 3- or 4-vertex polygons of a convex
    body: unit normals of the polygons' planes, turned towards the centroid
    of the distinct vertices."""
    n = len(polys)
    xyz = np.zeros((n, 4, 3))
    nv = np.zeros(n, dtype=np.int32)
    for k, p in enumerate(polys):
        p = np.asarray(p, dtype=np.float64)
        nv[k] = len(p)
        xyz[k, :len(p)] = p
        xyz[k, len(p):] = p[-1]
    c = vertex_centroid(xyz, nv)
    nrm = np.cross(xyz[:, 1] - xyz[:, 0], xyz[:, 2] - xyz[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    flip = np.einsum("ik,ik->i", nrm, c - xyz[:, 0]) < 0
    nrm[flip] = -nrm[flip]
    return np.ascontiguousarray(xyz), nv, np.ascontiguousarray(nrm)


def transformed(scene, M=None, offset=(0.0, 0.0, 0.0), factor=1.0):
    """The scene mapped by x -> factor (M x + offset), its normals recomputed
    (groups, when present, kept)."""
    xyz, nv = scene[0], scene[1]
    M = np.eye(3) if M is None else np.asarray(M, dtype=np.float64)
    polys = [factor * (xyz[k, :nv[k]] @ M.T + np.asarray(offset, dtype=np.float64)) for k in range(len(nv))]
    return _finish(polys) + tuple(scene[3:])


def affine_icosphere(level, M=None, offset=(0.0, 0.0, 0.0)):
    """The unit icosphere about the origin (20 * 4**level triangles) mapped
    by x -> M x + offset: an affine image of a convex polytope, so convex."""
    tris = H.icosphere(level, 1.0, (0.0, 0.0, 0.0))
    return transformed(_finish(list(tris)), M, offset)


def box(L, nd, rotate=False):
    """The box [0, L[0]] x [0, L[1]] x [0, L[2]] with nd[k] quads along its
    edges of axis k: the two faces across axis k hold nd[u] x nd[v] quads
    (u, v the other axes), face-major, so each face is a contiguous coplanar
    group.  `rotate`: turned by rodrigues() about the origin, so that no face
    lies on a plane of the scene's bounding box (a grouped box is then no box
    hull, rthx_scene3d_build.cpp detect_box_hull).  Returns (xyz, nv, normals,
    groups)."""
    lines = [np.linspace(0.0, float(L[k]), int(nd[k]) + 1) for k in range(3)]
    polys, groups = [], []
    for k in range(3):
        u, v = (k + 1) % 3, (k + 2) % 3
        for side in (0, 1):
            for j in range(len(lines[v]) - 1):
                for i in range(len(lines[u]) - 1):
                    q = np.zeros((4, 3))
                    q[:, k] = lines[k][-1] if side else 0.0
                    q[:, u] = [lines[u][i], lines[u][i + 1], lines[u][i + 1], lines[u][i]]
                    q[:, v] = [lines[v][j], lines[v][j], lines[v][j + 1], lines[v][j + 1]]
                    polys.append(q)
                    groups.append(2 * k + side)
    if rotate:
        Rm = rodrigues()
        polys = [q @ Rm.T for q in polys]
    return _finish(polys) + (np.array(groups, dtype=np.int32),)


def prism(m, h, sub):
    """A regular m-gon prism of circumradius 1 and height h along z: each
    side face `sub` quads along the axis (face-major; one group a face), then
    the bottom and the top cap, each a fan of m triangles about its centre
    (one group a cap).  The triangles of a cap are coplanar polygons with
    different ids: rays through their shared edges tie on t.  Returns (xyz,
    nv, normals, groups)."""
    a = 2.0 * np.pi * np.arange(m + 1) / m
    ring = np.stack([np.cos(a), np.sin(a)], axis=1)
    ring[m] = ring[0]
    z = np.linspace(0.0, float(h), sub + 1)
    polys, groups = [], []
    for f in range(m):
        for s in range(sub):
            polys.append(np.array([[*ring[f], z[s]], [*ring[f + 1], z[s]], [*ring[f + 1], z[s + 1]], [*ring[f], z[s + 1]]]))
            groups.append(f)
    for cap, zc in enumerate((0.0, float(h))):
        for f in range(m):
            polys.append(np.array([[0.0, 0.0, zc], [*ring[f], zc], [*ring[f + 1], zc]]))
            groups.append(m + cap)
    return _finish(polys) + (np.array(groups, dtype=np.int32),)


def tetrahedron():
    """The regular tetrahedron on four corners of the cube [-1, 1]^3: 4
    triangles, the fewest a closed scene can have (the cube map at its lowest
    resolution), each 1.23 rad from its centre to its corners as seen from
    the centroid."""
    v = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]])
    return _finish([v[[0, 1, 2]], v[[0, 3, 1]], v[[0, 2, 3]], v[[1, 3, 2]]])


def cvx_take_share(xyz, nv, normals, n_rays, seed, rows=None):
    """Share of a scene's rays whose exit cap is short enough for the exit
    map -- the map's geometric gate (rthx_trace3d.h CvxPlane, Walk::
    convex_exit) restated on rays of this function's own: the polygon drawn
    uniformly (every emitter sends as many rays), a uniform point on it, a
    cosine-law direction, all from numpy's generator.  `rows`: the emitters
    to draw from (an emitter shard), default all.

    c = mean of the distinct vertices, rin = min over polygons of
    n . (c - v0), rout = max |v - c|, arc = clip(sqrt(1 - (rin / rout)^2) / 4,
    kCvxArcMin, kCvxArcMax).  With q = o - c a ray is taken when the unit
    directions of q + t_lo d and q + t_out d have a dot product
    >= cos(2 arc): t_out where the ray leaves the ball of radius rout, t_lo
    its far root with the ball of radius rin clamped at 0 (0 without a root).

    A guard for choosing scenes, not a check of the kernel: it leaves out the
    kernel's test that the ray starts away from its polygon's edges and its
    grazing-exit cut."""
    rng = np.random.default_rng(seed)
    xyz = np.array(xyz, dtype=np.float64)
    n = len(nv)
    xyz[np.asarray(nv) == 3, 3] = xyz[np.asarray(nv) == 3, 2]  # (whatever the caller left in the unused slot)
    c = vertex_centroid(xyz, nv)
    nrm = normals / np.linalg.norm(normals, axis=1)[:, None]
    rin = float(np.min(np.einsum("ik,ik->i", nrm, c - xyz[:, 0])))
    rout = float(max(np.linalg.norm(xyz[k, :nv[k]] - c, axis=1).max() for k in range(n)))
    assert 0.0 < rin <= rout
    arc = float(np.clip(0.25 * np.sqrt(1.0 - (rin / rout) ** 2), K_CVX_ARC_MIN, K_CVX_ARC_MAX))
    p = rng.integers(0, n, n_rays) if rows is None else np.asarray(rows)[rng.integers(0, len(rows), n_rays)]
    # a uniform point: one of the triangles (v0 v1 v2), (v2 v3 v0) by area, uniform in it
    a1 = 0.5 * np.linalg.norm(np.cross(xyz[:, 1] - xyz[:, 0], xyz[:, 2] - xyz[:, 0]), axis=1)
    a2 = 0.5 * np.linalg.norm(np.cross(xyz[:, 3] - xyz[:, 2], xyz[:, 0] - xyz[:, 2]), axis=1)  # (0 for a triangle)
    second = rng.random(n_rays) * (a1 + a2)[p] >= a1[p]
    A = np.where(second[:, None], xyz[p, 2], xyz[p, 0])
    B = np.where(second[:, None], xyz[p, 3], xyz[p, 1])
    Cc = np.where(second[:, None], xyz[p, 0], xyz[p, 2])
    s = np.sqrt(rng.random(n_rays))[:, None]
    w = rng.random(n_rays)[:, None]
    o = (1.0 - s) * A + s * (1.0 - w) * B + s * w * Cc
    t1 = xyz[:, 1] - xyz[:, 0]
    t1 /= np.linalg.norm(t1, axis=1)[:, None]
    t2 = np.cross(nrm, t1)
    u = rng.random(n_rays)
    phi = 2.0 * np.pi * rng.random(n_rays)
    r = np.sqrt(u)
    d = (r * np.cos(phi))[:, None] * t1[p] + (r * np.sin(phi))[:, None] * t2[p] + np.sqrt(1.0 - u)[:, None] * nrm[p]
    q = o - c
    b = np.einsum("ik,ik->i", q, d)
    qq = np.einsum("ik,ik->i", q, q)
    t_out = -b + np.sqrt(np.maximum(b * b - (qq - rout * rout), 0.0))
    din = b * b - (qq - rin * rin)
    t_lo = np.where(din > 0.0, np.maximum(-b + np.sqrt(np.maximum(din, 0.0)), 0.0), 0.0)
    ea = q + t_lo[:, None] * d
    eb = q + t_out[:, None] * d
    cosab = np.einsum("ik,ik->i", ea, eb) / (np.linalg.norm(ea, axis=1) * np.linalg.norm(eb, axis=1))
    return float(np.mean(cosab >= np.cos(2.0 * arc)))


# Guard condition of every scene a device test traces on the exit map:
# at least MIN_SHARE of the rays pass the gate, and MIN_TAKEN rays in all.
MIN_SHARE, MIN_TAKEN = 0.02, 1e5

SHEAR = np.array([[1.0, 0.5, 0.0], [0.0, 1.0, 0.3], [0.0, 0.0, 1.0]])
FAR = (1000.0, -2000.0, 500.0)


def _ungrouped(scene):
    return scene[:3]


# name -> (builder of (xyz, nv, normals[, groups]), rays per emitter).  The
# rays per emitter: the smallest round figure with n R share >= MIN_TAKEN at
# the share cvx_take_share gives.
CASES = {
    "ico2_z1.5": (lambda: affine_icosphere(2, np.diag([1.0, 1.0, 1.5])), 5000),
    "ico2_0.6_1_1.6": (lambda: affine_icosphere(2, np.diag([0.6, 1.0, 1.6])), 10_000),
    "ico2_shear": (lambda: affine_icosphere(2, SHEAR), 4000),
    "ico2_z3": (lambda: affine_icosphere(2, np.diag([1.0, 1.0, 3.0])), 9000),
    "cube_1": (lambda: _ungrouped(box((1, 1, 1), (1, 1, 1))), 200_000),
    "cube_3": (lambda: _ungrouped(box((1, 1, 1), (3, 3, 3))), 20_000),
    "cube_8_8_1": (lambda: _ungrouped(box((1, 1, 1), (8, 8, 1))), 6000),
    "box_1_1_4": (lambda: _ungrouped(box((1, 1, 4), (4, 4, 16))), 10_000),
    "prism_6": (lambda: _ungrouped(prism(6, 1.0, 2)), 120_000),
    "prism_12": (lambda: _ungrouped(prism(12, 2.0, 4)), 7000),
    "tetrahedron": (tetrahedron, 1_000_000),
    # placement and scale: the sheared sphere far from the origin, and that scene shrunk and blown up
    "ico2_shear_far": (lambda: affine_icosphere(2, SHEAR, FAR), 4000),
    "ico2_shear_far_1e-3": (lambda: transformed(affine_icosphere(2, SHEAR, FAR), factor=1e-3), 4000),
    "ico2_shear_far_1e3": (lambda: transformed(affine_icosphere(2, SHEAR, FAR), factor=1e3), 4000),
    # the cube map at its highest resolution (5120 triangles)
    "ico4": (lambda: affine_icosphere(4), 1000),
    # coplanar groups: the six faces of a cube turned off the axes
    "cube_3_rotated_grouped": (lambda: box((1, 1, 1), (3, 3, 3), rotate=True), 20_000),
}


# The split-row shard of "ico2_z1.5": rows 0, 106, 212 at SHARD_R rays a row
# (3 R share >= MIN_TAKEN at the scene's share).
SHARD_STRIDE, SHARD_R = 106, 200_000


def case(name):
    """(scene, rays per emitter) of CASES[name]; the scene a tuple (xyz, nv,
    normals) or (xyz, nv, normals, groups)."""
    build, R = CASES[name]
    return build(), R


# Least share of the rays that noncoplanar_grouped_icosphere(level) must lose
# for its test to tell a tracer that skips the emitter's group from one that
# does not: 1 % at level 1.  At level 2 the four children lie half as steep to
# each other, and fewer rays graze from one into the next: half a percent, of
# 1.6e6 rays, is still 8000 rays spread over 320 rows.
NONCOPLANAR_MIN_LOST = {1: 0.01, 2: 0.005}


def noncoplanar_grouped_icosphere(level):
    """The unit icosphere with groups of four consecutive triangles (the four
    children of one parent triangle: adjacent, not coplanar).  A ray that
    would leave through another triangle of its emitter's group is lost."""
    xyz, nv, nrm = affine_icosphere(level)
    return xyz, nv, nrm, (np.arange(len(nv)) // 4).astype(np.int32)


def domain_icosphere():
    """The product entry's scene: ViewFactorDomain3D on the readme's
    icosphere at level 1, every face meshed 2 x 2 (coplanar sub-faces,
    ungrouped), as method="montecarlo" hands it to the tracer: (xyz, nv,
    inward normals)."""
    from rthx import ViewFactorDomain3D

    pts, faces = H.icosphere_mesh(1)
    n = len(faces)
    dom = ViewFactorDomain3D(pts, faces, 2, np.zeros(n), np.full(n, -1.0), np.ones(n))
    xyz, nv = dom.polygon_arrays()
    normals = np.array([s.inwardNormal for s in dom.subfaces()])
    return xyz, nv, normals
