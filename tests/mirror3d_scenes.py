"""Scenes of the 3D symmetry-plane tests, built without a
device: the "boxed" enclosure (unit cube, faces 4 x 4, around the box
[0.3, 0.7]^3, faces 2 x 2), its parts behind mirrors, and the fold that maps
the full scene onto a part.
"""
import numpy as np

MIRROR_SPAN = (-0.25, 1.25)  # oversized: no seam lies at a mirror's own edge


def _face_quads(lo, hi, n, outward):
    """The six faces of the box [lo, hi]^3, each n x n quads (axis-major, low
    side first); rays leave outward (a body) or inward (an enclosure)."""
    quads, normals = [], []
    t = np.linspace(lo, hi, n + 1)
    for k in range(3):
        u, v = (k + 1) % 3, (k + 2) % 3
        for side, plane in enumerate((lo, hi)):
            out = 1.0 if side else -1.0
            for j in range(n):
                for i in range(n):
                    q = np.zeros((4, 3))
                    q[:, k] = plane
                    q[:, u] = [t[i], t[i + 1], t[i + 1], t[i]]
                    q[:, v] = [t[j], t[j], t[j + 1], t[j + 1]]
                    nrm = np.zeros(3)
                    nrm[k] = out if outward else -out
                    quads.append(q)
                    normals.append(nrm)
    return quads, normals


def boxed_full():
    """The full scene in its natural order: (xyz[120][4][3], normals[120][3])."""
    q1, n1 = _face_quads(0.0, 1.0, 4, outward=False)
    q2, n2 = _face_quads(0.3, 0.7, 2, outward=True)
    return np.array(q1 + q2), np.array(n1 + n2)


def mirror_quads(axes):
    """One oversized mirror quad on x_k = 0.5 per axis k of `axes`:
    (mxyz[m][4][3], mnv[m])."""
    a, b = MIRROR_SPAN
    out = []
    for k in axes:
        u, v = (k + 1) % 3, (k + 2) % 3
        q = np.zeros((4, 3))
        q[:, k] = 0.5
        q[:, u] = [a, b, b, a]
        q[:, v] = [a, a, b, b]
        out.append(q)
    return np.array(out).reshape(-1, 4, 3), np.full(len(out), 4, dtype=np.int32)


def fold_point(c, axes):
    c = np.array(c, dtype=np.float64)
    for k in axes:
        c[..., k] = np.minimum(c[..., k], 1.0 - c[..., k])
    return c


def boxed(axes):
    """The boxed scene ordered for the part behind mirrors on x_k = 0.5, k in
    `axes` ((0,) the half, (0, 1, 2) the octant): the part's polygons (every
    folded coordinate of the centroid <= 0.5) come first, in the full scene's
    order, then the others.  Returns a dict: xyz, nv, normals (full scene, 120
    quads), n_part, mirrors (mxyz, mnv), col_of (full column -> part column by
    folded centroid) and row_of (part row -> the same polygon of the full
    scene)."""
    xyz, nrm = boxed_full()
    cen = xyz.mean(axis=1)
    in_part = np.all(cen[:, list(axes)] <= 0.5, axis=1)
    order = np.concatenate([np.flatnonzero(in_part), np.flatnonzero(~in_part)])
    xyz, nrm, cen = xyz[order], nrm[order], cen[order]
    n_part = int(in_part.sum())
    folded = fold_point(cen, axes)
    col_of = np.full(len(xyz), -1, dtype=np.int64)
    for j in range(len(xyz)):
        # (the same plane too: a cube face and a box face never share a centroid)
        hits = np.flatnonzero(np.all(np.abs(cen[:n_part] - folded[j]) < 1e-9, axis=1))
        assert len(hits) == 1, (j, hits)
        col_of[j] = hits[0]
    row_of = np.arange(n_part)
    return dict(xyz=np.ascontiguousarray(xyz), nv=np.full(len(xyz), 4, dtype=np.int32),
                normals=np.ascontiguousarray(nrm), n_part=n_part, mirrors=mirror_quads(axes), col_of=col_of,
                row_of=row_of)


def fold_counts(C_full_rows, col_of, n_part):
    """Counts of part rows over the full scene's columns, folded onto the
    part's columns."""
    B = np.zeros((C_full_rows.shape[0], n_part), dtype=np.int64)
    for j, cj in enumerate(col_of):
        B[:, cj] += C_full_rows[:, j]
    return B


def octant_cube():
    """The octant of the empty unit cube: three unsplit real quads on x, y,
    z = 0 (rays leave into the octant) and three oversized mirrors:
    (xyz[3][4][3], nv, normals, (mxyz, mnv))."""
    quads, normals = [], []
    for k in range(3):
        u, v = (k + 1) % 3, (k + 2) % 3
        q = np.zeros((4, 3))
        q[:, u] = [0.0, 0.5, 0.5, 0.0]
        q[:, v] = [0.0, 0.0, 0.5, 0.5]
        n = np.zeros(3)
        n[k] = 1.0
        quads.append(q)
        normals.append(n)
    return np.array(quads), np.full(3, 4, dtype=np.int32), np.array(normals), mirror_quads((0, 1, 2))


def mirror_box():
    """One real unit quad on z = 0 (rays leave upward) and five mirrors closing
    the unit cube over it: (xyz[1][4][3], nv, normals, (mxyz, mnv))."""
    q, _ = _face_quads(0.0, 1.0, 1, outward=False)
    real = np.array([q[4]])  # axis 2, low side: z = 0
    mir = np.array([q[i] for i in (0, 1, 2, 3, 5)])
    return real, np.full(1, 4, dtype=np.int32), np.array([[0.0, 0.0, 1.0]]), (mir, np.full(5, 4, dtype=np.int32))


def octant_domain_inputs():
    """ViewFactorDomain3D inputs of the octant cube: (points[8][3], faces,
    mirror_faces), 1-based vertex indices; faces x, y, z = 0, mirrors on 0.5."""
    pts = np.array([[x, y, z] for z in (0.0, 0.5) for y in (0.0, 0.5) for x in (0.0, 0.5)])

    def face(k, val):
        idx = [i for i in range(8) if pts[i, k] == val]
        u, v = (k + 1) % 3, (k + 2) % 3
        c = pts[idx].mean(axis=0)
        idx.sort(key=lambda i: np.arctan2(pts[i, v] - c[v], pts[i, u] - c[u]))
        return [i + 1 for i in idx]

    return pts, [face(k, 0.0) for k in range(3)], [face(k, 0.5) for k in range(3)]
