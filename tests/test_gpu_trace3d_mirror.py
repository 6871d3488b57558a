"""Specular symmetry planes in the 3D exchange tracer on the MI355X
(rthx_scene3d_create_mirrored).

The pins:
- the part of a symmetric scene traced behind mirrors on the GPU uses the
  very rays the CPU restatement traces through the full scene (emission
  depends on polygon, ray index and seed only), so the restatement's counts
  folded onto the part equal the GPU's but for rays that end within round-off
  of a cell boundary;
- the same fold with independent seeds, as a two-sample homogeneity statistic
  against ``chi2.isf(1e-7, dof)`` (tests/test_gpu_mirror.py's bound), with the
  mirror left out as the negative control;
- analytic: the octant of the empty cube (F = 0.2 / 0.4), a box of mirrors over
  one quad (every ray comes home);
- exact invariants: no mirror is the grouped scene, an unreachable mirror
  changes nothing, shards / repeats / count forms / row splits agree.
"""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import scipy.stats

import helpers as H
import mirror3d_scenes as M
from oracle import oracle
from rthx import abi

pytestmark = pytest.mark.gpu

R_FOLD = 20_000
P_BOUND = 1e-7


def dense_counts(rp, cols, cnt, n):
    D = np.zeros((len(rp) - 1, n), dtype=np.int64)
    for i in range(len(rp) - 1):
        D[i, cols[rp[i]:rp[i + 1]]] = cnt[rp[i]:rp[i + 1]]
    return D


def gpu_dense(xyz, nv, nrm, R, seed=1, mirrors=None, groups=None, faithful=False, begin=0, end=None, stride=1):
    """(dense counts[n][n], info, stats(), mirrors())."""
    from rthx.trace3d import Scene3D

    s = Scene3D(xyz, nv, nrm, groups=groups, mirrors=mirrors)
    try:
        st, mi = s.stats(), s.mirrors()
        rp, cols, cnt, info = s.trace(R, seed=seed, faithful=faithful, emitter_begin=begin, emitter_end=end,
                                      emitter_stride=stride)
    finally:
        s.close()
    return dense_counts(rp, cols, cnt, len(nv)), info, st, mi  # (the CSR has a row per emitter; untraced rows are empty)


def part_of(sc):
    n = sc["n_part"]
    return sc["xyz"][:n], sc["nv"][:n], sc["normals"][:n]


def homogeneity(A, B, min_bin=40):
    """Sum over rows of the two-sample homogeneity statistic
    X2 = sum_j (sqrt(Nb/Na) a_j - sqrt(Na/Nb) b_j)^2 / (a_j + b_j) (Na, Nb the
    row totals), columns with a_j + b_j < min_bin pooled into one bin; and its
    degrees of freedom, sum over rows of (bins - 1)."""
    x2, dof = 0.0, 0
    for a, b in zip(np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)):
        small = a + b < min_bin
        a = np.append(a[~small], a[small].sum())
        b = np.append(b[~small], b[small].sum())
        keep = a + b > 0
        a, b = a[keep], b[keep]
        na, nb = a.sum(), b.sum()
        if na == 0 or nb == 0:  # (a row without a tallied ray on one side: every bin disagrees)
            x2 += na + nb
            dof += max(len(a) - 1, 0)
            continue
        x2 += float(np.sum((math.sqrt(nb / na) * a - math.sqrt(na / nb) * b) ** 2 / (a + b)))
        dof += len(a) - 1
    return x2, dof


_SCENES = {}


def scene(name):
    if name not in _SCENES:
        sc = M.boxed({"half": (0,), "octant": (0, 1, 2)}[name])
        assert len(sc["nv"]) == 120 and sc["n_part"] == {"half": 60, "octant": 15}[name]
        assert len(sc["mirrors"][1]) == {"half": 1, "octant": 3}[name]
        # the fold composed with the part -> full row map is the identity
        assert np.array_equal(sc["col_of"][sc["row_of"]], np.arange(sc["n_part"]))
        _SCENES[name] = sc
    return _SCENES[name]


_FOLDED = {}


def folded_oracle(name, seed, faithful=False):
    """The restatement's counts of the part's rows in the full scene, folded
    onto the part's columns (computed once per case)."""
    key = (name, seed, faithful)
    if key not in _FOLDED:
        sc = scene(name)
        assert not faithful  # (the restatement has one sampling mode in 3D: see test_same_rays_unfolded)
        Cf, lost = oracle.trace_exchange_3d(sc["xyz"], sc["nv"], sc["normals"], R_FOLD, seed=seed, begin=0,
                                            end=sc["n_part"], nthreads=16)
        assert lost == 0
        B = M.fold_counts(Cf.astype(np.int64), sc["col_of"], sc["n_part"])
        B.setflags(write=False)
        _FOLDED[key] = B
    return _FOLDED[key]


@pytest.mark.parametrize("faithful", [False, True], ids=["optimized", "faithful"])
@pytest.mark.parametrize("name", ["half", "octant"])
def test_same_rays_unfolded(hip, name, faithful):
    """The main pin.  Both sides trace identical rays (groups = None on both;
    each plane reflects a ray at most once), so the folded restatement equals
    the GPU but for rays ending within round-off of a cell boundary, where the
    reflected path rounds differently from the straight one: a geometric chance
    of order 1e-14 per ray.  Bound: 2 * ceil(1e-5 * rays) in sum |A - B| (a
    moved ray counts twice).  A wrong normal, a kept emitter-group skip or a
    missed self-return moves 1e-3 of the rays or more.

    The CPU restatement draws the azimuth with libm in both modes of the 3D
    tracer (the device's faithful mode is libm too, its optimized mode the
    table, an ulp apart): one folded reference serves both."""
    sc = scene(name)
    n = sc["n_part"]
    xyz, nv, nrm = part_of(sc)
    A, info, st, mi = gpu_dense(xyz, nv, nrm, R_FOLD, seed=1, mirrors=sc["mirrors"], faithful=faithful)
    B = folded_oracle(name, 1)
    rays = n * R_FOLD
    mism = int(np.abs(A - B).sum())
    print(f"{name} faithful={faithful}: sum|A - B| = {mism} of {rays} rays, lost {info['lost_total']}, "
          f"diagonal {int(np.trace(A))}")
    assert mi == {"n_mirror": len(sc["mirrors"][1]), "n_mirror_tris": 2 * len(sc["mirrors"][1])}
    assert st["hull_mode"] == 0 and st["n_tri"] == 2 * n + mi["n_mirror_tris"]
    assert info["rays_traced"] == rays
    assert mism <= 2 * math.ceil(1e-5 * rays), mism
    assert info["lost_total"] == 0 and info["lost_max_row"] == 0
    assert np.all(A.sum(axis=1) == R_FOLD)


def test_fold_identity_independent_seeds(hip):
    """GPU seed 1 on the half scene against the restatement's seed 777 on the
    full scene, folded.  Restatement against itself on this fold (CPU): X2
    2486, dof 2469, z +0.25, bound 2852.  Negative control: the half scene
    without its mirror loses the rays a mirror returns (the restatement: 24 %,
    z about +570)."""
    sc = scene("half")
    n = sc["n_part"]
    xyz, nv, nrm = part_of(sc)
    B = folded_oracle("half", 777)
    A, info, _st, _mi = gpu_dense(xyz, nv, nrm, R_FOLD, seed=1, mirrors=sc["mirrors"])
    assert info["lost_total"] == 0 and np.all(A.sum(axis=1) == R_FOLD)
    x2, dof = homogeneity(A, B)
    bound = scipy.stats.chi2.isf(P_BOUND, dof)
    print(f"half fold: X2 {x2:.1f} dof {dof} z {(x2 - dof) / math.sqrt(2 * dof):+.2f} bound {bound:.1f}")
    assert x2 <= bound, (x2, dof, bound)
    Cn, cinfo, _st, cmi = gpu_dense(xyz, nv, nrm, R_FOLD, seed=1)
    assert cmi["n_mirror"] == 0 and cinfo["lost_total"] > 0
    x2c, dofc = homogeneity(Cn, B)
    print(f"half, no mirror: lost {cinfo['lost_total']} of {n * R_FOLD}, X2 {x2c:.1f} dof {dofc} "
          f"z {(x2c - dofc) / math.sqrt(2 * dofc):+.1f}")
    assert x2c > scipy.stats.chi2.isf(P_BOUND, dofc)


def test_self_return(hip):
    """A ray may come back to its own face after a reflection: the diagonal of
    the x = 0 face's elements is the view of their mirror images (the folded
    restatement: about 2 % of R)."""
    sc = scene("half")
    xyz, nv, nrm = part_of(sc)
    A, _info, _st, _mi = gpu_dense(xyz, nv, nrm, R_FOLD, seed=1, mirrors=sc["mirrors"])
    B = folded_oracle("half", 1)
    on_x0 = np.flatnonzero(np.all(np.abs(xyz[:, :, 0]) < 1e-12, axis=1))
    assert len(on_x0) == 16
    d, dref = np.diag(A)[on_x0], np.diag(B)[on_x0]
    print(f"diagonal on x = 0: GPU {d.min()}..{d.max()}, folded restatement {dref.min()}..{dref.max()} of {R_FOLD}")
    assert np.all(d > 0)


def test_analytic_octant(hip):
    """The octant of the empty unit cube: three real quarter faces and three
    mirrors.  By the cube's symmetries each quarter face sees what the whole
    face sees: F = 0.2 to the opposite face (its own image: the diagonal; the
    reference's F_EES) and 0.2 + 0.2 to each of the two others."""
    ref = json.load(open(os.path.join(H.GOLDEN, "reference_3d.json")))
    assert np.max(np.abs(np.array(ref["F_EES"])[~np.eye(6, dtype=bool)] - 0.2)) < 2e-4  # (the cube's face pairs)
    xyz, nv, nrm, mirrors = M.octant_cube()
    R = 1_000_000
    A, info, _st, _mi = gpu_dense(xyz, nv, nrm, R, seed=3, mirrors=mirrors)
    F = np.where(np.eye(3, dtype=bool), 0.2, 0.4)
    z = (A - R * F) / np.sqrt(R * F * (1 - F))
    print(f"octant: counts/R {np.round(A / R, 5).tolist()}, z {np.round(z, 2).tolist()}, lost {info['lost_total']}")
    assert np.all(np.abs(z) <= 5.0), z
    assert info["lost_total"] == 0 and np.all(A.sum(axis=1) == R)


def test_mirror_box(hip):
    """One real quad under five mirrors: every ray comes back to it, but the
    grazing ones that meet the reflection cap first (Lambert rays need about
    2 / cos(theta) bounces)."""
    xyz, nv, nrm, mirrors = M.mirror_box()
    R = 100_000
    A, info, st, mi = gpu_dense(xyz, nv, nrm, R, seed=4, mirrors=mirrors)
    lost = info["lost_total"]
    tallied = int(A.sum())
    print(f"mirror box: tallied {tallied}, lost {lost} of {R}")
    assert mi == {"n_mirror": 5, "n_mirror_tris": 10} and st["n_tri"] == 12
    assert A.shape == (1, 1) and A[0, 0] == tallied
    assert tallied + lost == R and info["lost_max_row"] == lost
    assert lost <= R // 1000


def test_no_mirror_is_the_grouped_scene(hip):
    """n_mirror = 0 through rthx_scene3d_create_mirrored: the scene of
    rthx_scene3d_create_grouped (box hull included) and the restatement's
    counts, bit for bit."""
    xyz, nv, nrm, _nc = H.cube_icosphere_scene(3, 1)
    g = H.cube_icosphere_groups(3, 1)
    none = (np.zeros((0, 4, 3)), np.zeros(0, dtype=np.int32))
    A, ainfo, ast, ami = gpu_dense(xyz, nv, nrm, 4000, seed=5, groups=g, mirrors=none)
    G, ginfo, gst, gmi = gpu_dense(xyz, nv, nrm, 4000, seed=5, groups=g)
    Cc, lost = oracle.trace_exchange_3d(xyz, nv, nrm, 4000, seed=5, nthreads=16, groups=g)
    assert ami == gmi == {"n_mirror": 0, "n_mirror_tris": 0}
    assert ast == gst and ast["hull_mode"] == 2
    assert np.array_equal(A, G) and np.array_equal(A, Cc)
    assert ainfo["lost_total"] == ginfo["lost_total"] == lost


def test_unreachable_mirror_changes_nothing(hip):
    """A mirror outside the cube: the counts of the scene without it (the
    restatement's), by the plain walk -- rthx_scene3d_hull reports 0."""
    xyz, nv, nrm, _nc = H.cube_icosphere_scene(3, 1)
    g = H.cube_icosphere_groups(3, 1)
    far = np.array([[[2.0, 0.0, 0.0], [2.0, 1.0, 0.0], [2.0, 1.0, 1.0], [2.0, 0.0, 1.0]]])
    A, info, st, mi = gpu_dense(xyz, nv, nrm, 4000, seed=5, groups=g, mirrors=(far, np.array([4], dtype=np.int32)))
    Cc, lost = oracle.trace_exchange_3d(xyz, nv, nrm, 4000, seed=5, nthreads=16, groups=g)
    assert mi == {"n_mirror": 1, "n_mirror_tris": 2}
    assert st["hull_mode"] == 0 and not st["hull"]
    assert st["n_tri"] == int(np.sum(np.where(nv == 4, 2, 1))) + 2
    assert np.array_equal(A, Cc) and info["lost_total"] == lost


def test_shards_repeats_and_count_forms_exact(hip, monkeypatch):
    """On the half scene: strided emitter shards concatenated, the same trace
    repeated, and both row-count forms (RTHX_T3_GHIST, read at every call)
    give the same counts, optimized and faithful."""
    sc = scene("half")
    xyz, nv, nrm = part_of(sc)
    for faithful in (False, True):
        A, ainfo, _st, _mi = gpu_dense(xyz, nv, nrm, 3000, seed=6, mirrors=sc["mirrors"], faithful=faithful)
        A2, a2info, _st, _mi = gpu_dense(xyz, nv, nrm, 3000, seed=6, mirrors=sc["mirrors"], faithful=faithful)
        assert np.array_equal(A, A2) and ainfo["lost_total"] == a2info["lost_total"] == 0
        S = np.zeros_like(A)
        for b in range(3):
            Sb, _i, _s, _m = gpu_dense(xyz, nv, nrm, 3000, seed=6, mirrors=sc["mirrors"], faithful=faithful, begin=b,
                                       stride=3)
            assert not Sb[[r for r in range(len(nv)) if r % 3 != b]].any()
            S += Sb
        assert np.array_equal(S, A)
        for form in ("0", "1"):
            monkeypatch.setenv("RTHX_T3_GHIST", form)
            Fm, finfo, _s, _m = gpu_dense(xyz, nv, nrm, 3000, seed=6, mirrors=sc["mirrors"], faithful=faithful)
            assert np.array_equal(Fm, A), form
            assert finfo["lost_total"] == 0
        monkeypatch.delenv("RTHX_T3_GHIST")


def test_split_rows_exact(hip, monkeypatch):
    """R large enough to split a row over workgroups (as
    test_shards_and_split_rows_exact): the counts of the unsplit trace
    (RTHX_T3_SPLIT_TARGET = 1: one workgroup per row) and of a strided shard."""
    sc = scene("half")
    xyz, nv, nrm = part_of(sc)
    R = 50_000
    A, info, _st, _mi = gpu_dense(xyz, nv, nrm, R, seed=7, mirrors=sc["mirrors"])
    assert info["lost_total"] == 0 and np.all(A.sum(axis=1) == R)
    S, _i, _s, _m = gpu_dense(xyz, nv, nrm, R, seed=7, mirrors=sc["mirrors"], begin=2, stride=5)
    full = np.zeros_like(A)
    full[2::5] = A[2::5]
    assert np.array_equal(S, full)
    monkeypatch.setenv("RTHX_T3_SPLIT_TARGET", "1")
    U, _i, _s, _m = gpu_dense(xyz, nv, nrm, R, seed=7, mirrors=sc["mirrors"])
    assert np.array_equal(U, A)


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


def test_errors(hip):
    """Bad mirror input is RTHX_EINVAL, names the mirror input and creates no
    scene; the same real polygons with a good mirror are accepted."""
    lib = hip.load()
    xyz, nv, nrm, (mxyz, mnv) = M.octant_cube()
    bent = mxyz.copy()
    bent[0, 3, 0] += 0.1  # vertex 4 off the plane x = 0.5
    nan = mxyz.copy()
    nan[1, 2, 1] = np.nan
    flat = mxyz.copy()
    flat[2, 1] = flat[2, 0]
    flat[2, 2] = flat[2, 0]
    cases = {
        "nv 5": (mxyz, np.array([4, 5, 4], dtype=np.int32), 3),
        "nv 2": (mxyz, np.array([2, 4, 4], dtype=np.int32), 3),
        "non-planar": (bent, mnv, 3),
        "non-finite": (nan, mnv, 3),
        "zero area": (flat, mnv, 3),
        "negative count": (mxyz, mnv, -1),
        "null xyz": (None, mnv, 3),
        "null nv": (mxyz, None, 3),
    }
    for what, (mx, mk, nm) in cases.items():
        rc, h, msg = _create(lib, xyz, nv, nrm, mx, mk, nm)
        assert rc == abi.RTHX_EINVAL, (what, rc, msg)
        assert "mirror" in msg, (what, msg)
        assert not h.value, what
    rc, h, msg = _create(lib, xyz, nv, nrm, mxyz, mnv, 3)
    assert rc == 0 and h.value, msg
    lib.rthx_scene3d_destroy(h)
    assert lib.rthx_scene3d_mirrors(None, None, None) == abi.RTHX_EINVAL


def test_view_factor_domain_octant(hip):
    """ViewFactorDomain3D of the octant cube (Ndims = 2, the three planes as
    mirror_faces), method="montecarlo": F_raw rows sum to 1, F_smooth is
    reciprocal, and the face-summed block is the 0.2 / 0.4 pattern within
    5 sigma of the raw counts (a face's 4 elements trace 4 R rays; the variance
    of their summed count is at most the binomial's at the mean share)."""
    from rthx.domain3d import ViewFactorDomain3D

    pts, faces, mirror_faces = M.octant_domain_inputs()
    dom = ViewFactorDomain3D(pts, faces, 2, [0.0] * 3, [1000.0, 0.0, 0.0], [1.0] * 3, mirror_faces=mirror_faces)
    assert dom.num_elements == 12 and len(dom.mirror_faces) == 3
    with pytest.raises(ValueError, match="montecarlo"):
        dom(method="analytic")
    rays_tot = 12 * 200_000
    dom(method="montecarlo", rays_tot=rays_tot, seed=9)
    R = dom.last_vf_info["rays_per_emitter"]
    assert R == 200_000
    np.testing.assert_allclose(dom.F_raw.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    area = np.array([s.area for s in dom.subfaces()])
    np.testing.assert_allclose(area, 0.0625, rtol=1e-12)
    W = area[:, None] * dom.F_smooth
    assert np.max(np.abs(W - W.T)) <= 1e-10
    block = (dom.F_raw * R).reshape(3, 4, 3, 4).sum(axis=(1, 3))
    p = np.where(np.eye(3, dtype=bool), 0.2, 0.4)
    z = (block - 4 * R * p) / np.sqrt(4 * R * p * (1 - p))
    print(f"octant domain: face blocks {np.round(block / (4 * R), 5).tolist()}, z {np.round(z, 2).tolist()}")
    assert np.all(np.abs(z) <= 5.0), z
