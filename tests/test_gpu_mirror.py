"""Specular symmetry walls on the GPU (rthx_domain_set_mirror_walls).

The CPU oracle knows no mirrors, so the feature is pinned to

* the oracle's trace of the *unfolded* domain: the half (quarter) domain with a
  mirror samples the distribution of the full symmetric domain with its columns
  folded onto the half.  Two-sample chi-square homogeneity per row, summed over
  the rows, against ``chi2.isf(1e-7, dof)`` -- a bound derived from the
  statistic's distribution, not measured; seeds are fixed, so a run is
  deterministic.  The same statistic on the half domain with the wall left open
  must exceed the bound (the test can fail);
* analytic answers: Hottel's crossed strings folded over the mirror, the slab
  transmission 2 E3(tau) with mirrored ends, reciprocity;
* exact identities: no mirror = the parent's trace = the oracle; ray ranges,
  strided shards and every planner branch a mirror domain reaches, bit for bit.

Counts are compared exactly wherever two GPU traces must agree.
"""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.special
import scipy.stats

import helpers as H
from helpers import dense, homogeneity
from oracle import oracle
from rthx import PolyVolume2D, RayTracingDomain2D, abi

pytestmark = pytest.mark.gpu

R_FOLD = 100_000
P_BOUND = 1e-7


# --------------------------------------------------------------------------
# domains: a symmetric full domain, its half (quarter) with mirrors, and the
# fold that maps a point of the full domain onto the half
# --------------------------------------------------------------------------
def _rot(pts, rotation):
    if rotation == 0.0:
        return list(pts)
    c, s = math.cos(rotation), math.sin(rotation)
    return [((x - 0.5) * c - (y - 0.5) * s + 0.5, (x - 0.5) * s + (y - 0.5) * c + 0.5) for x, y in pts]


def part_square(nx, ny, kappa=1.0, rotation=0.0, quarter=False, mirror=True, T_walls=(1000.0, 0.0, 0.0, 0.0)):
    """The left half [0, 0.5] x [0, 1] of helpers.square_face (or its lower
    left quarter), rotated with it about (0.5, 0.5); the cut walls are mirrors
    (or, mirror=False, open walls that lose the ray)."""
    y1 = 0.5 if quarter else 1.0
    verts = _rot([(0.0, 0.0), (0.5, 0.0), (0.5, y1), (0.0, y1)], rotation)
    cut = [False, True, quarter, False]
    face = PolyVolume2D(verts, [not c for c in cut], 1, kappa, 0.0, mirror_walls=cut if mirror else None)
    face.T_in_w = [T_walls[0], 0.0, 0.0 if quarter else T_walls[2], T_walls[3]]
    face.epsilon = [1.0] * 4
    face.T_in_g = -1.0
    face.q_in_g = 0.0
    return RayTracingDomain2D([face], [(nx, ny)])


def square_fold(rotation=0.0, quarter=False):
    def fold(p):
        c, s = math.cos(-rotation), math.sin(-rotation)
        x, y = (p[0] - 0.5) * c - (p[1] - 0.5) * s + 0.5, (p[0] - 0.5) * s + (p[1] - 0.5) * c + 0.5
        x = min(x, 1.0 - x)
        if quarter:
            y = min(y, 1.0 - y)
        return _rot([(x, y)], rotation)[0]
    return fold


def lattice_domain(half, mirror=True):
    """A 1 x 0.5 rectangle cut into 4 x 2 coarse squares (or its left half, 2 x
    2), each meshed 2 x 3, kappa = 0.5 + 2 min(x_mid, 1 - x_mid) + 0.7 j: a
    multi-polygon, non-uniform medium, symmetric about x = 0.5."""
    ncx = 2 if half else 4
    faces = []
    for j in range(2):
        for i in range(ncx):
            x0, x1, y0, y1 = 0.25 * i, 0.25 * (i + 1), 0.25 * j, 0.25 * (j + 1)
            xm = 0.5 * (x0 + x1)
            cut = half and i == ncx - 1
            solid = [j == 0, i == ncx - 1 and not half, j == 1, i == 0]
            f = PolyVolume2D([(x0, y0), (x1, y0), (x1, y1), (x0, y1)], solid, 1,
                             0.5 + 2.0 * min(xm, 1.0 - xm) + 0.7 * j, 0.0,
                             mirror_walls=[False, cut and mirror, False, False])
            f.T_in_g = -1.0
            faces.append(f)
    return RayTracingDomain2D(faces, [(2, 3)] * len(faces))


def slab_domain(kappas):
    """A 1 x 1 slab between two black plates in len(kappas) coarse layers,
    each meshed 3 x 2, both end walls of every layer mirrors: the infinite
    slab, without an edge."""
    L = len(kappas)
    faces = []
    for j, k in enumerate(kappas):
        y0, y1 = j / L, (j + 1) / L
        f = PolyVolume2D([(0.0, y0), (1.0, y0), (1.0, y1), (0.0, y1)], [j == 0, False, j == L - 1, False], 1,
                         float(k), 0.0, mirror_walls=[False, True, False, True])
        f.epsilon = [1.0] * 4
        f.T_in_g = -1.0
        faces.append(f)
    return RayTracingDomain2D(faces, [(3, 2)] * L)


def triangle_domain(mirror=True):
    """A right triangle (ndim 3), the leg on x = 0 a mirror."""
    f = PolyVolume2D([(0.0, 0.0), (1.0, 0.0), (0.0, 1.0)], [True, True, False], 1, 1.0, 0.0,
                     mirror_walls=[False, False, True] if mirror else None)
    f.T_in_g = -1.0
    return RayTracingDomain2D([f], [(3, 3)])


def match_elements(dom_from, dom_to, fold=lambda p: p):
    """For every element of dom_from the element of dom_to with the same kind
    at fold(its key point) (helpers.element_keys)."""
    kt = H.element_keys(dom_to)
    out = np.full(len(H.element_keys(dom_from)), -1, dtype=np.int64)
    for i, (kind, x, y) in enumerate(H.element_keys(dom_from)):
        fx, fy = fold((x, y))
        hits = [j for j, (k2, x2, y2) in enumerate(kt) if k2 == kind and abs(x2 - fx) < 1e-7 and abs(y2 - fy) < 1e-7]
        assert len(hits) == 1, (i, kind, x, y, hits)
        out[i] = hits[0]
    return out


# --------------------------------------------------------------------------
# traces
# --------------------------------------------------------------------------
def _args(hip, flat, R, seed=1, flags=0, begin=0, end=None, stride=1, rec=None):
    return hip.make_args(0, R, H.NUDGE, seed, begin, flat.n_emitters if end is None else end, stride, flags=flags,
                         record_ids=rec)


def gpu_counts(hip, dom, R, seed=1, ray_begin=0, **kw):
    """(row_ptr, cols, counts, info) of one GPU trace of dom (mirrors set by DeviceDomain)."""
    flat = dom.flat()
    args, _k = _args(hip, flat, R, seed=seed, **kw)
    dd = hip.DeviceDomain(flat, 0)
    res = hip.DeviceResult()
    try:
        assert dd.mirror_walls() == int(flat.coarse_mirror.sum())
        res.trace(dd, args, ray_begin=ray_begin)
        rp, c, v = res.csr()
        return rp.copy(), c.copy(), v.copy(), res.info()
    finally:
        res.close()
        dd.close()


def assert_same_counts(a, b, what=""):
    for k, name in enumerate(("row_ptr", "cols", "counts")):
        assert np.array_equal(a[k], b[k]), f"{what}: {name} differ"
    for k in ("rays_traced", "rows_traced", "nnz", "lost_total", "lost_max_row"):
        assert a[3][k] == b[3][k], (what, k, a[3][k], b[3][k])


FOLD_CASES = {
    # name: (full domain, part domain(mirror), fold, faithful flag)
    "square_k1": (lambda: H.square_domain(8, kappa=1.0), lambda m: part_square(4, 8, 1.0, mirror=m), square_fold(), 0),
    "square_k1_faithful": (lambda: H.square_domain(8, kappa=1.0), lambda m: part_square(4, 8, 1.0, mirror=m),
                           square_fold(), 1),
    "square_k0": (lambda: H.square_domain(8, kappa=0.0), lambda m: part_square(4, 8, 0.0, mirror=m), square_fold(), 0),
    "square_k5": (lambda: H.square_domain(8, kappa=5.0), lambda m: part_square(4, 8, 5.0, mirror=m), square_fold(), 0),
    "square_rotated": (lambda: H.square_domain(8, kappa=1.0, rotation=0.3),
                       lambda m: part_square(4, 8, 1.0, rotation=0.3, mirror=m), square_fold(0.3), 0),
    "quarter": (lambda: H.square_domain(8, kappa=1.0), lambda m: part_square(4, 4, 1.0, quarter=True, mirror=m),
                square_fold(quarter=True), 0),
    "lattice_variable": (lambda: lattice_domain(False), lambda m: lattice_domain(True, m), square_fold(), 0),
}


@pytest.mark.parametrize("case", list(FOLD_CASES))
def test_fold_identity_against_oracle(hip, case):
    """The main pin.  Reference alone (oracle against oracle on these inputs):
    z = (X2 - dof) / sqrt(2 dof) between -1.5 and -0.2, dof 552 to 2224; the
    open-wall control: z from 266 to 7459."""
    make_full, make_part, fold, flags = FOLD_CASES[case]
    full, part = make_full(), make_part(True)
    n = part.flat().n_emitters
    col_of = match_elements(full, part, fold)         # full column -> part column
    row_of = match_elements(part, full)               # part row -> the same element of the full domain
    assert np.array_equal(col_of[row_of], np.arange(n))
    if case == "lattice_variable":
        assert full.flat().uniform_beta[0] < 0 and part.flat().n_coarse == 4 and part.flat().coarse_mirror.sum() == 2

    oargs, _k = _args(hip, full.flat(), R_FOLD, seed=777, flags=flags)
    orp, ocols, ocnt, oinfo, _ = oracle.trace_exchange(full.flat(), oargs, 16)
    Cf = dense(orp, ocols, ocnt, full.flat().n_emitters)[row_of]
    B = np.zeros((n, n))
    for j, cj in enumerate(col_of):
        B[:, cj] += Cf[:, j]

    g = gpu_counts(hip, part, R_FOLD, seed=1, flags=flags)
    A = dense(*g[:3], n)
    # a closed enclosure: nothing lost, every row tallies R
    assert g[3]["lost_total"] == 0 and g[3]["lost_max_row"] == 0
    assert np.all(A.sum(axis=1) == R_FOLD)
    x2, dof = homogeneity(A, B)
    bound = scipy.stats.chi2.isf(P_BOUND, dof)
    print(f"{case}: X2 {x2:.1f} dof {dof} z {(x2 - dof) / math.sqrt(2 * dof):+.2f} bound {bound:.1f}")
    assert x2 <= bound, (x2, dof, bound)

    # negative control: the same wall left open loses the rays a mirror returns
    c = gpu_counts(hip, make_part(False), R_FOLD, seed=1, flags=flags)
    assert c[3]["lost_total"] > 0
    x2c, dofc = homogeneity(dense(*c[:3], n), B)
    print(f"{case} open wall: X2 {x2c:.1f} dof {dofc} z {(x2c - dofc) / math.sqrt(2 * dofc):+.1f}")
    assert x2c > scipy.stats.chi2.isf(P_BOUND, dofc)


# --------------------------------------------------------------------------
# analytic pins
# --------------------------------------------------------------------------
def test_transparent_half_square_is_folded_crossed_strings(hip):
    """kappa = 0: every wall-to-wall count within 5 binomial sigma of R times
    the crossed-strings factor to the target plus the one to its image."""
    R = 100_000
    full, part = H.square_domain(8, kappa=0.0), part_square(4, 8, 0.0)
    ns = part.num_surfaces
    row_of = match_elements(part, full)[:ns]
    col_of = match_elements(full, part, square_fold())[:full.num_surfaces]
    segs = H.surface_segments(full)
    F = np.zeros((ns, ns))
    for i in range(ns):
        for j, cj in enumerate(col_of):
            F[i, cj] += H.crossed_strings(segs[row_of[i]], segs[j])
    assert np.allclose(F.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    pos = F > 0
    assert pos.sum() == 224 and (R * F[pos]).min() >= 50
    g = gpu_counts(hip, part, R, seed=5, end=ns)
    assert g[3]["lost_total"] == 0
    A = dense(*g[:3], part.flat().n_emitters)[:ns]
    assert np.all(A[:, ns:] == 0) and np.all(A.sum(axis=1) == R)
    A = A[:, :ns]
    assert np.all(A[~pos] == 0)
    z = (A[pos] - R * F[pos]) / np.sqrt(R * F[pos] * (1 - F[pos]))
    print(f"crossed strings: max |z| {np.abs(z).max():.2f}, rms {np.sqrt(np.mean(z ** 2)):.3f} over {z.size} entries")
    assert np.abs(z).max() <= 5.0


@pytest.mark.parametrize("kappas", [(0.5, 1.5, 1.0, 2.0), (1.0, 1.0, 1.0, 1.0)], ids=["variable", "uniform"])
def test_mirrored_slab_transmits_2E3(hip, kappas):
    """Plate to plate a cold slab transmits 2 E3(tau), tau = mean(kappa) x 1,
    of every bottom-plate element's rays -- the end elements too."""
    R = 1_000_000
    dom = slab_domain(kappas)
    flat = dom.flat()
    assert (flat.uniform_beta[0] > -0.1) == (len(set(kappas)) == 1) and flat.coarse_mirror.sum() == 8
    L = len(kappas)
    bottom = sorted(dom.surface_mapping[(1, f, 1)] - 1 for f in range(1, 4))
    top = sorted(dom.surface_mapping[(L, f, 3)] - 1 for f in range(4, 7))
    assert bottom == list(range(bottom[0], bottom[0] + 3))
    g = gpu_counts(hip, dom, R, seed=9, begin=bottom[0], end=bottom[-1] + 1)
    assert g[3]["lost_total"] == 0 and g[3]["rows_traced"] == 3
    A = dense(*g[:3], flat.n_emitters)[bottom]
    assert np.all(A.sum(axis=1) == R)
    p = 2.0 * float(scipy.special.expn(3, sum(kappas) / L))
    share = A[:, top].sum(axis=1) / R
    z = (share - p) / math.sqrt(p * (1 - p) / R)
    print(f"slab {kappas}: 2 E3 = {p:.6f}, shares {share}, z {z}")
    assert np.all(np.abs(z) <= 5.0)


@pytest.mark.parametrize("shape", ["half_square", "triangle"])
def test_reciprocity_holds_with_a_mirror(hip, shape):
    """w_i F_ij = w_j F_ji on the part domain (folded oracle matrix here: max
    |z| 3.3, rms 0.99 over 1116 pairs)."""
    R = 100_000
    dom = part_square(4, 8, 1.0) if shape == "half_square" else triangle_domain()
    g = gpu_counts(hip, dom, R, seed=13)
    assert g[3]["lost_total"] == 0
    z = H.reciprocity_z(H.counts_matrix(*g[:3], dom.flat().n_emitters), R, H.reciprocity_weights(dom))
    print(f"{shape}: {z.size} pairs, max |z| {np.abs(z).max():.2f}, rms {np.sqrt(np.mean(z ** 2)):.3f}")
    assert z.size > (100 if shape == "half_square" else 20)
    assert np.abs(z).max() < 5.0


# --------------------------------------------------------------------------
# exact identities
# --------------------------------------------------------------------------
def test_no_mirror_is_the_parent_trace(hip):
    """Never set, set to all zero, and set then cleared: one and the same
    trace, the oracle's; the getter counts the flags."""
    dom = part_square(4, 8, 1.0)
    flat = dom.flat()
    mask = flat.coarse_mirror.copy()
    flat.coarse_mirror[:] = 0  # (DeviceDomain then leaves the domain unset)
    args, _k = _args(hip, flat, 5000, seed=3)
    want = oracle.trace_exchange(flat, args, 16)
    dd = hip.DeviceDomain(flat, 0)
    res = hip.DeviceResult()

    def trace():
        res.trace(dd, args)
        rp, c, v = res.csr()
        return rp.copy(), c.copy(), v.copy(), res.info()

    try:
        assert dd.mirror_walls() == 0
        never = trace()
        dd.set_mirror_walls(np.zeros_like(mask))
        assert dd.mirror_walls() == 0
        zero = trace()
        dd.set_mirror_walls(mask)
        assert dd.mirror_walls() == 1
        mirrored = trace()
        dd.set_mirror_walls(None)
        assert dd.mirror_walls() == 0
        cleared = trace()
    finally:
        res.close()
        dd.close()
    for got, what in ((never, "never set"), (zero, "all zero"), (cleared, "cleared")):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), what
        assert got[3]["lost_total"] == want[3]["lost_total"] > 0
    assert mirrored[3]["lost_total"] == 0 and not np.array_equal(mirrored[2], never[2])


@pytest.mark.parametrize("flagged", [0, 1], ids=["flag_on_left", "flag_on_right"])
def test_flagged_interior_wall_reflects_from_both_sides(hip, flagged):
    """The flag wins over a neighbour: the unit square as two coarse halves
    with the wall between them flagged on one of them only exchanges nothing
    across it, from either side, and loses nothing; unflagged it does."""
    def two_halves(mirror):
        left = PolyVolume2D([(0.0, 0.0), (0.5, 0.0), (0.5, 1.0), (0.0, 1.0)], [True, False, True, True], 1, 1.0, 0.0,
                            mirror_walls=[False, mirror and flagged == 0, False, False])
        right = PolyVolume2D([(0.5, 0.0), (1.0, 0.0), (1.0, 1.0), (0.5, 1.0)], [True, True, True, False], 1, 1.0, 0.0,
                             mirror_walls=[False, False, False, mirror and flagged == 1])
        return RayTracingDomain2D([left, right], [(3, 4), (3, 4)])

    dom = two_halves(True)
    n = dom.flat().n_emitters
    side = np.zeros(n, dtype=np.int64)
    for (c, _f, _w), s in dom.surface_mapping.items():
        side[s - 1] = c
    for (c, _f), v in dom.volume_mapping.items():
        side[dom.num_surfaces + v - 1] = c
    cross = side[:, None] != side[None, :]
    R = 20_000
    g = gpu_counts(hip, dom, R, seed=17)
    A = dense(*g[:3], n)
    assert dom.flat().coarse_mirror.sum() == 1 and g[3]["lost_total"] == 0
    assert np.all(A.sum(axis=1) == R) and not A[cross].any()
    o = gpu_counts(hip, two_halves(False), R, seed=17)
    assert o[3]["lost_total"] == 0 and dense(*o[:3], n)[cross].sum() > 0.1 * n * R


def _mirror_domain(name):
    return part_square(4, 8, 1.0) if name == "half_square" else lattice_domain(True)


def test_progressive_extension_equals_one_trace(hip):
    from rthx.progressive import ProgressiveTrace

    dom = part_square(4, 8, 1.0)
    one = gpu_counts(hip, dom, 1000, seed=1)
    with ProgressiveTrace(dom, seed=1) as t:
        t.extend(300)
        t.extend(700)
        assert t.rays_per_emitter == 1000
        rp, c, v = t.csr()
        assert np.array_equal(rp, one[0]) and np.array_equal(c, one[1]) and np.array_equal(v, one[2])
        assert t.info()["lost_total"] == 0
    dom.invalidate()


@pytest.mark.parametrize("name", ["half_square", "lattice"])
def test_strided_shards_are_rows_of_the_whole(hip, name):
    dom = _mirror_domain(name)
    n = dom.flat().n_emitters
    whole = gpu_counts(hip, dom, 3001, seed=4)
    for begin in range(3):
        shard = gpu_counts(hip, dom, 3001, seed=4, begin=begin, stride=3)
        want = H.csr_rows_subset(*whole[:3], n, np.arange(begin, n, 3))
        for k in range(3):
            assert np.array_equal(shard[k], want[k]), (begin, k)
        assert shard[3]["lost_total"] == 0


# name: (env knobs, trace keywords, R); every branch against the plain unsplit histogram launch of the same rows
_BRANCHES = {
    "short_hash_default": ({}, {}, 2001),
    "forced_hash_bitmap": ({"RTHX_FORCE_HASH": "1"}, {}, 2001),
    "forced_hash_sort": ({"RTHX_FORCE_HASH": "1", "RTHX_HASH_SORT": "1"}, {}, 2001),
    "threads512": ({"RTHX_NO_SHORT_HASH": "1", "RTHX_SPLIT_BELOW": "1", "RTHX_TRACE_THREADS": "512"}, {}, 2001),
    "faithful_hash": ({"RTHX_FORCE_HASH": "1"}, {"flags": 1}, 2001),
    "u32_counters": ({"RTHX_NO_SHORT_HASH": "1", "RTHX_SPLIT_BELOW": "1"}, {"end": 3}, 70_001),
    "split_histogram": ({"RTHX_NO_SHORT_HASH": "1"}, {"end": 3}, 12_301),
    "split_hash_part_lists": ({"RTHX_FORCE_HASH": "1", "RTHX_HASH_MAX": "2048"}, {"end": 3}, 12_301),
    "no_axis_no_clds_knobs": ({"RTHX_NO_AXIS": "1", "RTHX_NO_CLDS": "1", "RTHX_NO_LAT": "1", "RTHX_NO_LOOKBACK": "1"},
                              {}, 2001),
}


@pytest.mark.parametrize("name", ["half_square", "lattice"])
@pytest.mark.parametrize("branch", list(_BRANCHES))
def test_planner_branches_agree(hip, monkeypatch, name, branch):
    """Tally kinds, row splits, workgroup sizes and the sampling flag: the
    counts do not depend on the launch.  (The fast paths a mirror domain never
    takes -- lattices, LDS-staged coarse mesh, look-back -- are bypassed in
    planning: their knobs change nothing.)"""
    env, kw, R = _BRANCHES[branch]
    dom = _mirror_domain(name)
    base_env = {"RTHX_NO_SHORT_HASH": "1", "RTHX_SPLIT_BELOW": "1"}
    for k, v in base_env.items():
        monkeypatch.setenv(k, v)
    want = gpu_counts(hip, dom, R, seed=6, **kw)
    for k in base_env:
        monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got = gpu_counts(hip, dom, R, seed=6, **kw)
    assert_same_counts(got, want, branch)
    assert got[3]["lost_total"] == 0 and got[3]["rays_traced"] == got[3]["rows_traced"] * R


@pytest.mark.parametrize("name", ["half_square", "lattice"])
@pytest.mark.parametrize("env", [{}, {"RTHX_FORCE_HASH": "1", "RTHX_HASH_MAX": "2048"}], ids=["histogram", "split_hash"])
def test_ray_base_ranges_fold_to_one_trace(hip, monkeypatch, name, env):
    """A ray base that is not 0 (rthx_trace_exchange_rays), cut off the groups
    of four: the ranges' counts add up to the one trace's."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    dom = _mirror_domain(name)
    n = dom.flat().n_emitters
    R, cuts = 4099, (0, 1001, 2003, 4099)
    one = gpu_counts(hip, dom, R, seed=8)
    total = np.zeros((n, n))
    for b, e in zip(cuts[:-1], cuts[1:]):
        part = gpu_counts(hip, dom, e - b, seed=8, ray_begin=b)
        assert part[3]["lost_total"] == 0
        total += dense(*part[:3], n)
    assert np.array_equal(total, dense(*one[:3], n))


def test_async_and_device_only_flags(hip):
    """RTHX_FLAG_ASYNC on a mirror domain blocks (no enqueue-only path) and
    RTHX_FLAG_DEVICE_ONLY leaves the CSR on the device: the same counts."""
    dom = part_square(4, 8, 1.0)
    want = gpu_counts(hip, dom, 3000, seed=2)
    flags = abi.RTHX_FLAG_ASYNC | abi.RTHX_FLAG_DEVICE_ONLY
    first = gpu_counts(hip, dom, 3000, seed=2, flags=flags)
    assert_same_counts(first, want, "async | device-only")
    # (a second trace of the same shape into the same result: where a look-back domain goes enqueue-only)
    flat = dom.flat()
    args, _k = _args(hip, flat, 3000, seed=2, flags=flags)
    dd, res = hip.DeviceDomain(flat, 0), hip.DeviceResult()
    try:
        res.trace(dd, args)
        res.trace(dd, args)
        rp, c, v = res.csr()
        assert np.array_equal(rp, want[0]) and np.array_equal(c, want[1]) and np.array_equal(v, want[2])
        assert res.info()["superseded"] == 0 and res.info()["lost_total"] == 0
    finally:
        res.close()
        dd.close()


# --------------------------------------------------------------------------
# errors
# --------------------------------------------------------------------------
def test_bad_flags_are_refused_and_the_setting_stays(hip):
    dom = part_square(4, 8, 1.0)
    flat = dom.flat()
    args, _k = _args(hip, flat, 2000, seed=3)
    dd, res = hip.DeviceDomain(flat, 0), hip.DeviceResult()
    try:
        res.trace(dd, args)
        before = [x.copy() for x in res.csr()]
        solid = flat.coarse_mirror.copy()
        solid[0, 0] = 1  # the bottom wall is solid
        with pytest.raises(hip.RthxError, match="rthx error -1.*solid"):
            dd.set_mirror_walls(solid)
        assert dd.mirror_walls() == 1
        res.trace(dd, args)
        assert all(np.array_equal(a, b) for a, b in zip(res.csr(), before)) and res.info()["lost_total"] == 0
    finally:
        res.close()
        dd.close()
    tri = triangle_domain().flat()
    dd = hip.DeviceDomain(tri, 0)
    try:
        bad = tri.coarse_mirror.copy()
        bad[0, 3] = 1  # a triangle has no wall 3
        with pytest.raises(hip.RthxError, match="rthx error -1"):
            dd.set_mirror_walls(bad)
        assert dd.mirror_walls() == 1
        with pytest.raises(ValueError):
            dd.set_mirror_walls(np.zeros(3, dtype=np.uint8))
    finally:
        dd.close()


def test_recorder_and_direct_method_are_refused(hip):
    dom = part_square(4, 8, 1.0)
    flat = dom.flat()
    lib = hip.load()
    dd, res = hip.DeviceDomain(flat, 0), hip.DeviceResult()
    try:
        args, keep = _args(hip, flat, 100, rec=[0, 3])
        with pytest.raises(hip.RthxError, match="rthx error -1.*mirror"):
            res.trace(dd, args)
        del keep
        n, ns = flat.n_emitters, flat.n_surfaces
        w, eps, om = np.ones(n), np.ones(ns), np.zeros(n - ns)
        reemit, counts = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint64)
        a, info = abi.DirectArgs(), abi.DirectInfo()
        a.rays, a.ray_end, a.nudge, a.seed, a.max_iters = 1000, 1000, H.NUDGE, 1, 100
        dp = C.c_double
        rc = lib.rthx_trace_direct(dd.handle, abi.ptr(w, dp), abi.ptr(eps, dp), abi.ptr(om, dp),
                                   abi.ptr(reemit, C.c_uint8), C.byref(a), abi.ptr(counts, C.c_uint64), C.byref(info))
        assert rc == abi.RTHX_EINVAL and b"mirror" in lib.rthx_last_error()
        assert not counts.any()
        # without the mirror both work on this domain
        dd.set_mirror_walls(None)
        args, keep = _args(hip, flat, 100, rec=[0, 3])
        res.trace(dd, args)
        assert res.info()["n_recorded"] > 0
    finally:
        res.close()
        dd.close()
    with pytest.raises(hip.RthxError, match="mirror"):
        dom(10_000, method="direct", verbose=False)
    dom.invalidate()


# --------------------------------------------------------------------------
# end to end: trace -> smoothing -> solve on the half model
# --------------------------------------------------------------------------
def test_half_model_reproduces_the_full_square_temperatures(hip):
    """Crosbie-Schrenker square, bottom wall hot, kappa = 1: the gas
    temperatures of the 5 x 10 half model with a mirror at x = 0.5 against
    those of the full 10 x 10 square on the cells they share, at 1e5 rays per
    emitter.  Bound: 3 x the full model's own seed-to-seed RMS difference on
    the same cells, computed here from two full runs."""
    from rthx.equilibrium import solve_equilibrium

    R = 100_000

    def gas_T(dom, seed):
        dom(R * dom.num_emitters, seed=seed, verbose=False)
        T, _, _, _ = solve_equilibrium(dom)
        assert abs(dom.energy_error) < 1e-4
        return np.asarray(T[dom.num_surfaces:])

    half = part_square(5, 10, 1.0)
    assert half.flat().coarse_mirror.tolist() == [[0, 1, 0, 0]]
    T_half = gas_T(half, 1)
    half.invalidate()
    T_full = []
    for seed in (1, 2):
        full = H.square_domain(10)
        T_full.append(gas_T(full, seed))
        cells = match_elements(half, full)[half.num_surfaces:] - full.num_surfaces
        full.invalidate()
    assert len(set(cells)) == 50 and T_half.shape == (50,)
    rms = lambda x: float(np.sqrt(np.mean(np.square(x))))
    floor = rms(T_full[0][cells] - T_full[1][cells])
    diff = rms(T_half - T_full[0][cells])
    print(f"half vs full: RMS(T_half - T_full) = {diff:.4f} K, seed-to-seed RMS of the full model = {floor:.4f} K, "
          f"ratio {diff / floor:.3f}")
    assert T_half.min() > 500.0 and floor > 0.0
    assert diff <= 3.0 * floor
