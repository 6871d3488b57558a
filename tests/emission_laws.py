"""Analytic laws of 2D emission and free paths, and the statistics that hold
recorded rays to them (tests/test_emission_laws.py on the CPU restatement,
tests/test_gpu_emission_laws.py on the device).  A plain helper module.

The recorder returns the origin o and the absorption point e of every ray of
one emitter.  Far from every solid wall (an optically thick enclosure) the
pair obeys closed-form laws in which nothing of this project's code appears.

A 2D ray is the in-plane projection of a 3D ray, and the direction is left
un-normalised (emitVolumeRay2D.jl:26-31, lambertSample2D.jl).  Write the 3D
unit direction by its in-plane angle alpha and its elevation gamma off the
plane, gamma in (-pi/2, pi/2): the solid angle is dOmega = cos(gamma) dgamma
dalpha, and a 3D length s projects to the 2D length s cos(gamma).  The 3D
free path has optical depth t3 = -ln u, P(t3 > x) = exp(-x), whatever beta
does along the ray.  So the optical depth tau along the 2D segment from o to
e is tau = t3 cos(gamma), and

    P(tau > t | gamma) = exp(-t / cos(gamma)).

With the Bickley function Ki_n(x) = int_0^{pi/2} cos^{n-1}(gamma)
exp(-x / cos(gamma)) dgamma (Ki_1(0) = pi/2, Ki_2(0) = 1, Ki_3(0) = pi/4,
Ki_4(0) = 2/3, Ki_5(0) = 3 pi/16; Ki_n' = -Ki_{n-1}):

1. Volume emitter, direction: isotropic, density dOmega / (4 pi) = cos(gamma)
   dgamma dalpha / (4 pi).  It factorises, so alpha = atan2(e - o) is uniform
   on the circle and independent of gamma.
2. Volume emitter, free path: P(tau > t) = (1 / 4 pi) 2 pi 2 int_0^{pi/2}
   cos(gamma) exp(-t / cos(gamma)) dgamma = Ki_2(t).  Mean int_0^inf Ki_2 =
   Ki_3(0) = pi/4; second moment 2 int t Ki_2 = 2 Ki_4(0) = 4/3.
   Uniform beta: tau = beta |e - o|.  Beta a function of y only: along a
   straight segment dl = |e - o| / |y_e - y_o| dy, so tau = |e - o|
   |B(y_e) - B(y_o)| / |y_e - y_o| with B = int beta dy, and tau = beta(y_o)
   |e - o| in the limit y_e = y_o.
3. Surface emitter, direction: Lambert, density cos(theta) dOmega / pi with
   cos(theta) = cos(gamma) cos(alpha), alpha the in-plane angle off the inward
   normal: cos^2(gamma) cos(alpha) dgamma dalpha / pi.  The marginal of alpha
   is cos(alpha) / 2 on (-pi/2, pi/2): sin(alpha) is uniform on (-1, 1), and
   the normal component is positive for every ray.  (e - o) . t = |e - o|
   sin(alpha), t the wall's unit tangent.
4. Surface emitter, free path: P(tau > t) = (1 / pi) 2 . 2 Ki_3(t) =
   Ki_3(t) / Ki_3(0).  Mean Ki_4(0) / Ki_3(0) = 8 / (3 pi); second moment
   2 Ki_5(0) / Ki_3(0) = 3/2.
5. Origins: the wall parameter is uniform on [0, 1]; a point in a triangle is
   uniform, so each barycentric coordinate has the CDF 1 - (1 - a)^2; a point
   in a quad is uniform: ABC holds area(ABC) / area of the origins and they
   are uniform within ABC and within CDA.  The nudge toward the midpoint
   (helpers.NUDGE, 2e-12 relative) is below every statistic's resolution.
6. Independence: origin, alpha and tau are pairwise independent (the
   densities above factorise, and t3 is drawn apart).  A draw word used twice
   would show here.

Every statistic returns a p-value; seeds are fixed, so a run is deterministic,
and the bound is tests/test_gpu_mirror.py's P_BOUND = 1e-7.  The Kolmogorov-
Smirnov tests at n = 2e5 resolve about 1e-3 in a CDF, so the CDF tables are
held to 1e-7.
"""
from __future__ import annotations

import functools
import json
import math
import os

import numpy as np
import scipy.integrate
import scipy.interpolate
import scipy.stats

import helpers as H
from oracle import oracle
from rthx import PolyVolume2D, RayTracingDomain2D, abi

P_BOUND = 1e-7  # tests/test_gpu_mirror.py
R_LAWS = 200_000
FAITHFUL = abi.RTHX_FLAG_FAITHFUL_SAMPLING

KI0 = {2: 1.0, 3: math.pi / 4}
TAU_MEAN = {2: math.pi / 4, 3: 8 / (3 * math.pi)}
TAU_VAR = {2: 4 / 3 - (math.pi / 4) ** 2, 3: 3 / 2 - (8 / (3 * math.pi)) ** 2}


# --------------------------------------------------------------------------
# Bickley functions
# --------------------------------------------------------------------------
def bickley(n: int, x: float) -> float:
    """Ki_n(x) by adaptive quadrature."""
    f = lambda g: math.cos(g) ** (n - 1) * math.exp(-x / math.cos(g)) if math.cos(g) > 0 else 0.0
    return scipy.integrate.quad(f, 0.0, math.pi / 2, epsabs=1e-12, epsrel=1e-11, limit=200)[0]


_T_MAX = 40.0  # Ki_2(40) < 1e-18; -ln of a 32-bit draw stays below 23
_N_NODES = 1201


@functools.lru_cache(maxsize=None)
def tau_cdf(n: int):
    """t -> 1 - Ki_n(t) / Ki_n(0), the CDF of tau (n = 2: volume emitter,
    n = 3: surface emitter).  A cubic spline in s = sqrt(t) through
    quadrature values (Ki_n'' = Ki_{n-2} is logarithmic at 0 in t, not in s),
    checked against direct quadrature at 50 random points to 1e-7."""
    s = np.linspace(0.0, math.sqrt(_T_MAX), _N_NODES)
    ki = np.array([bickley(n, float(v * v)) for v in s])
    assert abs(ki[0] - KI0[n]) < 1e-12
    spline = scipy.interpolate.CubicSpline(s, 1.0 - ki / KI0[n])

    def cdf(t):
        t = np.asarray(t, dtype=np.float64)
        return np.where(t >= _T_MAX, 1.0, np.clip(spline(np.sqrt(np.clip(t, 0.0, _T_MAX))), 0.0, 1.0))

    assert table_error(n, cdf) <= 1e-7
    return cdf


def table_error(n: int, cdf=None, points: int = 50, seed: int = 2021) -> float:
    """max |table - quadrature| of tau_cdf(n) at random points: half of them
    uniform in (0, 3), where the mass is, half log-uniform in (1e-6, 40)."""
    cdf = tau_cdf(n) if cdf is None else cdf
    rng = np.random.default_rng(seed + n)
    t = np.concatenate([rng.uniform(0.0, 3.0, points // 2),
                        np.exp(rng.uniform(math.log(1e-6), math.log(_T_MAX), points - points // 2))])
    want = np.array([1.0 - bickley(n, float(x)) / KI0[n] for x in t])
    return float(np.abs(cdf(t) - want).max())


# --------------------------------------------------------------------------
# geometry from the flat domain
# --------------------------------------------------------------------------
def cell_polygon(flat, f: int) -> np.ndarray:
    """Vertices [nv, 2] of fine cell f (global fine index)."""
    return flat.fine_xy.reshape(-1, 4, 2)[f, : int(flat.fine_nv[f])].copy()


def emitter_wall(flat, g: int):
    """(p1, p2) of surface emitter g: wall w of its fine cell runs from vertex
    w to vertex w + 1, the cell counter-clockwise, so the inward normal is the
    tangent's left normal."""
    f, w = np.argwhere(flat.fine_surface.reshape(-1, 4) == g)[0]
    poly = cell_polygon(flat, int(f))
    return poly[w], poly[(w + 1) % len(poly)]


def mid_wall_emitters(flat):
    """The surface element at the middle of each coarse wall of a one-polygon
    domain."""
    cxy = flat.coarse_xy.reshape(-1, 4, 2)[0]
    mids = np.array([0.5 * sum(emitter_wall(flat, g)) for g in range(flat.n_surfaces)])
    out = []
    for k in range(4):
        m = 0.5 * (cxy[k] + cxy[(k + 1) % 4])
        d = np.linalg.norm(mids - m, axis=1)
        assert d.min() < 1e-12
        out.append(int(np.argmin(d)))
    return out


def slab_B(flat):
    """y -> int_0^y beta dy of a layered slab (helpers.layered_slab_domain:
    every coarse polygon a layer of one beta)."""
    cxy = flat.coarse_xy.reshape(-1, 4, 2)
    beta = flat.beta.reshape(flat.n_bins, flat.n_fine)[0]
    y0, y1 = cxy[:, :, 1].min(axis=1), cxy[:, :, 1].max(axis=1)
    order = np.argsort(y0)
    assert np.allclose(y0[order][1:], y1[order][:-1], rtol=0, atol=1e-15)
    b = []
    for c in order:
        cells = beta[flat.fine_offset[c]:flat.fine_offset[c + 1]]
        assert np.all(cells == cells[0])
        b.append(cells[0])
    edges = np.append(y0[order], y1[order][-1])
    cum = np.concatenate([[0.0], np.cumsum(np.array(b) * np.diff(edges))])
    return (lambda y: np.interp(y, edges, cum)), (lambda y: np.array(b)[np.clip(np.searchsorted(edges, y, "right") - 1,
                                                                                0, len(b) - 1)])


def optical_depth(flat, o, e):
    """tau along the segment o -> e (law 2): uniform beta, or beta(y)."""
    d = np.linalg.norm(e - o, axis=1)
    if flat.uniform_beta[0] > -0.1:
        return flat.beta[0] * d
    B, beta_at = slab_B(flat)
    dy = np.abs(e[:, 1] - o[:, 1])
    flat_ray = dy < 1e-9
    mean_beta = np.abs(B(e[:, 1]) - B(o[:, 1])) / np.where(flat_ray, 1.0, dy)
    return d * np.where(flat_ray, beta_at(o[:, 1]), mean_beta)


def barycentric(tri, p):
    """Barycentric coordinates [n, 3] of points p in triangle tri [3, 2]."""
    a, b, c = tri
    T = np.array([[b[0] - a[0], c[0] - a[0]], [b[1] - a[1], c[1] - a[1]]])
    lb, lc = np.linalg.solve(T, (p - a).T)
    return np.stack([1.0 - lb - lc, lb, lc], axis=1)


def tri_area(tri):
    a, b, c = tri
    return 0.5 * ((b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0]))


# --------------------------------------------------------------------------
# statistics
# --------------------------------------------------------------------------
def _ks(x, cdf):
    return float(scipy.stats.kstest(x, cdf).pvalue)


def _uniform(x):
    return np.clip(x, 0.0, 1.0)


def _bary_cdf(a):
    a = np.clip(a, 0.0, 1.0)
    return 1.0 - (1.0 - a) ** 2


def _terciles(x):
    return np.digitize(x, np.quantile(x, [1 / 3, 2 / 3]))


def _independent(i, j, ni, nj):
    table = np.zeros((ni, nj))
    np.add.at(table, (i, j), 1)
    return float(scipy.stats.chi2_contingency(table, correction=False)[1])


def _triangles(flat, g, o):
    """[(name, triangle, the origins in it)] of volume emitter g, and the
    share of ABC (None for a triangle cell)."""
    poly = cell_polygon(flat, g - flat.n_surfaces)
    if len(poly) == 3:
        return [("tri", poly, o)], None
    abc, cda = poly[[0, 1, 2]], poly[[2, 3, 0]]
    in_abc = barycentric(abc, o)[:, 1] > 0.0  # (B's side of the diagonal AC)
    return [("abc", abc, o[in_abc]), ("cda", cda, o[~in_abc])], tri_area(abc) / (tri_area(abc) + tri_area(cda))


def measure(flat, g, o, e):
    """What the laws speak of, from the recorded rays of emitter g: a dict
    with tau, the order n of its law, the angle statistic u_angle (uniform on
    [0, 1] under laws 1 / 3), its 8 bins, and the origin coordinate (x of a
    volume origin, the wall parameter of a surface origin)."""
    d = e - o
    m = {"tau": optical_depth(flat, o, e), "surface": g < flat.n_surfaces}
    if m["surface"]:
        p1, p2 = emitter_wall(flat, g)
        L = np.linalg.norm(p2 - p1)
        t = (p2 - p1) / L
        nrm = np.array([-t[1], t[0]])
        m["normal"] = d @ nrm
        m["sin_alpha"] = (d @ t) / np.linalg.norm(d, axis=1)
        m["u_angle"] = 0.5 * (m["sin_alpha"] + 1.0)
        m["coord"] = ((o - p1) @ t) / L
        m["n"] = 3
    else:
        m["u_angle"] = (np.arctan2(d[:, 1], d[:, 0]) + math.pi) / (2 * math.pi)
        m["coord"] = o[:, 0]
        m["n"] = 2
    m["octant"] = np.clip((8 * m["u_angle"]).astype(np.int64), 0, 7)
    return m


def laws(flat, g, o, e):
    """Named p-values of laws 1-6 for the recorded rays (o, e) of emitter g.
    What a law states without a distribution (a positive normal component,
    origins inside the cell) is asserted here."""
    m = measure(flat, g, o, e)
    n, tau, R = m["n"], m["tau"], len(o)
    p = {}
    if m["surface"]:
        assert np.all(m["normal"] > 0.0)                                    # law 3
        assert m["coord"].min() > -1e-9 and m["coord"].max() < 1.0 + 1e-9
        p["sin_alpha_uniform"] = _ks(m["u_angle"], _uniform)                # law 3
        p["wall_parameter_uniform"] = _ks(m["coord"], _uniform)             # law 5
    else:
        p["angle_uniform"] = _ks(m["u_angle"], _uniform)                    # law 1
        tris, share = _triangles(flat, g, o)
        for name, tri, pts in tris:                                         # law 5
            lam = barycentric(tri, pts)
            assert lam.min() >= -1e-9, (name, lam.min())
            for k, v in enumerate("abc"):
                p[f"{name}_barycentric_{v}"] = _ks(lam[:, k], _bary_cdf)
        if share is not None:
            z = (len(tris[0][2]) - R * share) / math.sqrt(R * share * (1.0 - share))
            assert abs(z) <= 5.0, (z, share)
            p["abc_share"] = float(2 * scipy.stats.norm.sf(abs(z)))
    p[f"tau_ki{n}"] = _ks(tau, tau_cdf(n))                                  # laws 2, 4
    z = (tau.mean() - TAU_MEAN[n]) / math.sqrt(TAU_VAR[n] / R)
    p["tau_mean"] = float(2 * scipy.stats.norm.sf(abs(z)))
    x3, t3 = _terciles(m["coord"]), _terciles(tau)                          # law 6
    p["independent_origin_angle"] = _independent(x3, m["octant"], 3, 8)
    p["independent_angle_tau"] = _independent(m["octant"], t3, 8, 3)
    p["independent_origin_tau"] = _independent(x3, t3, 3, 3)
    return p


def controls(flat, g, o, e):
    """Named p-values of the power controls on the same rays: each must be
    rejected (p < P_BOUND), or the laws' passing says nothing."""
    m = measure(flat, g, o, e)
    n, tau = m["n"], m["tau"]
    p = {"tau_scaled_1.03": _ks(1.03 * tau, tau_cdf(n)),
         f"tau_against_ki{5 - n}": _ks(tau, tau_cdf(5 - n))}
    if m["surface"]:
        p["alpha_uniform"] = _ks(np.arcsin(np.clip(m["sin_alpha"], -1.0, 1.0)) / math.pi + 0.5, _uniform)
    else:
        for name, tri, pts in _triangles(flat, g, o)[0]:
            lam = barycentric(tri, pts)
            for k, v in enumerate("abc"):
                p[f"{name}_barycentric_{v}_against_uniform"] = _ks(lam[:, k], _uniform)
    return p


# --------------------------------------------------------------------------
# the cases: optically thick domains, every solid wall far from the emitter
# --------------------------------------------------------------------------
def _square_emitters(flat):
    return {"centre": flat.n_surfaces + 12, **{f"wall{k}": g for k, g in enumerate(mid_wall_emitters(flat))}}


def _wedge_emitters(flat):
    # fine cells 0, 1, 2 of wedge 1: a triangle, a trapezoid, a triangle, all at the hub
    return {f"cell{k}": flat.n_surfaces + int(flat.fine_offset[1]) + k for k in range(3)}


def _layer_emitters(flat):
    # the lower middle cell (column 2 of 5, row 0 of 2) of layers 2 and 3 (from 0)
    return {f"layer{c}": flat.n_surfaces + int(flat.fine_offset[c]) + 2 for c in (2, 3)}


LAYER_KAPPAS = (30, 60, 20, 50, 40, 25)
# name: (domain, emitters, seed)
LAW_CASES = {
    "square": (lambda: H.square_domain(5, kappa=60), _square_emitters, 5),
    "rotated": (lambda: H.square_domain(5, kappa=60, rotation=0.3), _square_emitters, 7),
    "wedge": (lambda: H.wedge_domain(8, 3, kappa=60), _wedge_emitters, 9),
    "layers": (lambda: H.layered_slab_domain(LAYER_KAPPAS, W=4.0, nx=5), _layer_emitters, 11),
}
LAW_EMITTERS = [("square", k) for k in ("centre", "wall0", "wall1", "wall2", "wall3")] + \
               [("rotated", k) for k in ("centre", "wall0", "wall1", "wall2", "wall3")] + \
               [("wedge", f"cell{k}") for k in range(3)] + [("layers", "layer2"), ("layers", "layer3")]
LAW_IDS = [f"{c}-{k}" for c, k in LAW_EMITTERS]


@functools.lru_cache(maxsize=None)
def law_flat(case):
    flat = LAW_CASES[case][0]().flat()
    return flat, LAW_CASES[case][1](flat)


def law_args(case, key, flags):
    """(flat, g, args, keep-alive) of one recorded row: emitter g alone."""
    flat, emitters = law_flat(case)
    g = emitters[key]
    args, keep = oracle.make_args(0, R_LAWS, H.NUDGE, LAW_CASES[case][2], g, g + 1, 1, flags=flags, record_ids=[g])
    return flat, g, args, keep


def check_row(flat, g, rp, cols, cnt, info, rays):
    """The conditions under which the laws hold for the row: no ray lost,
    none absorbed by a surface, every ray recorded."""
    assert info["lost_total"] == 0
    row = cols[rp[g]:rp[g + 1]]
    assert row.size and row.min() >= flat.n_surfaces
    assert int(cnt[rp[g]:rp[g + 1]].sum()) == R_LAWS and rp[g + 1] - rp[g] == len(cols)
    assert info["n_recorded"] == R_LAWS and len(rays[0]) == R_LAWS and np.all(rays[2] == g)


@functools.lru_cache(maxsize=None)
def restatement_rays(case, key, flags):
    """(origins, endpoints) of the CPU restatement, computed once and left
    unchanged."""
    flat, g, args, _keep = law_args(case, key, flags)
    rp, cols, cnt, info, rays = oracle.trace_exchange(flat, args, 1)
    check_row(flat, g, rp, cols, cnt, info, rays)
    for a in rays[:2]:
        a.setflags(write=False)
    return rays[0], rays[1]


# --------------------------------------------------------------------------
# the two sampling modes, count for count
# --------------------------------------------------------------------------
R_MODES = 200_000
MODE_SEEDS = (101, 202)  # default sampling, faithful sampling


def open_square(kappa=1.0):
    """tests/test_gpu_ray_body.py's open-wall 5 x 5 square, kappa a parameter."""
    face = PolyVolume2D([(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)], [True, False, True, True], 1, kappa, 0.0)
    face.T_in_w = [1000.0, 0.0, 0.0, 0.0]
    face.epsilon = [1.0] * 4
    face.T_in_g = -1.0
    face.q_in_g = 0.0
    return RayTracingDomain2D([face], [(5, 5)])


SLAB_KAPPAS = (0.5, 1.5, 1.0, 2.0)
# name: every kappa scaled by s -> domain
MODE_CASES = {
    "square5": lambda s=1.0: H.square_domain(5, kappa=s),
    "rotated5": lambda s=1.0: H.square_domain(5, kappa=s, rotation=0.3),
    "wedges": lambda s=1.0: H.wedge_domain(8, 2, kappa=s),
    "quad_lattice": lambda s=1.0: H.quad_lattice_domain(kappa=0.8 * s),
    "open5": lambda s=1.0: open_square(s),
    "layered_slab": lambda s=1.0: H.layered_slab_domain(tuple(k * s for k in SLAB_KAPPAS)),
}
MODE_CPU_CASES = ("square5", "rotated5", "wedges", "quad_lattice")


def mode_runs(case):
    """[(name, flat, args, keep-alive)]: default sampling at seed 101,
    faithful at seed 202, and the control, faithful with every kappa x 1.02."""
    out = []
    for name, scale, seed, flags in (("default", 1.0, MODE_SEEDS[0], 0), ("faithful", 1.0, MODE_SEEDS[1], FAITHFUL),
                                     ("faithful_kappa_1.02", 1.02, MODE_SEEDS[1], FAITHFUL)):
        flat = MODE_CASES[case](scale).flat()
        args, keep = oracle.make_args(0, R_MODES, H.NUDGE, seed, 0, flat.n_emitters, 1, flags=flags)
        out.append((name, flat, args, keep))
    return out


def compare_modes(case, A, B, C, closed=True):
    """Asserts the acceptance of the count-level comparison on the dense
    count matrices A (default), B (faithful), C (the control) and returns the
    figures."""
    x2, dof = H.homogeneity(A, B, min_bin=40)
    hi, lo = scipy.stats.chi2.isf(P_BOUND, dof), scipy.stats.chi2.ppf(P_BOUND, dof)
    x2c, dofc = H.homogeneity(A, C, min_bin=40)
    fig = {"x2": x2, "dof": dof, "z": (x2 - dof) / math.sqrt(2 * dof), "bound_hi": float(hi), "bound_lo": float(lo),
           "control_x2": x2c, "control_dof": dofc, "control_z": (x2c - dofc) / math.sqrt(2 * dofc)}
    la, lb = R_MODES - A.sum(axis=1), R_MODES - B.sum(axis=1)
    if not closed:  # lost totals within 5 binomial sigma, the rows' variances summed
        ph = (la + lb) / (2.0 * R_MODES)
        fig["lost"] = [float(la.sum()), float(lb.sum())]
        fig["lost_z"] = float((la.sum() - lb.sum()) / math.sqrt(2.0 * R_MODES * np.sum(ph * (1.0 - ph))))
    print(f"{case}: {fig}")
    if closed:
        assert not la.any() and not lb.any()
    else:
        assert la.sum() > 0 and abs(fig["lost_z"]) <= 5.0
    assert x2 <= hi, (x2, dof, hi)
    assert x2 >= lo, (x2, dof, lo)  # (two independent seeds do not agree too well either)
    assert x2c > scipy.stats.chi2.isf(P_BOUND, dofc), (x2c, dofc)
    return fig


# --------------------------------------------------------------------------
# measurement runs: the figures as JSON
# --------------------------------------------------------------------------
def record(side, key, figures):
    """With RTHX_EMISSION_LAWS_RECORD=<file> set, merge {side: {key:
    figures}} into that JSON file (side: "cpu" or "gpu")."""
    path = os.environ.get("RTHX_EMISSION_LAWS_RECORD")
    if not path:
        return
    data = {}
    if os.path.exists(path):
        with open(path) as f:
            data = json.load(f)
    data.setdefault(side, {})[key] = figures
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
