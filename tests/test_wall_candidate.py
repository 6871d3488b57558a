"""The box walls' candidacy test and the theta draw's sine (rthx_device.h
wall_candidate, sin_theta_u32).

wall_candidate(s, d) decides whether the wall on the side a ray points to, at
the signed distance s along an axis with direction component d, can be hit:
|d| >= 1e-10 and |s| > 0.  Earlier versions formed the product |s| |d| > 0;
the reference forms the quotient (distToSurface2D.jl).  The three agree except
where the product underflows to zero, 0 < |s| < 2^-1040, and there the new form
is the reference's.

Host (no GPU): the three forms on the cross product of
  s in +-{0, 2^-1074, 2^-1041, 2^-1040, 1e-300, 2^-60, 1e-16, 0.3, 1}
  d in +-{0, 5e-11, nextafter(1e-10, 0), 1e-10, nextafter(1e-10, 1), 1e-3, 1}.

GPU: sin_theta_u32 against the earlier expression 2.0 * sqrt_unit(u (1 - u))
on all 2^32 words (16 launches of 2^28, 0 differing words required), and
against numpy on edge words and 10^5 random words; then exact CSR parity with
the CPU oracle (every row, no tolerance, lost totals included) on shapes where
the candidacy test decides: a 3 x 2 lattice on (-0.4, 0.25)-(0.1, 0.95) (s of
both signs, x0, y0 != 0) with all walls solid and with the right and top walls
open, the 4 x 4 unit square (dyadic bounds: rays end on bounds exactly more
often) at kappa = 0.01 and 1, a 1 x 1 lattice, an edge round (R = 4099), each
on volume and surface rows (lat_ray_fast<true> and <false>) and again from a
non-zero ray base (segment_lat / box_hit_in); a 2-polygon MLAT domain and a
direct-method trace, which go through box_hit_in.  box_hit_in itself keeps the
product form (with wall_candidate the MLAT walks measured slower,
profiles/round17/INDEX.md); its cases stay, so a later change of that site
meets them.
"""
import ctypes as C

import numpy as np
import pytest

import helpers as H
from oracle import oracle
from rthx import PolyVolume2D, RayTracingDomain2D

# --------------------------------------------------------------------------
# host: the candidacy predicate
# --------------------------------------------------------------------------
S_MAGS = [0.0, 2.0 ** -1074, 2.0 ** -1041, 2.0 ** -1040, 1e-300, 2.0 ** -60, 1e-16, 0.3, 1.0]
D_MAGS = [0.0, 5e-11, float(np.nextafter(1e-10, 0.0)), 1e-10, float(np.nextafter(1e-10, 1.0)), 1e-3, 1.0]
NEW, PRODUCT, QUOTIENT = 0, 1, 2

# The corner 0 < |s| < 2^-1040, listed in full: for every |d| of D_MAGS the
# value (new, product, quotient) gives, the same for either sign of s and d.
# 2^-1041 |d| is at least half of the least subnormal for |d| >= 1e-3 only
# (2^-1041 1e-10 = 0.87 2^-1074 rounds up to 2^-1074, so the product form
# still sees it there); 2^-1074 |d| rounds to 0 for every |d| <= 1/2.
CORNER = {
    2.0 ** -1074: {0.0: (0, 0, 0), 5e-11: (0, 0, 0), D_MAGS[2]: (0, 0, 0), 1e-10: (1, 0, 1), D_MAGS[4]: (1, 0, 1),
                   1e-3: (1, 0, 1), 1.0: (1, 1, 1)},
    2.0 ** -1041: {0.0: (0, 0, 0), 5e-11: (0, 0, 0), D_MAGS[2]: (0, 0, 0), 1e-10: (1, 1, 1), D_MAGS[4]: (1, 1, 1),
                   1e-3: (1, 1, 1), 1.0: (1, 1, 1)},
}


def _forms(s, d):
    from rthx import _lib

    f = _lib.load().rthx_debug_wall_candidate
    out = tuple(f(s, d, form) for form in (NEW, PRODUCT, QUOTIENT))
    assert all(v in (0, 1) for v in out), out
    return out


def _signed(mags):
    return [sg * m for m in mags for sg in (1.0, -1.0)]


def test_candidacy_is_the_quotient_form_everywhere():
    for s in _signed(S_MAGS):
        for d in _signed(D_MAGS):
            new, _prod, quot = _forms(s, d)
            assert new == quot, (s, d, new, quot)
            assert new == int(abs(d) >= 1e-10 and s != 0.0), (s, d, new)


def test_candidacy_is_the_product_form_outside_the_underflow_corner():
    n = 0
    for s in _signed(S_MAGS):
        if 0.0 < abs(s) < 2.0 ** -1040:
            continue
        for d in _signed(D_MAGS):
            new, prod, _quot = _forms(s, d)
            assert new == prod, (s, d, new, prod)
            n += 1
    assert n == 2 * 7 * 2 * 7


def test_the_underflow_corner_is_listed():
    """Every pair with 0 < |s| < 2^-1040: the value each form gives."""
    inside = [m for m in S_MAGS if 0.0 < m < 2.0 ** -1040]
    assert sorted(inside) == sorted(CORNER)
    differ = 0
    for m in inside:
        assert sorted(CORNER[m]) == sorted(D_MAGS)
        for dm in D_MAGS:
            for s in (m, -m):
                for d in (dm, -dm):
                    got = _forms(s, d)
                    print(f"s = {s!r:>24} d = {d!r:>24}: new {got[0]} product {got[1]} quotient {got[2]}")
                    assert got == CORNER[m][dm], (s, d, got, CORNER[m][dm])
                    differ += got[NEW] != got[PRODUCT]
    assert differ == 4 * 3  # 2^-1074 against |d| in [1e-10, 1e-3]: the product underflows, the quotient does not


# --------------------------------------------------------------------------
# GPU: sin(theta) of the isotropic draw
# --------------------------------------------------------------------------
@pytest.mark.gpu
def test_sin_theta_equals_the_earlier_expression_on_every_word(hip):
    lib = hip.load()
    total = 0
    for k in range(16):
        n_diff, first = C.c_uint64(1 << 63), C.c_uint64(0)
        rc = lib.rthx_debug_sin_theta_sweep(0, k << 28, 1 << 28, C.byref(n_diff), C.byref(first))
        assert rc == 0, lib.rthx_last_error()
        print(f"words [{k} 2^28, {k + 1} 2^28): {n_diff.value} differ" + (f", first {first.value:#x}" if n_diff.value else ""))
        total += n_diff.value
    assert total == 0, f"{total} of 2^32 words differ from 2.0 * sqrt_unit(u (1 - u))"


@pytest.mark.gpu
def test_sin_theta_sweep_refuses_a_range_past_the_last_word(hip):
    lib = hip.load()
    n_diff, first = C.c_uint64(0), C.c_uint64(0)
    assert lib.rthx_debug_sin_theta_sweep(0, 15 << 28, (1 << 28) + 1, C.byref(n_diff), C.byref(first)) != 0


@pytest.mark.gpu
def test_sin_theta_against_numpy(hip):
    """2 sqrt(u (1 - u)) with u (1 - u) formed as the oracle forms it (u =
    w 2^-32, 1 - u exact, one rounded product) and numpy's correctly rounded
    root: the same bits."""
    lib = hip.load()
    rng = np.random.default_rng(20261020)
    w = np.concatenate([np.array([0, 1, 2**31 - 1, 2**31, 2**31 + 1, 2**32 - 1], dtype=np.uint32),
                        rng.integers(0, 2**32, size=100_000, dtype=np.uint64).astype(np.uint32)])
    out = np.empty(w.size)
    rc = lib.rthx_debug_sin_theta(0, w.ctypes.data_as(C.POINTER(C.c_uint32)), w.size,
                                  out.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == 0, lib.rthx_last_error()
    u = w.astype(np.float64) * 2.0 ** -32
    want = 2.0 * np.sqrt(u * (1.0 - u))
    bad = np.flatnonzero(out.view(np.uint64) != want.view(np.uint64))
    assert bad.size == 0, f"{bad.size} words differ, first {int(w[bad[0]]):#x}: {out[bad[0]]!r} != {want[bad[0]]!r}"
    assert out[0] == 0.0 and out[3] == 1.0


# --------------------------------------------------------------------------
# GPU: exact parity with the CPU oracle
# --------------------------------------------------------------------------
_ORACLE = {}
_DOMAINS = {}


def _rect(x0, y0, x1, y1, nx, ny, kappa, open_walls=()):
    # walls: 0 bottom, 1 right, 2 top, 3 left (bit w of the coarse solid mask)
    face = PolyVolume2D([(x0, y0), (x1, y0), (x1, y1), (x0, y1)], [w not in open_walls for w in range(4)], 1, kappa, 0.0)
    face.T_in_w = [1000.0, 0.0, 0.0, 0.0]
    face.epsilon = [1.0] * 4
    face.T_in_g = -1.0
    face.q_in_g = 0.0
    return RayTracingDomain2D([face], [(nx, ny)])


_MAKE = {
    "off32": lambda: _rect(-0.4, 0.25, 0.1, 0.95, 3, 2, 1.0),
    "off32_open12": lambda: _rect(-0.4, 0.25, 0.1, 0.95, 3, 2, 1.0, (1, 2)),
    "unit4_thin": lambda: _rect(0.0, 0.0, 1.0, 1.0, 4, 4, 0.01),
    "unit4": lambda: _rect(0.0, 0.0, 1.0, 1.0, 4, 4, 1.0),
    "one": lambda: _rect(-0.4, 0.25, 0.1, 0.95, 1, 1, 1.0),
    "mlat2": lambda: H.quad_lattice_domain(2, 1, 4, 3),
}
# (key, R): R = 4099 on 256 lanes is four full rounds and one group whose last
# three rays lie outside the row's range
CASES = [("off32", 2052), ("off32_open12", 2052), ("unit4_thin", 2052), ("unit4", 2052), ("one", 2052),
         ("off32_open12", 4099), ("mlat2", 1500)]


def _case(hip, key, R, seed=61):
    k = (key, R, seed)
    if k not in _ORACLE:
        if key not in _DOMAINS:
            _DOMAINS[key] = _MAKE[key]().flat()
        flat = _DOMAINS[key]
        args, keep = hip.make_args(0, R, H.NUDGE, seed, 0, flat.n_emitters)
        rp, cols, cnt, info = oracle.trace_exchange(flat, args, 16)[:4]
        for a in (rp, cols, cnt):
            a.setflags(write=False)
        _ORACLE[k] = (flat, args, keep, (rp, cols, cnt), info)
    flat, args, _keep, want, info = _ORACLE[k]
    return flat, args, want, info


def _gpu(hip, flat, args, cuts=None):
    """One trace, or the ray ranges [cuts[i], cuts[i+1]) traced one by one
    (rthx_trace_exchange_rays) and accumulated."""
    dd = hip.DeviceDomain(flat, 0)
    res, part = hip.DeviceResult(), hip.DeviceResult()
    try:
        if cuts is None:
            res.trace(dd, args)
        else:
            for n, (b, e) in enumerate(zip(cuts[:-1], cuts[1:])):
                a, keep = hip.make_args(0, e - b, H.NUDGE, args.seed, 0, flat.n_emitters)
                (res if n == 0 else part).trace(dd, a, ray_begin=b)
                if n:
                    res.accumulate(part)
                del keep
        rp, cols, cnt = res.csr()
        return (rp.copy(), cols.copy(), cnt.copy()), res.info()
    finally:
        part.close()
        res.close()
        dd.close()


@pytest.mark.gpu
@pytest.mark.parametrize("base", [0, 1001])
@pytest.mark.parametrize("key,R", CASES)
def test_counts_equal_the_oracle(hip, monkeypatch, key, R, base):
    """base = 1001: the rays [0, 1001) and [1001, R) as two traces, the second
    through the instance that reads a ray base and keeps segment_lat."""
    flat, args, want, oinfo = _case(hip, key, R)
    if "open" in key:  # a case that loses no ray proves nothing about an open wall
        assert 0.05 <= oinfo["lost_total"] / oinfo["rays_traced"] <= 0.95
    elif key != "one":  # (the mesher gives a 1 x 1 mesh's only cell two solid fine walls: the oracle loses rays there)
        assert oinfo["lost_total"] == 0
    monkeypatch.setenv("RTHX_NO_SHORT_HASH", "1")
    monkeypatch.setenv("RTHX_SPLIT_BELOW", "1")
    monkeypatch.setenv("RTHX_TRACE_THREADS", "256")
    got, info = _gpu(hip, flat, args, cuts=(0, base, R) if base else None)
    assert np.array_equal(got[0], want[0]), "row_ptr differs from the oracle"
    assert np.array_equal(got[1], want[1]), "cols differ from the oracle"
    assert np.array_equal(got[2], want[2]), "counts differ from the oracle"
    assert info["lost_total"] == oinfo["lost_total"]
    if not base:
        for k in ("rays_traced", "lost_max_row"):
            assert info[k] == oinfo[k], (k, info[k], oinfo[k])
    # both loops ran: surface rows and volume rows are present and tallied
    ns = flat.n_surfaces
    rows = np.diff(want[0])
    assert ns > 0 and np.all(rows[:ns] > 0) and np.all(rows[ns:] > 0)


@pytest.mark.gpu
def test_direct_method_counts_equal_the_oracle(hip):
    """The direct method's legs go through box_hit_in: the 5 x 5 reflecting,
    scattering square, the smallest of tests/test_gpu_direct.py."""
    from rthx import direct as DR
    from rthx._lib import device_domain

    dom = H.square_domain(5, kappa=0.5, sigma_s=0.5, epsilon=0.6, T_walls=(1000.0, -1.0, 400.0, -1.0))
    w, _ = DR.prepare_emitters(dom, 1)
    eps, om, re = DR.element_data(dom, 1)
    args = DR.make_direct_args(0, 200_000, H.NUDGE, 2)
    g, gi = DR.trace_direct_counts(device_domain(dom, 0), w, eps, om, re, args)
    o, oi = oracle.trace_direct(dom.flat(), w, eps, om, re, args, 16)
    assert int(np.count_nonzero(g != o)) == 0, (gi, oi)
    for k in ("rays_traced", "absorbed", "escaped", "rouletted", "capped", "events", "replayed"):
        assert gi[k] == oi[k], (k, gi[k], oi[k])
    assert gi["events"] > gi["absorbed"]
