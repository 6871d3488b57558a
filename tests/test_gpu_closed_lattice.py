"""The closed-enclosure copy of the uniform LAT ray (rthx_device.h
lat_ray_fast<INSIDE, PLAIN>): a single axis-aligned rectangle whose four
coarse walls are solid, on a lattice in cell order, traces its rays without
the coarse wall index, the solid bit and lat_map (lat_plain).  The copy is
a set of kernel instances of its own; the launcher picks them from the host's
copy of the domain record, and rthx_debug_lat_plain returns that choice.

Every GPU case compares the device CSR (row_ptr, cols, counts) and the
lost-ray totals for exact equality with the CPU oracle on the same arguments:
every row, no tolerance.  The histogram path is forced as
tests/test_gpu_ray_body.py forces it.  A closed enclosure loses no ray, with
or without the scaled guess (RTHX_LAT_GUESS_SCALE: the guess only seeds an
exact search, so every scale gives the unscaled oracle's counts while a scale
off 1 sends rays through the cold continuation).

Shapes: a 3 x 2 lattice on a 0.3 x 0.7 rectangle, a 1 x 1 lattice (nx - 1 =
0), and the 5 x 5 unit square at kappa = 0.01 (nearly every ray a wall ray),
kappa = 0 (S = inf: every ray a wall ray) and kappa = 50 (nearly every ray a
gas ray).  Each shape has a twin with wall 1 (the right wall) open, which
takes the general copy: both copies run in this file.
"""
import ctypes as C
from unittest import mock

import numpy as np
import pytest

import helpers as H
from oracle import oracle
from rthx import PolyVolume2D, RayTracingDomain2D, domain, geometry

MAX_ROW = 8200  # rays a row on the oracle side
_ORACLE = {}
_DOMAINS = {}

# key: (W, H, nx, ny, kappa)
_SHAPES = {
    "rect32": (0.3, 0.7, 3, 2, 1.0),
    "one1": (1.0, 1.0, 1, 1, 1.0),
    "sq5_k001": (1.0, 1.0, 5, 5, 0.01),
    "sq5_k0": (1.0, 1.0, 5, 5, 0.0),
    "sq5_k50": (1.0, 1.0, 5, 5, 50.0),
}
CLOSED = tuple(_SHAPES)


def _mesh_quad_every_wall(volume, Nx, Ny):
    """mesh_quad, then every boundary wall of a cell takes the coarse wall's
    solid flag.  meshQuad marks a row's or column's far wall in an `elif` of
    the near wall's test, so with one cell along an axis the top and right
    walls of the enclosure are no surfaces and the rays that reach them are
    lost, in the oracle and on the device alike ("_meshed" below keeps that
    form).  A closed 1 x 1 enclosure needs all four."""
    geometry.mesh_quad(volume, Nx, Ny)
    for k, sub in enumerate(volume.subVolumes):
        n, m = k % Nx, k // Nx  # (cells x-fastest)
        on = [m == 0, n == Nx - 1, m == Ny - 1, n == 0]
        sub.solidWalls = [bool(volume.solidWalls[w]) and on[w] for w in range(4)]
    return volume


def _make(key):
    """The shape `key`, or with the suffix "_open" its twin with wall 1 open,
    or with "_meshed" the shape as meshQuad marks its walls."""
    W, Ht, nx, ny, kappa = _SHAPES[key.replace("_open", "").replace("_meshed", "")]
    solid = [True, not key.endswith("_open"), True, True]
    face = PolyVolume2D([(0.0, 0.0), (W, 0.0), (W, Ht), (0.0, Ht)], solid, 1, kappa, 0.0)
    face.T_in_w = [1000.0, 0.0, 0.0, 0.0]
    face.epsilon = [1.0] * 4
    face.T_in_g = -1.0
    face.q_in_g = 0.0
    if key.endswith("_meshed"):
        return RayTracingDomain2D([face], [(nx, ny)])
    with mock.patch.object(domain, "mesh_quad", _mesh_quad_every_wall):
        return RayTracingDomain2D([face], [(nx, ny)])


def _flat(key):
    if key not in _DOMAINS:
        _DOMAINS[key] = _make(key).flat()
    return _DOMAINS[key]


def _case(hip, key, R, seed):
    """(flat, args, oracle CSR, oracle info), computed once and left unchanged."""
    assert R <= MAX_ROW
    k = (key, R, seed)
    if k not in _ORACLE:
        flat = _flat(key)
        args, keep = hip.make_args(0, R, H.NUDGE, seed, 0, flat.n_emitters)
        rp, cols, cnt, info = oracle.trace_exchange(flat, args, 16)[:4]
        for a in (rp, cols, cnt):
            a.setflags(write=False)
        _ORACLE[k] = (flat, args, keep, (rp, cols, cnt), info)
    flat, args, _keep, want, info = _ORACLE[k]
    return flat, args, want, info


def _gpu(hip, flat, args, cuts=None):
    """CSR and info of one trace, or of the ray ranges [cuts[i], cuts[i+1])
    traced one by one (rthx_trace_exchange_rays) and accumulated."""
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


def _assert_csr(got, want):
    assert np.array_equal(got[0], want[0]), "row_ptr differs from the oracle"
    assert np.array_equal(got[1], want[1]), "cols differ from the oracle"
    assert np.array_equal(got[2], want[2]), "counts differ from the oracle"


def _assert_lost(info, oinfo, closed):
    for k in ("rays_traced", "lost_total", "lost_max_row"):
        assert info[k] == oinfo[k], (k, info[k], oinfo[k])
    if closed:
        assert info["lost_total"] == 0 and oinfo["lost_total"] == 0


def _histogram_path(monkeypatch, threads=None, split=False, scale=None):
    monkeypatch.setenv("RTHX_NO_SHORT_HASH", "1")
    if not split:
        monkeypatch.setenv("RTHX_SPLIT_BELOW", "1")
    if threads is not None:
        monkeypatch.setenv("RTHX_TRACE_THREADS", str(threads))
    if scale is not None:
        monkeypatch.setenv("RTHX_LAT_GUESS_SCALE", repr(scale))


def _lat_plain(hip, flat):
    """rthx_debug_lat_plain of the domain: 1, 0, or -1 without the lattice."""
    f = hip.load().rthx_debug_lat_plain
    f.argtypes = [C.c_void_p]
    f.restype = C.c_int
    dd = hip.DeviceDomain(flat, 0)
    try:
        return f(dd.handle)
    finally:
        dd.close()


# --------------------------------------------------------------------------
# the tie term on the CPU
# --------------------------------------------------------------------------
def test_x_wall_without_the_tie_order():
    """The closed-enclosure copy picks the coarse x wall by vx & (!vy | cx < cy)
    and defers a ray with cx == cy (rthx_device.h x_wall_untied).  Against
    the reference form vx & (!vy | (y_first & cx < cy) | (!y_first & !(cy <
    cx))) on 400 pairs of cross products, every fourth an exact tie, with
    every combination of vx, vy and y_first: off a tie the two agree, and
    every tie raises the flag."""
    from rthx import _lib

    f = _lib.load().rthx_debug_x_wall
    f.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_int32]
    f.restype = C.c_int
    rng = np.random.default_rng(20261021)
    cx = rng.random(400) * 10.0 ** rng.integers(-12, 3, 400)
    cy = rng.random(400) * 10.0 ** rng.integers(-12, 3, 400)
    cy[::4] = cx[::4]
    cy[1::8] = np.nextafter(cx[1::8], np.inf)  # (one ulp off a tie is no tie)
    n_tie = 0
    for a, b in zip(cx.tolist(), cy.tolist()):
        for vx in (0, 1):
            for vy in (0, 1):
                got = f(vx, vy, 0, a, b, 0)
                assert (got >> 1) == (1 if a == b else 0)
                n_tie += got >> 1
                for yf in (0, 1):
                    want = int(bool(vx) and (not vy or (bool(yf) and a < b) or (not yf and not (b < a))))
                    assert f(vx, vy, yf, a, b, 1) == want
                    if a != b:
                        assert (got & 1) == want, (vx, vy, yf, a, b)
    assert n_tie == 4 * 100
    # on a tie the reference form does depend on y_first, which is why the ray is deferred
    assert f(1, 1, 0, 0.25, 0.25, 1) == 1 and f(1, 1, 1, 0.25, 0.25, 1) == 0


# --------------------------------------------------------------------------
# the copy a domain takes
# --------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("key", CLOSED)
def test_copy_a_domain_takes(hip, key):
    """PLAIN for each closed shape, not PLAIN for its twin with wall 1 open.
    (The Python builders mesh a rectangle in cell order only -- mesh_quad from
    the first vertex, which the lattice needs at the lower left -- so no
    lattice out of cell order can be built here.)"""
    assert _lat_plain(hip, _flat(key)) == 1
    assert _lat_plain(hip, _flat(key + "_open")) == 0


# --------------------------------------------------------------------------
# exact counts
# --------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("threads", [256, 512])
@pytest.mark.parametrize("R", [1, 4, 257, 4099])
@pytest.mark.parametrize("key", CLOSED)
def test_closed_shapes(hip, monkeypatch, key, R, threads):
    """R = 4099: an edge round whose last group holds rays outside the range."""
    flat, args, want, oinfo = _case(hip, key, R, 300 + R % 97)
    _histogram_path(monkeypatch, threads)
    got, info = _gpu(hip, flat, args)
    _assert_csr(got, want)
    _assert_lost(info, oinfo, closed=True)


@pytest.mark.gpu
@pytest.mark.parametrize("key", CLOSED)
def test_open_twins(hip, monkeypatch, key):
    """The same shapes with wall 1 open: the general copy, lost rays counted."""
    flat, args, want, oinfo = _case(hip, key + "_open", 257, 300 + 257 % 97)
    if key != "sq5_k50":  # (at kappa = 50 few rays reach a wall at all)
        assert oinfo["lost_total"] > 0
    _histogram_path(monkeypatch, 256)
    got, info = _gpu(hip, flat, args)
    _assert_csr(got, want)
    _assert_lost(info, oinfo, closed=False)


@pytest.mark.gpu
@pytest.mark.parametrize("R", [4, 257])
def test_one_cell_as_meshed(hip, monkeypatch, R):
    """The 1 x 1 square as meshQuad marks it: four solid coarse walls (PLAIN),
    two of them no surfaces, so wall rays are lost at the fine wall."""
    flat, args, want, oinfo = _case(hip, "one1_meshed", R, 300 + R % 97)
    assert flat.n_surfaces == 2 and _lat_plain(hip, flat) == 1
    assert oinfo["lost_total"] > 0
    _histogram_path(monkeypatch, 256)
    got, info = _gpu(hip, flat, args)
    _assert_csr(got, want)
    _assert_lost(info, oinfo, closed=False)


@pytest.mark.gpu
def test_split_rows(hip, monkeypatch):
    """Every row split into parts: the slab hand-off sums the parts' tallies."""
    flat, args, want, oinfo = _case(hip, "rect32", 5003, 41)
    _histogram_path(monkeypatch, 256, split=True)
    got, info = _gpu(hip, flat, args)
    _assert_csr(got, want)
    _assert_lost(info, oinfo, closed=True)


@pytest.mark.gpu
def test_ray_base_not_zero(hip, monkeypatch):
    """Ray ranges [0, 1001) and [1001, 2052) accumulated: one trace of 2052
    rays.  The second range runs the instance that reads the ray base, which
    keeps segment_lat and has no PLAIN copy."""
    flat, args, want, oinfo = _case(hip, "sq5_k001", 2052, 43)
    _histogram_path(monkeypatch, 256)
    got, info = _gpu(hip, flat, args, cuts=(0, 1001, 2052))
    _assert_csr(got, want)
    assert info["lost_total"] == 0 and oinfo["lost_total"] == 0


# --------------------------------------------------------------------------
# the cold path
# --------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("R", [257, 2052])
@pytest.mark.parametrize("scale", [0.5, 1.03, 2.0])
@pytest.mark.parametrize("key", ["rect32", "sq5_k001", "sq5_k50"])
def test_cold_rays(hip, monkeypatch, key, scale, R):
    """1.03 leaves a few cold rays a row, which the row lists (at R = 257
    fewer than the list's 128 slots on every shape: at most a share
    (m - 1) |1 - 1/s| / 2 of the end points misses along an axis of m cells,
    0.12 of them for 5 x 5); 0.5 and 2.0 make most rays cold, at R = 2052 more than
    the list holds, and the whole row is traced again."""
    flat, args, want, oinfo = _case(hip, key, R, 47)
    _histogram_path(monkeypatch, 256, scale=scale)
    got, info = _gpu(hip, flat, args)
    _assert_csr(got, want)
    _assert_lost(info, oinfo, closed=True)


@pytest.mark.gpu
@pytest.mark.parametrize("scale,R", [(None, 257), (1.03, 257), (0.5, 2052)])
@pytest.mark.parametrize("key", ["rect32", "sq5_k001"])
def test_cold_rays_with_the_hash_tally(hip, monkeypatch, key, scale, R):
    """The hash-tally instances (RTHX_FORCE_HASH) compile the same list and
    the same reset: a few listed rays at 1.03, and at 0.5 the overflow, which
    zeroes the table and its bitmap before the row is traced again."""
    flat, args, want, oinfo = _case(hip, key, R, 47)
    monkeypatch.setenv("RTHX_FORCE_HASH", "1")
    monkeypatch.setenv("RTHX_SPLIT_BELOW", "1")
    monkeypatch.setenv("RTHX_TRACE_THREADS", "256")
    if scale is not None:
        monkeypatch.setenv("RTHX_LAT_GUESS_SCALE", repr(scale))
    got, info = _gpu(hip, flat, args)
    _assert_csr(got, want)
    _assert_lost(info, oinfo, closed=True)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [0.5, 1.03])
@pytest.mark.parametrize("key", ["rect32", "sq5_k001"])
def test_cold_rays_in_an_edge_round(hip, monkeypatch, key, scale):
    """R = 4099: the last round masks its rays by range while lanes are cold."""
    flat, args, want, oinfo = _case(hip, key, 4099, 300 + 4099 % 97)
    _histogram_path(monkeypatch, 256, scale=scale)
    got, info = _gpu(hip, flat, args)
    _assert_csr(got, want)
    _assert_lost(info, oinfo, closed=True)
