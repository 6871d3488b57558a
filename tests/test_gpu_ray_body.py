"""The uniform LAT ray of the SINGLE trace kernels (rthx_device.h lat_ray_fast
/ lat_ray_fixup): the straight-line body, the cold lanes' continuation, the
lost-ray count that replaces the per-lane tally counter, and both in the
rounds that mask their rays by range.

Every GPU case compares the device CSR (row_ptr, cols, counts) for exact
equality with the CPU oracle on the same arguments: every row, no tolerance.
RTHX_LAT_GUESS_SCALE scales the lattice's first guess of a cell; the guess only
seeds an exact search, so every scale must give the unscaled oracle's counts,
while a scale off 1 sends rays through the continuation.

Shapes: the 5 x 5 unit square (45 emitters: 20 surface rows, which run the
any-emitter loop, and 25 volume rows, which run the rectangle loop) and a 7 x 3
lattice on a 0.3 x 0.7 rectangle (inexact spacing, extents no powers of two).
"""
import numpy as np
import pytest

import helpers as H
from oracle import oracle
from rthx import PolyVolume2D, RayTracingDomain2D

MAX_ROW = 8200  # rays a row on the oracle side
_ORACLE = {}
_DOMAINS = {}
SCALES = (0.5, 0.97, 1.03, 2.0)


def _rect73():
    return H.rect_domain(0.3, 0.7, 7, 3, 1.0, [1000.0, 0.0, 0.0, 0.0], [1.0] * 4)


def _open_square():
    """The 5 x 5 square with its right wall open: rays that reach it are lost."""
    face = PolyVolume2D([(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)], [True, False, True, True], 1, 1.0, 0.0)
    face.T_in_w = [1000.0, 0.0, 0.0, 0.0]
    face.epsilon = [1.0] * 4
    face.T_in_g = -1.0
    face.q_in_g = 0.0
    return RayTracingDomain2D([face], [(5, 5)])


_MAKE = {"square5": lambda: H.square_domain(5), "rect73": _rect73, "open5": _open_square}
_LATTICE = {"square5": (5, 5), "rect73": (7, 3), "open5": (5, 5)}


def _case(hip, key, R, seed):
    """(flat, args, oracle CSR, oracle info), computed once and left unchanged."""
    assert R <= MAX_ROW
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


def _assert_lost(info, oinfo):
    for k in ("rays_traced", "lost_total", "lost_max_row"):
        assert info[k] == oinfo[k], (k, info[k], oinfo[k])


def _histogram_path(monkeypatch, threads=None, split=False, scale=None):
    monkeypatch.setenv("RTHX_NO_SHORT_HASH", "1")
    if not split:
        monkeypatch.setenv("RTHX_SPLIT_BELOW", "1")
    if threads is not None:
        monkeypatch.setenv("RTHX_TRACE_THREADS", str(threads))
    if scale is not None:
        monkeypatch.setenv("RTHX_LAT_GUESS_SCALE", repr(scale))


# --------------------------------------------------------------------------
# the scaled guess on the CPU: the cases do exercise the continuation
# --------------------------------------------------------------------------
def _miss_share(nx, ny, scale, n=200_000, seed=7):
    """Share of uniform points of the box whose scaled first guess (the
    kernel's: truncate (x - x0) inv scale, clamp to [0, n - 1]) is not the
    cell that holds them; unit box, which the share does not depend on."""
    rng = np.random.default_rng(seed)
    miss = np.zeros(n, dtype=bool)
    for m in (nx, ny):
        x = rng.random(n)
        guess = np.clip(np.trunc(x * m * scale), 0, m - 1).astype(np.int64)
        miss |= guess != np.floor(x * m).astype(np.int64)
    return float(miss.mean())


@pytest.mark.parametrize("key", ["square5", "rect73"])
@pytest.mark.parametrize("scale", SCALES)
def test_scaled_guess_exercises_the_fixup(key, scale):
    """Scales 0.5 and 2.0 miss the cell for more than half of the end
    points.  Scales 0.97 and 1.03 cannot on these lattices: along an axis of m
    cells the guess floor(m s x) differs from floor(m x) on a share
    (m - 1) |1 - 1/s| / 2 of the points at most, 0.09 for m = 7, so about an
    eighth of the points miss -- the bound asserted for them is the one their
    purpose needs: a 64-lane wave runs the continuation when one lane misses,
    and more than half of the waves do."""
    p = _miss_share(*_LATTICE[key], scale)
    print(f"{key} scale {scale}: miss share {p:.4f}, waves with a miss {1 - (1 - p) ** 64:.4f}")
    assert _miss_share(*_LATTICE[key], 1.0) == 0.0
    if scale in (0.5, 2.0):
        assert p > 0.5
    else:
        assert p > 0.05 and 1 - (1 - p) ** 64 > 0.5


# --------------------------------------------------------------------------
# GPU cases
# --------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("threads", [256, 512])
@pytest.mark.parametrize("R", [1, 4, 257, 2052])
@pytest.mark.parametrize("key", ["square5", "rect73"])
def test_fast_path(hip, monkeypatch, key, R, threads):
    flat, args, want, oinfo = _case(hip, key, R, 700 + R % 89)
    _histogram_path(monkeypatch, threads)
    got, info = _gpu(hip, flat, args)
    _assert_csr(got, want)
    _assert_lost(info, oinfo)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("key", ["square5", "rect73"])
def test_fixup_on_most_rays(hip, monkeypatch, key, scale):
    """The upward walk (scale < 1), the downward walk and the n - 1 clamp
    (scale > 1); counts equal the unscaled oracle's."""
    flat, args, want, oinfo = _case(hip, key, 2052, 700 + 2052 % 89)
    _histogram_path(monkeypatch, 256, scale=scale)
    got, info = _gpu(hip, flat, args)
    _assert_csr(got, want)
    _assert_lost(info, oinfo)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [None, 0.5, 1.03])
@pytest.mark.parametrize("split", [False, True])
def test_lost_rays(hip, monkeypatch, split, scale):
    """An open wall: exact CSR and the oracle's lost-ray totals, unsplit and
    with every row split into parts (the slab hand-off sums the parts'
    tallied counts), with and without the continuation on most rays.  The 20
    surface rows run the any-emitter loop: their tallied totals too."""
    R = 5003 if split else 2052
    flat, args, want, oinfo = _case(hip, "open5", R, 29)
    assert oinfo["lost_total"] > 0 and oinfo["lost_max_row"] > 0
    _histogram_path(monkeypatch, 256, split=split, scale=scale)
    got, info = _gpu(hip, flat, args)
    _assert_csr(got, want)
    _assert_lost(info, oinfo)
    tallied = np.add.reduceat(got[2].astype(np.int64), got[0][:-1])
    otallied = np.add.reduceat(want[2].astype(np.int64), want[0][:-1])
    assert np.array_equal(tallied[:20], otallied[:20]) and np.all(tallied[:20] < R)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [0.5, 1.03])
@pytest.mark.parametrize("key", ["square5", "rect73", "open5"])
def test_edge_rounds_with_cold_lanes(hip, monkeypatch, key, scale):
    """R = 4 (T + 17) - 3: the last round masks its rays by range while its
    lanes run the continuation."""
    T = 256
    flat, args, want, oinfo = _case(hip, key, 4 * (T + 17) - 3, 53)
    _histogram_path(monkeypatch, T, scale=scale)
    got, info = _gpu(hip, flat, args)
    _assert_csr(got, want)
    _assert_lost(info, oinfo)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [None, 0.97, 2.0])
@pytest.mark.parametrize("key", ["square5", "open5"])
def test_ray_base_off_a_group(hip, monkeypatch, key, scale):
    """Ray ranges [0, 1001) and [1001, 2052) through rthx_trace_exchange_rays,
    accumulated: one trace of 2052 rays.  The first range ends off a group
    (its last round masks by range, on the straight-line body); the second
    runs the instance that reads the ray base, which keeps segment_lat and
    reads the scaled guess through lattice_index, first round masked."""
    seed = 29 if key == "open5" else 700 + 2052 % 89
    flat, args, want, oinfo = _case(hip, key, 2052, seed)
    _histogram_path(monkeypatch, 256, scale=scale)
    got, info = _gpu(hip, flat, args, cuts=(0, 1001, 2052))
    _assert_csr(got, want)
    assert info["lost_total"] == oinfo["lost_total"]
