"""The uniform LAT ray's coarse wall (rthx_device.h lat_ray_fast: the wall the
ray points to, its bit of the coarse solid mask, and a lost ray where that wall
is open) for every choice of open walls, and the free-path logarithm's
high-word form (neg_log_u32).

A form of lat_ray_fast<true> that takes the wall's solid bit by mask logic,
without a wall index, was built against these cases and taken out again (it
measured slower, profiles/round16/INDEX.md); the cases stay, because the
existing suite opens one wall of one shape only.

Every GPU case compares the device CSR (row_ptr, cols, counts) and the lost-ray
totals with the CPU oracle on the same arguments: every row, no tolerance.  The
histogram path is forced as in test_gpu_ray_body.py.  Volume rows run
lat_ray_fast<true> and surface rows lat_ray_fast<false>, so every case covers
both.

Shapes: a 3 x 2 lattice on a 0.3 x 0.7 rectangle with each wall alone open,
two opposite walls open and all four open, the same with the lattice's first
guess scaled (cold lanes and an open wall in one ray), a 1 x 1 lattice
(nx - 1 = 0), R = 4099 (an edge round whose last group holds rays outside the
range) and the 5 x 5 unit square at kappa = 0.01 (nearly every ray is a wall
ray).

The host check holds neg_log_u32 to the bits the parent commit's library gave
(tests/golden/neg_log_u32_parent.json: the four edge words and the first 1000
of 10^5 random words in full, and a SHA-256 of every block of 1000 results).
"""
import ctypes as C
import hashlib

import numpy as np
import pytest

import helpers as H
from oracle import oracle
from rthx import PolyVolume2D, RayTracingDomain2D

_ORACLE = {}
_DOMAINS = {}

# walls: 0 bottom, 1 right, 2 top, 3 left (bit w of the coarse solid mask)
OPEN = {
    "open0": (0,), "open1": (1,), "open2": (2,), "open3": (3,),
    "open02": (0, 2), "open0123": (0, 1, 2, 3),
}


def _rect(W, Hh, nx, ny, kappa, open_walls=()):
    face = PolyVolume2D([(0.0, 0.0), (W, 0.0), (W, Hh), (0.0, Hh)], [w not in open_walls for w in range(4)], 1, kappa, 0.0)
    face.T_in_w = [1000.0, 0.0, 0.0, 0.0]
    face.epsilon = [1.0] * 4
    face.T_in_g = -1.0
    face.q_in_g = 0.0
    return RayTracingDomain2D([face], [(nx, ny)])


def _make(key):
    if key.startswith("open"):
        return _rect(0.3, 0.7, 3, 2, 1.0, OPEN[key])
    return {
        "one": lambda: _rect(0.3, 0.7, 1, 1, 1.0),
        "one_open1": lambda: _rect(0.3, 0.7, 1, 1, 1.0, (1,)),
        "thin5": lambda: _rect(1.0, 1.0, 5, 5, 0.01),
        "thin5_open3": lambda: _rect(1.0, 1.0, 5, 5, 0.01, (3,)),
    }[key]()


def _case(hip, key, R, seed):
    """(flat, args, oracle CSR, oracle info), computed once and left unchanged."""
    k = (key, R, seed)
    if k not in _ORACLE:
        if key not in _DOMAINS:
            _DOMAINS[key] = _make(key).flat()
        flat = _DOMAINS[key]
        args, keep = hip.make_args(0, R, H.NUDGE, seed, 0, flat.n_emitters)
        rp, cols, cnt, info = oracle.trace_exchange(flat, args, 16)[:4]
        for a in (rp, cols, cnt):
            a.setflags(write=False)
        _ORACLE[k] = (flat, args, keep, (rp, cols, cnt), info)
    flat, args, _keep, want, info = _ORACLE[k]
    return flat, args, want, info


def _gpu(hip, flat, args):
    dd = hip.DeviceDomain(flat, 0)
    res = hip.DeviceResult()
    try:
        res.trace(dd, args)
        rp, cols, cnt = res.csr()
        return (rp.copy(), cols.copy(), cnt.copy()), res.info()
    finally:
        res.close()
        dd.close()


def _check(hip, monkeypatch, key, R, seed, scale=None, lost=None):
    flat, args, want, oinfo = _case(hip, key, R, seed)
    share = oinfo["lost_total"] / oinfo["rays_traced"]
    print(f"{key} R={R}: oracle loses {oinfo['lost_total']} of {oinfo['rays_traced']} rays ({share:.3f})")
    if lost == "some":  # a case that loses no ray proves nothing about an open wall
        assert 0.05 <= share <= 0.95
    elif lost == "none":
        assert oinfo["lost_total"] == 0
    monkeypatch.setenv("RTHX_NO_SHORT_HASH", "1")
    monkeypatch.setenv("RTHX_SPLIT_BELOW", "1")
    monkeypatch.setenv("RTHX_TRACE_THREADS", "256")
    if scale is not None:
        monkeypatch.setenv("RTHX_LAT_GUESS_SCALE", repr(scale))
    got, info = _gpu(hip, flat, args)
    assert np.array_equal(got[0], want[0]), "row_ptr differs from the oracle"
    assert np.array_equal(got[1], want[1]), "cols differ from the oracle"
    assert np.array_equal(got[2], want[2]), "counts differ from the oracle"
    for k in ("rays_traced", "lost_total", "lost_max_row"):
        assert info[k] == oinfo[k], (k, info[k], oinfo[k])


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [None, 0.5, 2.0])
@pytest.mark.parametrize("key", sorted(OPEN))
def test_every_wall_open(hip, monkeypatch, key, scale):
    """One case per choice of open walls; with the guess scaled, cold lanes
    and an open wall meet in one ray."""
    _check(hip, monkeypatch, key, 2052, 41, scale=scale, lost="some")


@pytest.mark.gpu
@pytest.mark.parametrize("key,lost", [("one", None), ("one_open1", "some")])
def test_one_cell_lattice(hip, monkeypatch, key, lost):
    """Every wall ray ends in the only cell; the guess's clamp is nx - 1 = 0.
    (The mesher gives the single cell of a 1 x 1 mesh two solid fine walls, so
    the oracle loses rays here with every coarse wall solid, too.)"""
    _check(hip, monkeypatch, key, 2052, 43, lost=lost)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["open3", "open02"])
def test_edge_round(hip, monkeypatch, key):
    """R = 4099 on 256 lanes: four full rounds and one group whose last three
    rays lie outside the row's range."""
    _check(hip, monkeypatch, key, 4099, 47, lost="some")


@pytest.mark.gpu
@pytest.mark.parametrize("key,lost", [("thin5", "none"), ("thin5_open3", "some")])
def test_wall_rays_fill_the_wave(hip, monkeypatch, key, lost):
    """kappa = 0.01 on the unit square: the mean free path is 100 sides, so
    nearly every ray is a wall ray and the wall-lane block runs for full waves."""
    flat, _args, want, oinfo = _case(hip, key, 2052, 53)
    ns = flat.n_emitters - 25
    to_walls = int(want[2][want[1] < ns].astype(np.int64).sum())
    assert to_walls + oinfo["lost_total"] > 0.95 * oinfo["rays_traced"]
    _check(hip, monkeypatch, key, 2052, 53, lost=lost)


# --------------------------------------------------------------------------
# host: neg_log_u32 returns the parent's bits
# --------------------------------------------------------------------------
def _neg_log_words():
    rng = np.random.default_rng(20260116)
    return np.concatenate([np.array([0, 1, 2**31, 2**32 - 1], dtype=np.uint32),
                           rng.integers(0, 2**32, size=100_000, dtype=np.uint64).astype(np.uint32)])


def test_neg_log_u32_keeps_the_parents_bits():
    from rthx import _lib

    gold = H.golden("neg_log_u32_parent.json")
    f = _lib.load().rthx_debug_neg_log_u32
    f.argtypes = [C.POINTER(C.c_uint32), C.c_int64, C.POINTER(C.c_double)]
    w = _neg_log_words()
    assert w.size == gold["n"] and hashlib.sha256(w.tobytes()).hexdigest() == gold["words_sha256"]
    out = np.empty(w.size)
    assert f(w.ctypes.data_as(C.POINTER(C.c_uint32)), w.size, out.ctypes.data_as(C.POINTER(C.c_double))) == 0
    bits = out.view(np.uint64)
    head = np.array([int(x, 16) for x in gold["head_bits_hex"]], dtype=np.uint64)
    assert out[0] == np.inf
    assert np.array_equal(bits[:head.size], head)
    block = gold["block"]
    got = [hashlib.sha256(bits[k:k + block].tobytes()).hexdigest() for k in range(0, bits.size, block)]
    bad = [k for k, (a, b) in enumerate(zip(got, gold["block_sha256"])) if a != b]
    assert len(got) == len(gold["block_sha256"]) and not bad, f"blocks of {block} results that differ from the parent: {bad}"
