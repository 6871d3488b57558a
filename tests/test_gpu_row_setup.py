"""The per-row set-up of the trace kernels (rthx_kernels.hip): the row's
tally zeroed by 16-byte LDS stores -- a histogram through its padding to whole
uint4s, a hash table and its bitmap with a scalar tail -- and the row's ray
count added to s_tallied by lane 0 of the workgroup instead of a wave
reduction (the uniform LAT ray, whose lanes count only their lost rays).

Every case compares the device CSR (row_ptr, cols, counts) and rays_traced,
lost_total, lost_max_row for exact equality with the CPU oracle on the same
arguments: a word left unzeroed shows as a count that is too large or an
entry that should not be there, a wrong ray count as wrong lost-ray totals.

Shapes (N emitters, packed histogram words): the 5 x 5 square (45, 23: the
last uint4 holds one word of padding), a 7 x 3 rectangle (41, 21: three
words of padding), the 23 x 23 square (621, 311: more uint4s than the lanes
of a wave, one word of padding).  compact_row is not changed; the cases run
it at every workgroup size because the zeroing loop strides by it.
"""
import numpy as np
import pytest

import helpers as H
from oracle import oracle
from rthx import PolyVolume2D, RayTracingDomain2D

_ORACLE = {}
_DOMAINS = {}


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


_MAKE = {"square5": lambda: H.square_domain(5), "rect73": _rect73, "square23": lambda: H.square_domain(23),
         "open5": _open_square}
_N = {"square5": 45, "rect73": 41, "square23": 621, "open5": 40}


def _case(hip, key, R, seed):
    """(flat, args, oracle CSR, oracle info); the oracle runs once per (shape, R, seed)."""
    if key not in _DOMAINS:
        _DOMAINS[key] = _MAKE[key]().flat()
    flat = _DOMAINS[key]
    assert flat.n_emitters == _N[key]
    k = (key, R, seed)
    if k not in _ORACLE:
        args, keep = hip.make_args(0, R, H.NUDGE, seed, 0, flat.n_emitters)
        rp, cols, cnt, info = oracle.trace_exchange(flat, args, 16)[:4]
        for a in (rp, cols, cnt):
            a.setflags(write=False)
        _ORACLE[k] = ((args, keep), (rp, cols, cnt), info)
    args, want, info = _ORACLE[k]
    return flat, args, want, info


def _pins(monkeypatch, threads=None):
    monkeypatch.setenv("RTHX_NO_SHORT_HASH", "1")
    monkeypatch.setenv("RTHX_SPLIT_BELOW", "1")
    if threads is not None:
        monkeypatch.setenv("RTHX_TRACE_THREADS", str(threads))


def _gpu(hip, flat, args):
    dd = hip.DeviceDomain(flat, 0)
    res = hip.DeviceResult()
    try:
        res.trace(dd, args[0])
        rp, cols, cnt = res.csr()
        return (rp.copy(), cols.copy(), cnt.copy()), res.info()
    finally:
        res.close()
        dd.close()


def _assert_same(got, info, want, oinfo):
    assert np.array_equal(got[0], want[0]), "row_ptr differs from the oracle"
    assert np.array_equal(got[1], want[1]), "cols differ from the oracle"
    assert np.array_equal(got[2], want[2]), "counts differ from the oracle"
    for k in ("rays_traced", "lost_total", "lost_max_row"):
        assert info[k] == oinfo[k], (k, info[k], oinfo[k])


@pytest.mark.gpu
@pytest.mark.parametrize("R", [9, 64, 333])
@pytest.mark.parametrize("key", ["square5", "rect73", "square23"])
def test_direct_csr_rows(hip, monkeypatch, key, R):
    """Fewer rays than lanes (9), whole rounds (64) and edge rounds (333: not
    a multiple of four); rows written straight into the CSR by the look-back."""
    flat, args, want, oinfo = _case(hip, key, R, 900 + R)
    _pins(monkeypatch)
    got, info = _gpu(hip, flat, args)
    _assert_same(got, info, want, oinfo)
    assert info["lookback_fallbacks"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("threads", [256, 512, 1024])
def test_workgroup_sizes(hip, monkeypatch, threads):
    """78 uint4s zeroed by 256, 512 and 1024 lanes, and compacted by 4, 8 and
    16 waves."""
    flat, args, want, oinfo = _case(hip, "square23", 333, 900 + 333)
    _pins(monkeypatch, threads)
    got, info = _gpu(hip, flat, args)
    _assert_same(got, info, want, oinfo)


@pytest.mark.gpu
def test_u32_histogram(hip, monkeypatch):
    """65600 rays a row: the unpacked histogram (45 words, one counter a word)."""
    flat, args, want, oinfo = _case(hip, "square5", 65600, 17)
    _pins(monkeypatch)
    got, info = _gpu(hip, flat, args)
    _assert_same(got, info, want, oinfo)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["square5", "rect73", "open5"])
def test_hash_table_tail(hip, monkeypatch, key):
    """RTHX_FORCE_HASH=1: the row is a hash table and an N-bit bitmap, 2 x
    the table's slots + 2 bitmap words, so the zeroing ends with two words
    that no uint4 covers.  The open square's lanes also take lost rays off
    s_tallied."""
    R, seed = (2052, 29) if key == "open5" else (333, 900 + 333)
    flat, args, want, oinfo = _case(hip, key, R, seed)
    assert -(-flat.n_emitters // 32) % 4 == 2
    monkeypatch.setenv("RTHX_FORCE_HASH", "1")
    monkeypatch.setenv("RTHX_SPLIT_BELOW", "1")
    got, info = _gpu(hip, flat, args)
    _assert_same(got, info, want, oinfo)


@pytest.mark.gpu
def test_lost_rays_per_row(hip, monkeypatch):
    """An open wall: lane 0 adds the row's ray count to the lost rays'
    subtractions, so the lost-ray totals and every row's tallied count equal
    the oracle's."""
    flat, args, want, oinfo = _case(hip, "open5", 2052, 29)
    assert oinfo["lost_total"] > 0 and oinfo["lost_max_row"] > 0
    _pins(monkeypatch)
    got, info = _gpu(hip, flat, args)
    _assert_same(got, info, want, oinfo)


@pytest.mark.gpu
def test_stalled_rows_fall_back_to_staging(hip, monkeypatch):
    """RTHX_LB_WAIT_US=0: a row gives up its look-back as soon as a row below
    it is unpublished, the host traces the launch again on the staging path,
    and the counts still equal the oracle's."""
    flat, args, want, oinfo = _case(hip, "square23", 333, 900 + 333)
    _pins(monkeypatch)
    monkeypatch.setenv("RTHX_LB_WAIT_US", "0")
    fallbacks = 0
    for _ in range(3):  # (which row finishes first is not fixed: three launches, as tests/test_gpu_boundary.py)
        got, info = _gpu(hip, flat, args)
        _assert_same(got, info, want, oinfo)
        fallbacks += info["lookback_fallbacks"]
    assert fallbacks >= 1, "a zero wait bound never stalled"


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["square5", "square23"])
def test_staging_sequence(hip, monkeypatch, key):
    """RTHX_NO_LOOKBACK=1: the same rows compacted into staging slots."""
    flat, args, want, oinfo = _case(hip, key, 333, 900 + 333)
    _pins(monkeypatch)
    monkeypatch.setenv("RTHX_NO_LOOKBACK", "1")
    got, info = _gpu(hip, flat, args)
    _assert_same(got, info, want, oinfo)
