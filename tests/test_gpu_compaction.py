"""compact_row (rthx_kernels.hip): the LDS histogram of a row turned into its
CSR entries, at the shapes where its partition and its loops change.

Every case compares the device CSR (row_ptr, cols, counts) for exact equality
with the CPU oracle on the same arguments.  Square enclosures of ndim x ndim
cells have N = ndim^2 + 4 ndim absorbers and a packed histogram of
ceil(N / 2) words, shared among the 4, 8 or 16 waves of the workgroup
(RTHX_TRACE_THREADS) in runs of whole 64-word steps; a wave reads the steps
before its last unmasked and masks the last one:

  ndim   N      words
  3      21     11     most waves own an empty range
  8      96     48     under one step
  22     572    286    no multiple of 64, nor of 64 x waves
  31     1085   543    N odd: the last word's high half is no column
  45     2205   1103   N odd
  101    10605  5303   the benchmark's row: 21, 11 and 6 steps a wave at 256,
                       512 and 1024 lanes
  105    11445  5723   12 steps at 512 lanes, the last wave's range short
"""
import numpy as np
import pytest

import helpers as H
from oracle import oracle

pytestmark = pytest.mark.gpu

_ORACLE = {}


def _args(hip, flat, R, seed):
    return hip.make_args(0, R, H.NUDGE, seed, 0, flat.n_emitters, 1)


def _case(hip, key, make, R, seed):
    """(flat, args, oracle CSR) of a case, computed once and left unchanged."""
    if key not in _ORACLE:
        flat = make().flat()
        args, keep = _args(hip, flat, R, seed)
        rp, cols, cnt = oracle.trace_exchange(flat, args, 16)[:3]
        for a in (rp, cols, cnt):
            a.setflags(write=False)
        _ORACLE[key] = (flat, args, keep, (rp, cols, cnt))
    flat, args, _keep, want = _ORACLE[key]
    return flat, args, want


def _gpu_csr(hip, flat, args):
    dd = hip.DeviceDomain(flat, 0)
    res = hip.DeviceResult()
    try:
        res.trace(dd, args)
        info = res.info()
        rp, cols, cnt = res.csr()
        return rp.copy(), cols.copy(), cnt.copy(), info
    finally:
        res.close()
        dd.close()


def _assert_csr(got, want):
    assert np.array_equal(got[0], want[0]), "row_ptr differs from the oracle"
    assert np.array_equal(got[1], want[1]), "cols differ from the oracle"
    assert np.array_equal(got[2], want[2]), "counts differ from the oracle"


def _histogram_path(monkeypatch, threads=None, split=False):
    monkeypatch.setenv("RTHX_NO_SHORT_HASH", "1")
    if not split:
        monkeypatch.setenv("RTHX_SPLIT_BELOW", "1")
    if threads is not None:
        monkeypatch.setenv("RTHX_TRACE_THREADS", str(threads))


def _square(ndim, R):
    return ("square", ndim, R), (lambda: H.square_domain(ndim)), R, 100 + ndim


@pytest.mark.parametrize("threads", [256, 512, 1024])
@pytest.mark.parametrize("ndim", [3, 8, 22, 31, 45])
def test_unsplit_direct_csr(hip, monkeypatch, ndim, threads):
    """Unsplit rows written straight into the CSR (look-back), at every
    workgroup size."""
    flat, args, want = _case(hip, *_square(ndim, 1500))
    assert flat.n_emitters == ndim * ndim + 4 * ndim
    _histogram_path(monkeypatch, threads)
    got = _gpu_csr(hip, flat, args)
    assert got[3]["lookback_fallbacks"] == 0
    _assert_csr(got, want)


@pytest.mark.parametrize("ndim,threads", [(101, 256), (101, 512), (101, 1024), (105, 512)])
def test_long_shares(hip, monkeypatch, ndim, threads):
    """Shares of 21, 11, 6 and 12 steps: many unmasked steps before the masked
    last one, and rows of some 170 entries spread over all the waves."""
    flat, args, want = _case(hip, *_square(ndim, 200))
    _histogram_path(monkeypatch, threads)
    _assert_csr(_gpu_csr(hip, flat, args), want)


@pytest.mark.parametrize("threads", [256, 512, 1024])
def test_u32_tallies(hip, monkeypatch, threads):
    """R >= 65536: one u32 tally per word (PAIRS = false), 21 words."""
    flat, args, want = _case(hip, *_square(3, 70_000))
    _histogram_path(monkeypatch, threads)
    _assert_csr(_gpu_csr(hip, flat, args), want)


@pytest.mark.parametrize("threads", [256, 512, 1024])
def test_staging_slots(hip, monkeypatch, threads):
    """RTHX_NO_LOOKBACK: rows compacted into their staging slots (base 0)."""
    flat, args, want = _case(hip, *_square(22, 1500))
    _histogram_path(monkeypatch, threads)
    monkeypatch.setenv("RTHX_NO_LOOKBACK", "1")
    _assert_csr(_gpu_csr(hip, flat, args), want)


@pytest.mark.parametrize("threads", [256, 512, 1024])
def test_split_rows(hip, monkeypatch, threads):
    """Default splitting (572 rows of 5000 rays: several parts a row): the part
    that arrives last compacts the merged histogram."""
    flat, args, want = _case(hip, *_square(22, 5000))
    _histogram_path(monkeypatch, threads, split=True)
    _assert_csr(_gpu_csr(hip, flat, args), want)


@pytest.mark.parametrize("threads", [256, 512, 1024])
def test_cap_overflow_writes_nothing_and_retraces(hip, monkeypatch, threads):
    """RTHX_CSR_CAP=1000: the rows past the reservation write nothing, the
    library traces again, and the CSR is the one without the cap."""
    flat, args, want = _case(hip, *_square(22, 1500))
    _histogram_path(monkeypatch, threads)
    monkeypatch.setenv("RTHX_CSR_CAP", "1000")
    got = _gpu_csr(hip, flat, args)
    assert got[3]["lookback_fallbacks"] == 1
    _assert_csr(got, want)


def _all_open_square(ndim):
    """A transparent square (kappa = 0) with four open walls: every ray leaves."""
    face = H.PolyVolume2D([(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)], [False] * 4, 1, 0.0, 0.0)
    face.T_in_w = [0.0] * 4
    face.epsilon = [1.0] * 4
    face.T_in_g = -1.0
    face.q_in_g = 0.0
    return H.RayTracingDomain2D([face], [(ndim, ndim)])


@pytest.mark.parametrize("threads", [256, 512, 1024])
def test_every_ray_lost(hip, monkeypatch, threads):
    """No row has an entry: row_ptr is all zeros, cols and counts are empty."""
    flat, args, want = _case(hip, ("open", 22), lambda: _all_open_square(22), 1500, 7)
    assert not want[0].any() and want[1].size == 0
    _histogram_path(monkeypatch, threads)
    got = _gpu_csr(hip, flat, args)
    assert got[3]["nnz"] == 0 and got[3]["lost_total"] == flat.n_emitters * 1500
    _assert_csr(got, want)
