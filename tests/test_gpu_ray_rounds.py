"""The SINGLE trace kernels' ray loop (rthx_kernels.hip, `rounds`): group
rounds of four rays a lane, the partial last round, and the rounds that mask
their rays by range, at the ray counts where that indexing changes.

Every case compares the device CSR (row_ptr, cols, counts) for exact equality
with the CPU oracle on the same arguments: every row, no tolerance.  A row of
R rays is ceil(R / 4) groups; a workgroup of T lanes (RTHX_TRACE_THREADS)
traces them in ceil(groups / T) rounds.  With R = 4 (m T + L) - p a row has m
full rounds, L groups in the partial round (none when L = 0) and a last group
of 4 - p rays, so the last round masks by range when p > 0.  Split rows give
parts whose first ray is no multiple of four: their first round masks too.
"""
import numpy as np
import pytest

import helpers as H
from oracle import oracle
from rthx.domain import validate_extinction_uniformity

pytestmark = pytest.mark.gpu

MAX_ROW = 8200  # rays a row: the oracle side stays well under a second a case
_ORACLE = {}
_DOMAINS = {}


def _flat(key, make):
    if key not in _DOMAINS:
        _DOMAINS[key] = make().flat()
    return _DOMAINS[key]


def _case(hip, key, make, R, seed, flags=0, begin=0, stride=1):
    """(flat, args, oracle CSR) of a case, computed once and left unchanged."""
    k = (key, R, seed, flags, begin, stride)
    if k not in _ORACLE:
        flat = _flat(key, make)
        args, keep = hip.make_args(0, R, H.NUDGE, seed, begin, flat.n_emitters, stride, flags=flags)
        rp, cols, cnt = oracle.trace_exchange(flat, args, 16)[:3]
        for a in (rp, cols, cnt):
            a.setflags(write=False)
        _ORACLE[k] = (flat, args, keep, (rp, cols, cnt))
    flat, args, _keep, want = _ORACLE[k]
    return flat, args, want


def _gpu_csr(hip, flat, args):
    dd = hip.DeviceDomain(flat, 0)
    res = hip.DeviceResult()
    try:
        res.trace(dd, args)
        rp, cols, cnt = res.csr()
        return rp.copy(), cols.copy(), cnt.copy()
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


def _square(ndim):
    return ("square", ndim), (lambda: H.square_domain(ndim))


def _ray_counts(T):
    """The fixed list of R = 4 (m T + L) - p for T lanes, and the four
    smallest rows."""
    mlp = [
        # no full round: only the partial one
        (0, 1, 0), (0, 15, 1), (0, 16, 0), (0, 17, 3), (0, 63, 1), (0, 64, 0), (0, 65, 3), (0, T - 1, 0),
        # one full round; L = 0, p = 0: no partial round and no masked one
        (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 16, 3), (1, 64, 1), (1, 65, 0), (1, T - 1, 0),
        # two full rounds
        (2, 0, 0), (2, 0, 3), (2, 1, 1), (2, 17, 0), (2, T - 1, 1),
    ]
    rs = [1, 2, 3, 5] + [4 * (m * T + L) - p for m, L, p in mlp]
    rs = sorted({r for r in rs if r <= MAX_ROW})
    assert len(rs) <= 24
    return rs


_BOUNDARY = [(T, R) for T in (256, 512, 1024) for R in _ray_counts(T)]


def test_ray_count_list_covers_the_named_shapes():
    for T in (256, 512, 1024):
        rs = _ray_counts(T)
        assert 4 * T in rs  # L = 0, p = 0: no tail
        assert 4 * (T - 1) in rs  # L = T - 1: the partial round on all lanes but one
        assert 4 * 17 - 3 in rs and 4 * (T + 65) in rs  # the last round ends inside a wave
        assert {1, 2, 3, 5} <= set(rs)


@pytest.mark.parametrize("threads,R", _BOUNDARY)
def test_round_and_tail_boundaries(hip, monkeypatch, threads, R):
    """45 rows (20 surface and 25 volume emitters) of R rays, unsplit."""
    flat, args, want = _case(hip, *_square(5), R, 500 + R % 97)
    assert flat.n_emitters == 45
    _histogram_path(monkeypatch, threads)
    _assert_csr(_gpu_csr(hip, flat, args), want)


@pytest.mark.parametrize("R", [4999, 5000, 5003])
def test_split_parts_start_off_a_group(hip, monkeypatch, R):
    """Default splitting of 21 rows: parts [p chunk, (p + 1) chunk) whose
    first ray is no multiple of four, so a group is shared by two parts."""
    flat, args, want = _case(hip, *_square(3), R, 11)
    assert flat.n_emitters == 21
    _histogram_path(monkeypatch, split=True)
    _assert_csr(_gpu_csr(hip, flat, args), want)


@pytest.mark.parametrize("threads,R", [(256, 4 * 17 - 3), (512, 4 * (512 + 16) - 3)])
def test_faithful_sampling(hip, monkeypatch, threads, R):
    """RTHX_FLAG_FAITHFUL_SAMPLING: the any-emitter loop for volume rows too."""
    flat, args, want = _case(hip, *_square(5), R, 23, flags=hip.abi.RTHX_FLAG_FAITHFUL_SAMPLING)
    _histogram_path(monkeypatch, threads)
    _assert_csr(_gpu_csr(hip, flat, args), want)


def test_u32_tallies(hip, monkeypatch):
    """R = 70 000: the u32-tally instance of the loop (68 full rounds of 256
    lanes and a partial one)."""
    flat, args, want = _case(hip, *_square(3), 70_000, 103)
    _histogram_path(monkeypatch, 256)
    _assert_csr(_gpu_csr(hip, flat, args), want)


@pytest.mark.parametrize("R", [4 * (256 + 65), 4 * 15 - 1])
def test_strided_shard(hip, monkeypatch, R):
    """Rows 1, 4, 7, ... of the 45 (emitter_begin 1, emitter_stride 3)."""
    flat, args, want = _case(hip, *_square(5), R, 31, begin=1, stride=3)
    _histogram_path(monkeypatch, 256)
    got = _gpu_csr(hip, flat, args)
    assert len(got[0]) == len(want[0])
    _assert_csr(got, want)


def _checker_square(ndim):
    """One rectangle whose cells alternate between two extinction
    coefficients: the variable-beta lattice kernel (the start point is
    located too)."""
    dom = H.square_domain(ndim)
    for k, f in enumerate(dom.fine_mesh[0]):
        if k % 2:
            f.kappa_g = np.asarray(f.kappa_g) * 1.7
    fine_all = [f for sub in dom.fine_mesh for f in sub]
    dom.uniform_across_bin = validate_extinction_uniformity(fine_all, dom.n_spectral_bins)
    return dom


@pytest.mark.parametrize("threads,R", [(256, 4 * (256 + 17) - 3), (512, 4 * 65), (1024, 5)])
def test_variable_beta_rectangle(hip, monkeypatch, threads, R):
    flat, args, want = _case(hip, ("checker", 5), lambda: _checker_square(5), R, 41)
    assert flat.uniform_beta[0] < 0 and len(np.unique(flat.beta)) == 2
    _histogram_path(monkeypatch, threads)
    _assert_csr(_gpu_csr(hip, flat, args), want)
