"""Progressive traces on the GPU: ray ranges (rthx_trace_exchange_rays), the
count-matrix sum (rthx_result_accumulate, rthx_result_accumulate_csr), the
sampling error (rthx_result_sampling_error) and what is built on them
(rthx.progressive, rthx.distributed.trace_ray_sharded).

Counts are compared exactly: a ray is a pure function of (seed, bin, emitter,
ray id), so ranges of one seed folded together are one trace of their union,
and that trace equals the CPU oracle.  Tolerances appear only where stated.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import helpers as H
from oracle import oracle
from rthx.distributed import accumulate_csr_host, trace_ray_sharded
from test_accumulate_host import accumulate_cases, csr_of_dense, dense_of, random_csr

pytestmark = pytest.mark.gpu

R3 = 4099  # no multiple of 4, cut where no cut is one
CUTS3 = (0, 1001, 2003, R3)
INFO_KEYS = ("rays_per_emitter", "rays_traced", "rows_traced", "nnz", "lost_total", "lost_max_row")


def _ranged(hip, dd, flat, b, e, seed=1, flags=0, begin=0, end=None, stride=1, res=None, rec=None):
    """Ray ids [b, e) of the selected rows into a (new) DeviceResult."""
    args, keep = hip.make_args(0, e - b, H.NUDGE, seed, begin, flat.n_emitters if end is None else end, stride,
                               flags=flags, record_ids=rec)
    res = hip.DeviceResult() if res is None else res
    res.trace(dd, args, ray_begin=b)
    del keep
    return res


def _snapshot(res):
    rp, c, v = res.csr()
    return rp.copy(), c.copy(), v.copy(), res.info()


def _assert_same(got, want, what):
    for k, name in enumerate(("row_ptr", "cols", "counts")):
        assert np.array_equal(got[k], want[k]), f"{what}: {name} differ"
    for k in INFO_KEYS:
        assert got[3][k] == want[3][k], (what, k, got[3][k], want[3][k])


def _fold(hip, dd, flat, cuts, order=None, **kw):
    """The ranges [cuts[i], cuts[i+1]) traced one by one and accumulated in `order`."""
    order = range(len(cuts) - 1) if order is None else order
    acc, scratch = None, hip.DeviceResult()
    try:
        for i in order:
            b, e = cuts[i], cuts[i + 1]
            if acc is None:
                acc = _ranged(hip, dd, flat, b, e, **kw)
                assert acc.info()["rays_per_emitter"] == e - b
            else:
                _ranged(hip, dd, flat, b, e, res=scratch, **kw)
                assert scratch.info()["rays_per_emitter"] == e - b
                acc.accumulate(scratch)
        return acc
    finally:
        scratch.close()


def _layers():
    return H.layered_slab_domain([0.3, 1.1, 0.6, 2.0], W=4.0, nx=5)


# name: (domain, env knobs, trace keywords, (R, cuts))
_FAMILIES = {
    "lat": (lambda: H.square_domain(11), {}, {}, None),
    "single_not_axis": (lambda: H.square_domain(5, rotation=0.3), {}, {}, None),
    "clds": (lambda: H.wedge_domain(16, 2), {}, {}, None),
    "generic": (lambda: H.wedge_domain(16, 2), {"RTHX_NO_CLDS": "1"}, {}, None),
    "mlat": (lambda: H.quad_lattice_domain(), {}, {}, None),
    "walk_layers": (_layers, {}, {}, None),
    "faithful": (lambda: H.square_domain(11), {}, {"flags": 1}, None),
    "strided": (lambda: H.square_domain(5), {}, {"begin": 1, "stride": 3}, None),
    "histogram": (lambda: H.square_domain(5), {"RTHX_NO_SHORT_HASH": "1", "RTHX_SPLIT_BELOW": "1"}, {}, None),
    "threads512": (lambda: H.square_domain(5), {"RTHX_NO_SHORT_HASH": "1", "RTHX_SPLIT_BELOW": "1",
                                                "RTHX_TRACE_THREADS": "512"}, {}, None),
    "hash": (lambda: H.square_domain(5), {"RTHX_FORCE_HASH": "1"}, {}, None),
    # three rows of >= 4096 rays a range: plan_trace splits every row (slab hand-off / sorted part lists)
    "split_histogram": (lambda: H.square_domain(11), {"RTHX_NO_SHORT_HASH": "1"}, {"end": 3},
                        (12301, (0, 4099, 8201, 12301))),
    "split_hash": (lambda: H.square_domain(11), {"RTHX_FORCE_HASH": "1", "RTHX_HASH_MAX": "2048"}, {"end": 3},
                   (12301, (0, 4099, 8201, 12301))),
}


@pytest.mark.parametrize("family", list(_FAMILIES))
def test_ranges_fold_to_one_trace(hip, monkeypatch, family):
    """Three ranges, cut off the groups of four, folded with
    rthx_result_accumulate = one trace of R = the CPU oracle at R."""
    make, env, kw, shape = _FAMILIES[family]
    R, cuts = shape if shape else (R3, CUTS3)
    assert all(c % 4 for c in cuts[1:])
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    flat = make().flat()
    if family == "walk_layers":
        assert flat.uniform_beta[0] < 0
    dd = hip.DeviceDomain(flat, 0)
    one = acc = None
    try:
        one = _ranged(hip, dd, flat, 0, R, **kw)
        want = _snapshot(one)
        oargs, _k = hip.make_args(0, R, H.NUDGE, 1, kw.get("begin", 0), kw.get("end", flat.n_emitters),
                                  kw.get("stride", 1), flags=kw.get("flags", 0))
        orp, ocols, ocnt = oracle.trace_exchange(flat, oargs, 16)[:3]
        assert np.array_equal(want[0], orp) and np.array_equal(want[1], ocols) and np.array_equal(want[2], ocnt)
        acc = _fold(hip, dd, flat, cuts, **kw)
        _assert_same(_snapshot(acc), want, family)
    finally:
        for r in (one, acc):
            if r is not None:
                r.close()
        dd.close()


def test_fold_order_and_seeds(hip):
    flat = H.square_domain(11).flat()
    dd = hip.DeviceDomain(flat, 0)
    res = []
    try:
        a = _fold(hip, dd, flat, CUTS3)
        b = _fold(hip, dd, flat, CUTS3, order=(2, 0, 1))
        res += [a, b]
        _assert_same(_snapshot(b), _snapshot(a), "another order")
        # two seeds: the host sum of their CSRs
        s1 = _ranged(hip, dd, flat, 0, 1500, seed=11)
        s2 = _ranged(hip, dd, flat, 0, 2001, seed=12)
        res += [s1, s2]
        h1, h2 = _snapshot(s1), _snapshot(s2)
        s1.accumulate(s2)
        got = _snapshot(s1)
        want = accumulate_csr_host(h1[:3], h2[:3], flat.n_emitters)
        for k in range(3):
            assert np.array_equal(got[k], want[k])
        assert got[3]["rays_per_emitter"] == 3501 and got[3]["lost_total"] == h1[3]["lost_total"] + h2[3]["lost_total"]
        # (the source is left as it was)
        _assert_same(_snapshot(s2), h2, "source")
    finally:
        for r in res:
            r.close()
        dd.close()


def test_mismatched_results_rejected(hip):
    flat = H.square_domain(5).flat()
    dd = hip.DeviceDomain(flat, 0)
    a = _ranged(hip, dd, flat, 0, 100)
    b = _ranged(hip, dd, flat, 100, 200, begin=1, stride=3)
    c = _ranged(hip, dd, flat, 100, 200, end=7)
    try:
        for other in (b, c):
            with pytest.raises(hip.RthxError, match="rthx error -1"):
                a.accumulate(other)
    finally:
        for r in (a, b, c):
            r.close()
        dd.close()


def test_recorded_rays_of_a_range(hip):
    """A ranged trace records the rays of its range, in ray order: per
    recorded emitter the three ranges' rays, concatenated, are the one-shot
    trace's."""
    flat = H.wedge_domain(8, 3).flat()
    ids = [0, 5, 17]
    R, cuts = 1003, (0, 333, 701, 1003)
    dd = hip.DeviceDomain(flat, 0)
    try:
        one = _ranged(hip, dd, flat, 0, R, seed=7, rec=ids)
        o1, e1, g1 = one.rays()
        one.close()
        parts = []
        for b, e in zip(cuts[:-1], cuts[1:]):
            r = _ranged(hip, dd, flat, b, e, seed=7, rec=ids)
            parts.append(r.rays())
            r.close()
    finally:
        dd.close()
    assert sum(len(p[2]) for p in parts) == len(g1) > 0
    for g in ids:
        o = np.concatenate([p[0][p[2] == g] for p in parts])
        e = np.concatenate([p[1][p[2] == g] for p in parts])
        assert np.array_equal(o, o1[g1 == g]) and np.array_equal(e, e1[g1 == g])


# ---- rthx_result_accumulate_csr on synthetic blocks ----

@pytest.fixture(scope="module")
def wide_domain(hip):
    """N = 4352 columns: rows longer than a 256-lane tile and than 4096 entries."""
    flat = H.square_domain(64).flat()
    assert flat.n_emitters == 4352
    dd = hip.DeviceDomain(flat, 0)
    yield flat, dd
    dd.close()


def _long_row_cases():
    rng = np.random.default_rng(77)
    n = 4352
    # a workgroup per row (mean row length >= 512): full rows, rows that end inside a tile, an empty one
    a = random_csr(rng, 6, n, 0.55, max_count=200, full_rows={0, 3}, empty_rows={5})
    b = random_csr(rng, 6, n, 0.5, max_count=200, full_rows={3, 4}, empty_rows={1})
    # a wave per row: short rows around one row of all 4352 columns
    c = random_csr(rng, 40, n, 0.004, max_count=50, full_rows={7})
    d = random_csr(rng, 40, n, 0.006, max_count=50, full_rows={7}, empty_rows={0, 39})
    # tile edges: 255 / 256 / 257 and 63 / 64 / 65 columns against a full row
    D = np.zeros((7, n), dtype=np.uint64)
    E = np.zeros((7, n), dtype=np.uint64)
    for r, k in enumerate((63, 64, 65, 255, 256, 257, 4097)):
        D[r, rng.choice(n, size=k, replace=False)] = 3
        E[r, :] = 1 + r
    return [("wide", a, b, 6, n), ("narrow_with_long_row", c, d, 40, n),
            ("tile_edges", csr_of_dense(D), csr_of_dense(E), 7, n)]


def _to_dev(csr, torch):
    rp, c, v = csr
    dev = torch.device("cuda", 0)
    return (torch.from_numpy(np.ascontiguousarray(rp)).to(dev), torch.from_numpy(np.ascontiguousarray(c)).to(dev),
            torch.from_numpy(np.ascontiguousarray(v).view(np.int32)).to(dev))


@pytest.mark.parametrize("case", accumulate_cases() + _long_row_cases(), ids=lambda c: c[0])
def test_accumulate_csr_blocks(hip, wide_domain, case):
    """Two synthetic blocks added to an empty result equal the host sum."""
    import torch

    _name, a, b, rows, n = case
    flat, dd = wide_domain
    res = _ranged(hip, dd, flat, 0, 0, end=rows)  # no rays: `rows` empty rows
    try:
        assert res.info()["rows_traced"] == rows and res.info()["nnz"] == 0
        Da, Db = dense_of(a, rows, n), dense_of(b, rows, n)
        Ra = int(Da.sum(axis=1).max()) + 5 if rows else 5
        Rb = int(Db.sum(axis=1).max()) if rows else 0
        res.accumulate_csr(*_to_dev(a, torch), Ra)
        res.accumulate_csr(*_to_dev(b, torch), Rb)
        rp, c, v = res.csr()
        want = accumulate_csr_host(a, b, n)
        assert np.array_equal(rp[:rows + 1], want[0]) and np.all(rp[rows:] == want[0][-1])
        assert np.array_equal(c, want[1]) and np.array_equal(v, want[2])
        info = res.info()
        lost = (Ra + Rb) - (Da + Db).sum(axis=1).astype(np.int64)
        assert info["rays_per_emitter"] == Ra + Rb and info["nnz"] == len(want[1])
        assert info["lost_total"] == int(lost.sum()) and info["lost_max_row"] == (int(lost.max()) if rows else 0)
        assert res.accumulate_ms() >= 0.0
    finally:
        res.close()


def test_accumulate_csr_rejects_other_shapes(hip, wide_domain):
    import torch

    flat, dd = wide_domain
    rng = np.random.default_rng(9)
    res = _ranged(hip, dd, flat, 0, 0, end=6)
    try:
        with pytest.raises(hip.RthxError, match="rthx error -1"):  # 5 rows into 6
            res.accumulate_csr(*_to_dev(random_csr(rng, 5, 40, 0.3), torch), 10)
        bad = random_csr(rng, 6, 40, 0.3)
        bad[1][0] = flat.n_emitters  # a column >= N
        with pytest.raises(hip.RthxError, match="rthx error -1"):
            res.accumulate_csr(*_to_dev(bad, torch), 10)
        assert res.info()["nnz"] == 0 and res.info()["rays_per_emitter"] == 0  # (left as it was)
        with pytest.raises(hip.RthxError, match="rthx error -4"):  # summed rays >= 2^32
            res.accumulate_csr(*_to_dev(random_csr(rng, 6, 40, 0.3), torch), 2 ** 32)
    finally:
        res.close()


# ---- readers of an accumulated result ----

@pytest.fixture(scope="module")
def square_pair(hip):
    """square_domain(11): one trace of 4099 rays and the three folded ranges."""
    dom = H.square_domain(11)
    flat = dom.flat()
    dd = hip.DeviceDomain(flat, 0)
    one = _ranged(hip, dd, flat, 0, R3)
    acc = _fold(hip, dd, flat, CUTS3)
    yield dom, flat, one, acc
    one.close()
    acc.close()
    dd.close()


def test_readers_after_accumulate(hip, square_pair):
    from rthx.smoothing import get_w, smooth_F_device

    dom, flat, one, acc = square_pair
    n = flat.n_emitters
    rp, c, v = acc.csr()
    frp, fc, fv = acc.F()
    rows = np.repeat(np.arange(n), np.diff(rp))
    tallied = np.bincount(rows, weights=v, minlength=n)[rows]  # (exact: integers below 2^53)
    assert np.array_equal(frp, rp) and np.array_equal(fc, c)
    # one fp64 division each: 1e-15 relative, as test_gpu_boundary holds rthx_result_copy_F
    assert np.allclose(fv, v / tallied, rtol=1e-15, atol=0.0)
    colptr, rowval, nz = acc.F_csc()
    F = sp.csr_matrix((fv, fc, frp), shape=(n, n))
    Fc = sp.csc_matrix((nz, rowval, colptr), shape=(n, n))
    assert (F != Fc.tocsr()).nnz == 0
    ro, pairs, d = acc.torch_csr()
    assert d["nnz"] == len(c) and np.array_equal(pairs[0].cpu().numpy(), c)
    assert np.array_equal(pairs[1].cpu().numpy().view(np.uint32), v) and np.array_equal(ro.cpu().numpy(), rp)
    # smoothing: the same counts, so the same F_smooth (test_gpu_smooth's 1e-12)
    w = get_w(dom)
    sa = smooth_F_device(acc, n, w, dom.num_surfaces, verbose=False)
    so_ = smooth_F_device(one, n, w, dom.num_surfaces, verbose=False)
    try:
        A, B = sa.host(), so_.host()
        A = A.toarray() if sp.issparse(A) else A
        B = B.toarray() if sp.issparse(B) else B
        assert np.abs(A - B).max() <= 1e-12
    finally:
        sa.close()
        so_.close()


def _sampling_error_host(rp, v, n_rows, n):
    s = np.zeros(n_rows)
    for i in range(n_rows):
        c = v[rp[i]:rp[i + 1]].astype(np.float64)
        t = c.sum()
        if t > 0:
            p = c / t
            s[i] = (1.0 - np.sum(p * p)) / t
    return float(np.sqrt(s.sum() / (n_rows * n))), float(np.sqrt(s.max()))


def test_sampling_error_formula(hip, square_pair):
    """Against numpy from the host CSR, relative 1e-10 (at most 165^2 positive
    fp64 terms, whose order moves the sums by far less)."""
    _dom, flat, one, acc = square_pair
    n = flat.n_emitters
    for res in (one, acc):
        rp, _c, v = res.csr()
        rms, mx = res.sampling_error()
        wr, wm = _sampling_error_host(rp, v, n, n)
        assert rms > 0 and abs(rms - wr) <= 1e-10 * wr and abs(mx - wm) <= 1e-10 * wm
    assert one.sampling_error() == acc.sampling_error()


def test_sampling_error_falls_as_root_of_rays(hip):
    """R = 4096 extended to 8192: the rms falls by sqrt(2) within 5 % (the
    binomial formula with nearly stable p).  Observed when first run on an
    MI355X: rms ratio 1.414096 (max_row ratio 1.413947), 0.008 % off sqrt(2)."""
    from rthx.progressive import ProgressiveTrace

    with ProgressiveTrace(H.square_domain(11)) as t:
        t.extend(4096)
        r1, m1 = t.sampling_error()
        t.extend(4096)
        r2, m2 = t.sampling_error()
        assert t.rays_per_emitter == 8192 and t.info()["rays_per_emitter"] == 8192
    ratio = r1 / r2
    print(f"rms ratio 4096 -> 8192: {ratio:.6f} (sqrt 2 = {np.sqrt(2):.6f}); max_row ratio {m1 / m2:.6f}")
    assert abs(ratio / np.sqrt(2) - 1) <= 0.05, ratio


def test_progressive_trace_equals_one_shot(hip, square_pair):
    from rthx.progressive import ProgressiveTrace

    dom, _flat, one, _acc = square_pair
    with ProgressiveTrace(dom) as t:
        for r in (1001, 1002, 2096):
            t.extend(r)
        assert t.rays_per_emitter == R3
        rp, c, v = t.csr()
        want = _snapshot(one)
        assert np.array_equal(rp, want[0]) and np.array_equal(c, want[1]) and np.array_equal(v, want[2])
        assert t.F()[2].shape == v.shape and t.device_result.info()["nnz"] == want[3]["nnz"]


def test_trace_to_tolerance(hip):
    from rthx.progressive import trace_to_tolerance

    dom = H.square_domain(5)
    # no tolerance to reach: batches up to the cap, the last one cut to it
    t, hist = trace_to_tolerance(dom, 0.0, 300, 1000)
    t.close()
    assert [h[0] for h in hist] == [300, 600, 900, 1000]
    assert all(a[1] > b[1] for a, b in zip(hist, hist[1:]))
    # the same batches (same seed, same ranges): stops at the first one at or under the tolerance
    t, hist2 = trace_to_tolerance(dom, hist[1][1], 300, 1000)
    try:
        assert hist2 == hist[:2] and t.rays_per_emitter == 600
        assert hist2[-1][1] <= hist[1][1] < hist2[0][1]
    finally:
        t.close()


# ---- ray-sharded traces, emulated on one GPU ----

@pytest.mark.parametrize("domain", ["square", "wedge"])
@pytest.mark.parametrize("world,R", [(2, 4099), (3, 4099), (8, 4099), (8, 29)])
def test_ray_sharded_emulation_equals_one_shot(hip, domain, world, R):
    """Every rank traces all rows over its share of the ray ids (R = 29 < 4 W:
    shares of 3 and 4 rays); the owner's fold is the one-shot trace."""
    dom = H.square_domain(11) if domain == "square" else H.wedge_domain(16, 2)
    flat = dom.flat()
    dd = hip.device_domain(dom, 0)
    one = _ranged(hip, dd, flat, 0, R)
    res = None
    try:
        res = trace_ray_sharded(dom, R, world, dst=world - 1 if world == 3 else 0)
        _assert_same(_snapshot(res), _snapshot(one), f"W = {world}")
    finally:
        one.close()
        if res is not None:
            res.close()


def test_3d_results_accumulate(hip):
    """Two rthx_trace_exchange_3d results of different seeds sum to their host sum."""
    from rthx.trace3d import Scene3D

    xyz, nv, nrm, g, _nh = H.box_scene([np.linspace(0, 1, 3)] * 3)
    s = Scene3D(xyz, nv, nrm, groups=g)
    a = b = None
    try:
        a = s.trace_result(700, seed=3)
        b = s.trace_result(901, seed=4)
        ha, hb = _snapshot(a), _snapshot(b)
        a.accumulate(b)
        got = _snapshot(a)
        want = accumulate_csr_host(ha[:3], hb[:3], s.n)
        for k in range(3):
            assert np.array_equal(got[k], want[k])
        assert got[3]["rays_per_emitter"] == 1601
        assert got[3]["lost_total"] == ha[3]["lost_total"] + hb[3]["lost_total"]
    finally:
        for r in (a, b):
            if r is not None:
                r.close()
        s.close()
