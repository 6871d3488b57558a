"""Progressive traces without a GPU: the numpy reference of the count-matrix
sum (rthx.distributed.accumulate_csr_host) against a dense sum, the argument
checks of rthx_trace_exchange_rays / rthx_result_accumulate* /
rthx_result_sampling_error that need no device, and the ray-shard split.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers as H
from rthx import abi, _lib
from rthx.direct import ray_shard
from rthx.distributed import accumulate_csr_host, fold_ray_shards_host


def random_csr(rng, rows, n, density, max_count=1000, full_rows=(), empty_rows=()):
    """A count CSR with column-ascending rows; `full_rows` hold all of 0..n-1."""
    rp = [0]
    cols, cnt = [], []
    for r in range(rows):
        if r in empty_rows:
            c = np.zeros(0, dtype=np.int64)
        elif r in full_rows:
            c = np.arange(n)
        else:
            c = np.nonzero(rng.random(n) < density)[0]
        cols.append(c)
        cnt.append(rng.integers(1, max_count, size=len(c)))
        rp.append(rp[-1] + len(c))
    return (np.asarray(rp, dtype=np.int64), np.concatenate(cols).astype(np.int32) if rows else np.zeros(0, np.int32),
            np.concatenate(cnt).astype(np.uint32) if rows else np.zeros(0, np.uint32))


def dense_of(csr, rows, n):
    rp, c, v = csr
    out = np.zeros((rows, n), dtype=np.uint64)
    for r in range(rows):
        out[r, c[rp[r]:rp[r + 1]]] = v[rp[r]:rp[r + 1]]
    return out


def csr_of_dense(D):
    rows, _n = D.shape
    rp = np.zeros(rows + 1, dtype=np.int64)
    nz = D != 0
    np.cumsum(nz.sum(axis=1), out=rp[1:])
    r, c = np.nonzero(nz)
    return rp, c.astype(np.int32), D[r, c].astype(np.uint32)


def accumulate_cases():
    """(name, a, b, rows, n): the pairs the device test covers too."""
    rng = np.random.default_rng(20251019)
    out = []
    a = random_csr(rng, 9, 37, 0.3, empty_rows={0, 4})
    b = random_csr(rng, 9, 37, 0.4, empty_rows={0, 5})  # row 0 empty in both, 4 and 5 on one side
    out.append(("empty_rows", a, b, 9, 37))
    a = random_csr(rng, 6, 50, 0.5)
    b = (a[0].copy(), a[1].copy(), rng.integers(1, 99, size=len(a[1])).astype(np.uint32))
    out.append(("identical_columns", a, b, 6, 50))
    D = np.zeros((5, 40), dtype=np.uint64)
    E = np.zeros((5, 40), dtype=np.uint64)
    D[:, 0::2] = rng.integers(1, 9, size=(5, 20))
    E[:, 1::2] = rng.integers(1, 9, size=(5, 20))
    out.append(("disjoint_columns", csr_of_dense(D), csr_of_dense(E), 5, 40))
    a = random_csr(rng, 4, 70, 0.2, full_rows={1})
    b = random_csr(rng, 4, 70, 0.2, full_rows={1, 2})
    out.append(("full_row", a, b, 4, 70))
    z = (np.zeros(1, dtype=np.int64), np.zeros(0, np.int32), np.zeros(0, np.uint32))
    out.append(("no_rows", z, z, 0, 11))
    return out


@pytest.mark.parametrize("case", accumulate_cases(), ids=lambda c: c[0])
def test_accumulate_csr_host_equals_dense_sum(case):
    _name, a, b, rows, n = case
    rp, c, v = accumulate_csr_host(a, b, n)
    want = csr_of_dense(dense_of(a, rows, n) + dense_of(b, rows, n)) if rows else a
    assert rp.dtype == np.int64 and c.dtype == np.int32 and v.dtype == np.uint32
    assert np.array_equal(rp, want[0]) and np.array_equal(c, want[1]) and np.array_equal(v, want[2])
    for r in range(rows):  # column-ascending rows
        assert np.all(np.diff(c[rp[r]:rp[r + 1]]) > 0)


def test_accumulate_csr_host_rejects_bad_blocks():
    rng = np.random.default_rng(3)
    a = random_csr(rng, 4, 10, 0.5)
    b = random_csr(rng, 5, 10, 0.5)
    with pytest.raises(ValueError):
        accumulate_csr_host(a, b, 10)
    with pytest.raises(ValueError):
        accumulate_csr_host(a, a, 5)  # columns >= n
    big = (np.array([0, 1], dtype=np.int64), np.array([2], dtype=np.int32), np.array([0xFFFFFFFF], dtype=np.uint32))
    with pytest.raises(OverflowError):
        accumulate_csr_host(big, big, 4)


def test_fold_ray_shards_host_sums_blocks():
    rng = np.random.default_rng(5)
    blocks = [random_csr(rng, 7, 23, 0.4) for _ in range(3)]
    want = sum(dense_of(b, 7, 23) for b in blocks)
    got = fold_ray_shards_host([(b[0], np.stack([b[1], b[2].view(np.int32)])) for b in blocks], 23)
    assert np.array_equal(dense_of(got, 7, 23), want)


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("R", [0, 1, 7, 29, 4096, 4099])
def test_ray_shards_tile_the_range(world, R):
    """ray_shard(k, W, R), k = 0 .. W-1, are consecutive ranges that cover
    [0, R) once, their lengths differing by at most one."""
    at = 0
    lens = []
    for k in range(world):
        b, e = ray_shard(k, world, R)
        assert b == at and e >= b
        lens.append(e - b)
        at = e
    assert at == R and max(lens) - min(lens) <= 1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-s", "-C", os.path.dirname(os.path.dirname(_lib.LIB_PATH))], check=True)
    return _lib.load()


def test_validation_without_gpu(lib):
    """The checks that come before any device work."""
    assert lib.rthx_abi_version() == 5
    r = C.c_void_p()
    s = C.c_void_p()
    assert lib.rthx_result_create(C.byref(r)) == 0 and lib.rthx_result_create(C.byref(s)) == 0
    try:
        args, _keep = _lib.make_args(0, 100, H.NUDGE, 1, 0, 10)
        # the ray range is checked first, whatever else the call was given
        assert lib.rthx_trace_exchange_rays(None, C.byref(args), -1, r) == abi.RTHX_EINVAL
        assert b"ray_begin" in lib.rthx_last_error()
        assert lib.rthx_trace_exchange_rays(None, C.byref(args), 2 ** 32 - 100, r) == abi.RTHX_ERANGE
        assert lib.rthx_trace_exchange_rays(None, C.byref(args), 2 ** 32 - 101, r) == abi.RTHX_EINVAL  # in range: null domain
        args.rays_per_emitter = 2 ** 32 - 1
        assert lib.rthx_trace_exchange_rays(None, C.byref(args), 1, r) == abi.RTHX_ERANGE
        assert lib.rthx_trace_exchange_rays(None, None, 0, r) == abi.RTHX_EINVAL
        # NULL operands
        assert lib.rthx_result_accumulate(None, r) == abi.RTHX_EINVAL
        assert lib.rthx_result_accumulate(r, None) == abi.RTHX_EINVAL
        assert lib.rthx_result_accumulate(r, r) == abi.RTHX_EINVAL
        assert lib.rthx_result_accumulate_csr(None, 0, None, None, None, 0) == abi.RTHX_EINVAL
        assert lib.rthx_result_accumulate_csr(r, 0, None, None, None, 0) == abi.RTHX_EINVAL
        assert lib.rthx_result_sampling_error(None, None, None) == abi.RTHX_EINVAL
        # results that hold no trace
        assert lib.rthx_result_accumulate(r, s) == abi.RTHX_ESTATE
        one = (C.c_int64 * 1)(0)
        assert lib.rthx_result_accumulate_csr(r, 0, one, None, None, 0) == abi.RTHX_ESTATE
        assert lib.rthx_result_accumulate_csr(r, -1, one, None, None, 0) == abi.RTHX_EINVAL
        rms = C.c_double(-1.0)
        assert lib.rthx_result_sampling_error(r, C.byref(rms), None) == abi.RTHX_ESTATE
        ms = C.c_double(-1.0)
        assert lib.rthx_result_accumulate_ms(r, C.byref(ms)) == 0 and ms.value == 0.0
    finally:
        lib.rthx_result_destroy(r)
        lib.rthx_result_destroy(s)


def _gloo_worker(rank, world, port, out_path):
    """Rank k holds block k over the same 7 rows; rank 1 gathers and folds."""
    import sys

    sys.path[:0] = [H.PKG, H.ROOT, os.path.join(H.ROOT, "tests")]
    import torch
    import torch.distributed as dist

    from rthx.distributed import fold_ray_shards_host, gather_ray_shards

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    rp, c, v = _gloo_block(rank)
    pairs = torch.from_numpy(np.stack([c, v.view(np.int32)]))
    blocks = gather_ray_shards(torch.from_numpy(rp), pairs, dst=1)
    assert (blocks is None) == (rank != 1)
    if rank == 1:
        srp, sc, sv = fold_ray_shards_host(blocks, 23)
        np.savez(out_path, row_ptr=srp, cols=sc, counts=sv)
    dist.barrier()
    dist.destroy_process_group()


def _gloo_block(rank):
    # (rank 0: one count above 2^31, which travels as int32 bits)
    blk = random_csr(np.random.default_rng(100 + rank), 7, 23, 0.3 + 0.2 * rank, empty_rows={rank})
    if rank == 0:
        blk[2][0] = 3_000_000_000
    return blk


def test_gloo_gather_and_fold_of_ray_shards(tmp_path):
    """The real-rank form's gather and host fold on a two-rank gloo group:
    blocks over the same rows are summed, not merged."""
    torch = pytest.importorskip("torch")
    import socket

    import torch.multiprocessing as mp

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "sum.npz")
    mp.spawn(_gloo_worker, args=(2, port, out), nprocs=2, join=True)
    m = np.load(out)
    want = csr_of_dense(dense_of(_gloo_block(0), 7, 23) + dense_of(_gloo_block(1), 7, 23))
    assert np.array_equal(m["row_ptr"], want[0]) and np.array_equal(m["cols"], want[1])
    assert np.array_equal(m["counts"], want[2])
