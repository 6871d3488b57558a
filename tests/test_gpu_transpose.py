"""rthx_csr_transpose (rthx.csr_transpose; csrc/rthx_transpose_kernels.hip,
DESIGN.md §7h) against scipy's A.T.tocsr() with sorted indices.  The
transpose moves entries and computes nothing, so the offsets, indices and
values must be bit-equal; duplicate (row, column) pairs must keep their
input order, which scipy's own transpose is not asked for: those cases are
held against a stable counting sort in numpy.

Shapes: T = 4096 entries is the kernel's tile (256 lanes x 16 rounds), 256
the bins of a radix pass; n_cols 1 .. 256 take one pass, .. 65536 two, above
that three.
"""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

T = 4096


def distinct_values(rng, nnz):
    """nnz finite doubles with pairwise distinct bit patterns (a misplaced
    payload cannot go unnoticed)."""
    v = rng.standard_normal(nnz) * np.exp(rng.uniform(-30, 30, nnz))
    v += np.arange(nnz) * 1e-7 * np.abs(v)
    assert len(np.unique(v.view(np.uint64))) == nnz
    return v


def stable_transpose(n_rows, n_cols, rp, ci, vv):
    """Counting sort by column, rows visited in order (the host transpose of
    rthx_solve_grey): the reference for inputs with duplicates."""
    rows = np.repeat(np.arange(n_rows), np.diff(rp))
    order = np.argsort(ci, kind="stable")
    trp = np.zeros(n_cols + 1, dtype=np.int64)
    np.cumsum(np.bincount(ci, minlength=n_cols), out=trp[1:])
    return trp, rows[order].astype(np.int32), vv[order]


def random_csr(rng, n_rows, n_cols, nnz, sort_rows=False):
    """nnz entries without duplicates, row-major, columns within a row in
    random order (or ascending)."""
    flat = rng.choice(n_rows * n_cols, size=nnz, replace=False) if n_rows * n_cols < (1 << 26) else \
        np.unique(rng.integers(0, n_rows * n_cols, size=2 * nnz))[:nnz]
    nnz = len(flat)
    r, c = np.divmod(np.sort(flat), n_cols)
    if not sort_rows:
        perm = np.lexsort((rng.random(nnz), r))  # shuffle within rows
        r, c = r[perm], c[perm]
    rp = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=n_rows), out=rp[1:])
    return sp.csr_matrix((distinct_values(rng, nnz), c.astype(np.int32), rp), shape=(n_rows, n_cols))


def check(hip, A):
    from rthx import csr_transpose

    At = csr_transpose(A)
    rp = A.indptr.astype(np.int64)
    trp, tci, tv = stable_transpose(A.shape[0], A.shape[1], rp, A.indices, A.data)
    assert At.shape == (A.shape[1], A.shape[0])
    assert np.array_equal(At.indptr, trp)
    assert np.array_equal(At.indices, tci)
    assert np.array_equal(At.data.view(np.uint64), tv.view(np.uint64))
    keys = np.repeat(np.arange(A.shape[0]), np.diff(rp)) * A.shape[1] + A.indices
    if len(np.unique(keys)) == A.nnz:  # no duplicates: scipy's own transpose is the same matrix
        S = A.T.tocsr()
        S.sort_indices()
        assert np.array_equal(S.indptr, At.indptr) and np.array_equal(S.indices, At.indices)
        assert np.array_equal(S.data.view(np.uint64), At.data.view(np.uint64))
    return At


def test_empty_and_single_entry(hip):
    check(hip, sp.csr_matrix((5, 7)))
    check(hip, sp.csr_matrix((0, 3)))
    check(hip, sp.csr_matrix((3, 0)))
    for shape, r, c in (((1, 1), 0, 0), ((9, 300), 4, 299), ((300, 9), 299, 0)):
        A = sp.csr_matrix((np.array([np.pi]), (np.array([r]), np.array([c]))), shape=shape)
        check(hip, A)


def test_single_column_holding_every_row(hip):
    """One digit bin that spans several tiles: the place of an entry is its
    rank across rounds, waves and tiles alone."""
    rng = np.random.default_rng(1)
    n = 3 * T + 5
    for n_cols, col in ((1, 0), (300, 77)):
        A = sp.csr_matrix((distinct_values(rng, n), np.full(n, col, dtype=np.int32), np.arange(n + 1)),
                          shape=(n, n_cols))
        check(hip, A)


def test_empty_leading_and_trailing_columns(hip):
    rng = np.random.default_rng(2)
    B = random_csr(rng, 200, 100, 3000)
    A = sp.csr_matrix((B.data, B.indices + 450, B.indptr), shape=(200, 1000))  # columns 450 .. 549 only
    At = check(hip, A)
    assert np.all(At.indptr[:451] == 0) and np.all(At.indptr[550:] == A.nnz)


@pytest.mark.parametrize("n_cols", [1, 255, 256, 257, 300, 65537])
def test_pass_counts(hip, n_cols):
    rng = np.random.default_rng(n_cols)
    n_rows = 5000 if n_cols == 1 else 97
    nnz = min(5000, n_rows * n_cols)
    A = random_csr(rng, n_rows, n_cols, nnz)
    if n_cols > 256:  # the top column present: every digit of the last pass's range is exercised
        A = sp.vstack([A, sp.csr_matrix((np.array([1.5]), (np.array([0]), np.array([n_cols - 1]))),
                                        shape=(1, n_cols))]).tocsr()
    check(hip, A)


@pytest.mark.parametrize("shape", [(3, 20000), (20000, 3), (1, 70000), (70000, 1)])
def test_rectangular(hip, shape):
    rng = np.random.default_rng(shape[0])
    check(hip, random_csr(rng, shape[0], shape[1], min(6000, shape[0] * shape[1])))


@pytest.mark.parametrize("nnz", [T - 1, T, T + 1])
def test_tile_edges(hip, nnz):
    rng = np.random.default_rng(nnz)
    check(hip, random_csr(rng, 130, 700, nnz))
    check(hip, random_csr(rng, 130, 700, nnz, sort_rows=True))


def test_one_column_in_5000_consecutive_rows(hip):
    """Cross-tile and cross-wave rank order: column 123 in rows 1000 .. 5999
    among random other entries."""
    rng = np.random.default_rng(3)
    B = random_csr(rng, 7000, 400, 20000).tocoo()
    keep = B.col != 123
    rows = np.arange(1000, 6000)
    r = np.concatenate([B.row[keep], rows])
    c = np.concatenate([B.col[keep], np.full(5000, 123)])
    perm = np.lexsort((rng.random(len(r)), r))  # row-major, the column's place within its rows varies
    rp = np.zeros(7001, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=7000), out=rp[1:])
    A = sp.csr_matrix((distinct_values(rng, len(r)), c[perm].astype(np.int32), rp), shape=(7000, 400))
    At = check(hip, A)
    assert np.array_equal(At.indices[At.indptr[123]:At.indptr[124]], rows)


def test_duplicates_keep_input_order(hip):
    rng = np.random.default_rng(5)
    n_rows, n_cols, per = 600, 300, 20
    ci = rng.integers(0, 12, size=n_rows * per).astype(np.int32) * 25  # 12 columns: many repeats within a row
    rp = np.arange(0, n_rows * per + 1, per, dtype=np.int64)
    A = sp.csr_matrix((distinct_values(rng, len(ci)), ci, rp), shape=(n_rows, n_cols))
    assert not A.has_canonical_format
    check(hip, A)


def test_two_runs_give_identical_bytes(hip):
    from rthx import csr_transpose

    rng = np.random.default_rng(6)
    A = random_csr(rng, 900, 1300, 3 * T + 5)
    a, b = csr_transpose(A), csr_transpose(A)
    for x, y in ((a.indptr, b.indptr), (a.indices, b.indices), (a.data, b.data)):
        assert x.tobytes() == y.tobytes()
    info = {}
    csr_transpose(A, info=info)
    assert info["device_ms"] > 0.0
