"""rthx_csr_symmetrize (rthx.csr_symmetrize; csrc/rthx_symmetrize_kernels.hip,
DESIGN.md §7i): X = (Diagonal(w) A + (Diagonal(w) A)') / 2 held bit-equal --
indptr, indices and the bytes of data -- to a union merge written here in
numpy with the arithmetic the header fixes: a_ij = RN(w_i v_ij) for a stored
entry and +0.0 for an absent one, x_ij = RN(0.5 RN(a_ij + a_ji)), every
stored entry kept (scipy's A + A.T drops zero sums, so it is not the
reference).

Shapes: the launcher has one form, a wave (G = 64 lanes) per row in
workgroups of four rows, with no switch on the row length; the mark pass
walks a row of A' 64 entries at a time and the write pass strides both rows
by 64, so rows and columns of G - 1, G, G + 1 and 2G + 1 entries are the
edges.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import solver_ref as SR

pytestmark = pytest.mark.gpu

G = 64  # rthx::sym::kGroup


def csr(n, rows, cols, vals):
    """CSR with the entries as given (stored zeros kept), rows sorted by column."""
    rows, cols, vals = np.asarray(rows, np.int64), np.asarray(cols, np.int64), np.asarray(vals, np.float64)
    order = np.lexsort((cols, rows))
    rp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=rp[1:])
    return sp.csr_matrix((vals[order], cols[order].astype(np.int32), rp), shape=(n, n))


def reference(A, w=None):
    """(indptr, indices, data) of X by a union merge of the (row, column) keys
    of A and A' (row-major key order = every row column-ascending)."""
    n = A.shape[0]
    rp, ci, v = A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data.astype(np.float64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    a = (np.ones(n) if w is None else np.asarray(w, np.float64))[rows] * v  # RN(w_i v_ij)
    key_a, key_t = rows * n + ci, ci * n + rows
    keys = np.union1d(key_a, key_t)
    xa, xt = np.zeros(len(keys)), np.zeros(len(keys))  # absent: +0.0
    xa[np.searchsorted(keys, key_a)] = a
    xt[np.searchsorted(keys, key_t)] = a
    x = 0.5 * (xa + xt)
    xrp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(keys // max(n, 1), minlength=n), out=xrp[1:])
    return xrp, (keys % max(n, 1)).astype(np.int32), x


def check(hip, A, w=None):
    from rthx import csr_symmetrize

    X = csr_symmetrize(A, w)
    xrp, xci, xv = reference(A, w)
    assert X.shape == A.shape
    assert np.array_equal(X.indptr, xrp)
    assert np.array_equal(X.indices, xci)
    assert np.array_equal(X.data.view(np.uint64), xv.view(np.uint64))
    return X


def values(rng, k):
    return rng.standard_normal(k) * np.exp(rng.uniform(-5, 5, k))


def test_empty_and_single(hip):
    check(hip, sp.csr_matrix((0, 0)))
    check(hip, sp.csr_matrix((1, 1)))
    X = check(hip, csr(1, [0], [0], [np.pi]), w=np.array([3.0]))
    assert X.nnz == 1 and X.data[0] == 0.5 * (3.0 * np.pi + 3.0 * np.pi)
    X = check(hip, sp.csr_matrix((5, 5)))
    assert X.nnz == 0 and np.all(X.indptr == 0)


def test_diagonal_only(hip):
    rng = np.random.default_rng(1)
    n = 3 * G + 7
    v, w = values(rng, n), SR.weights(n, rng)
    X = check(hip, csr(n, np.arange(n), np.arange(n), v), w)
    assert X.nnz == n and np.array_equal(X.data, w * v)  # x_ii = a_ii


def test_strictly_upper_triangular(hip):
    rng = np.random.default_rng(2)
    n = 150
    r, c = np.triu_indices(n, k=1)
    keep = rng.random(len(r)) < 0.3
    A = csr(n, r[keep], c[keep], values(rng, keep.sum()))
    X = check(hip, A, SR.weights(n, rng))
    assert X.nnz == 2 * A.nnz  # no match: lenA + lenT
    assert np.array_equal(np.diff(X.indptr), np.diff(A.indptr) + np.bincount(A.indices, minlength=n))


def test_symmetric_pattern_unequal_values(hip):
    rng = np.random.default_rng(3)
    n = 200
    P = sp.random(n, n, density=0.1, random_state=7, format="coo")
    r = np.concatenate([P.row, P.col])
    c = np.concatenate([P.col, P.row])
    keys = np.unique(r.astype(np.int64) * n + c)
    A = csr(n, keys // n, keys % n, values(rng, len(keys)))
    X = check(hip, A, SR.weights(n, rng))
    assert X.nnz == A.nnz and np.array_equal(X.indices, A.indices)  # every entry matches
    Xt = X.T.tocsr()
    Xt.sort_indices()
    assert np.array_equal(Xt.data.view(np.uint64), X.data.view(np.uint64))  # x_ij == x_ji bitwise


def test_one_full_row_and_one_full_column(hip):
    rng = np.random.default_rng(4)
    n = 600
    v, w = values(rng, n), SR.weights(n, rng)
    A = csr(n, np.zeros(n, int), np.arange(n), v)
    X = check(hip, A, w)
    assert np.array_equal(np.diff(X.indptr), np.r_[n, np.ones(n - 1, int)])
    X = check(hip, csr(n, np.arange(n), np.zeros(n, int), v), w)  # the mirror image
    assert np.array_equal(np.diff(X.indptr), np.r_[n, np.ones(n - 1, int)])


@pytest.mark.parametrize("transposed", [False, True])
def test_row_lengths_at_the_group_edges(hip, transposed):
    """Rows (or, transposed, columns: rows of A') of G - 1, G, G + 1 and
    2 G + 1 entries, partly matched by the other side."""
    rng = np.random.default_rng(5)
    lens = [G - 1, G, G + 1, 2 * G + 1, 1, 0]
    n = 2 * G + 40
    r, c = [], []
    for i in range(n):
        L = lens[i % len(lens)]
        r += [i] * L
        c += list(np.sort(rng.choice(n, L, replace=False)))
    A = csr(n, c if transposed else r, r if transposed else c, values(rng, len(r)))
    check(hip, A, SR.weights(n, rng))
    check(hip, A)


def test_empty_rows_at_start_middle_end(hip):
    rng = np.random.default_rng(6)
    n = 300
    B = sp.random(n, n, density=0.05, random_state=11, format="coo")
    live = (B.row >= 10) & ~((B.row >= 100) & (B.row < 180)) & (B.row < 290)
    live &= (B.col >= 5) & (B.col < 280)  # rows of A' empty at both ends too
    A = csr(n, B.row[live], B.col[live], values(rng, live.sum()))
    X = check(hip, A, SR.weights(n, rng))
    assert X.indptr[5] == 0 and X.indptr[-1] == X.indptr[290]


@pytest.mark.parametrize("n", [9, 515])
def test_synth_sparse_with_random_weights(hip, n):
    F, _w = SR.synth_sparse(n, seed=n, lens=[3, 40, 1, 130, 65])
    w = SR.weights(n, np.random.default_rng(n + 1))
    check(hip, F, w)
    check(hip, F)  # w = None


def test_signs_zeros_and_exact_cancellation(hip):
    """Negative values, stored zeros (+0.0 and -0.0) and an entry whose mirror
    cancels it exactly: every stored entry stays, a cancelled sum is +0.0."""
    n = 6
    rows = [0, 0, 1, 1, 2, 3, 4, 5]
    cols = [1, 3, 0, 2, 2, 0, 5, 4]
    vals = [2.5, -1.0, -2.5, 0.0, -0.0, 7.0, -3.0, 0.0]
    A = csr(n, rows, cols, vals)
    assert A.nnz == 8
    X = check(hip, A)
    D = {(i, int(j)): X.data[k] for i in range(n) for k, j in
         zip(range(X.indptr[i], X.indptr[i + 1]), X.indices[X.indptr[i]:X.indptr[i + 1]])}
    for key in ((0, 1), (1, 0), (1, 2), (2, 1)):  # the cancelled pair, a stored zero and its mirror
        assert D[key] == 0.0 and not np.signbit(D[key]), key
    assert D[(2, 2)] == 0.0 and np.signbit(D[(2, 2)])  # -0.0 + -0.0: the diagonal matches itself
    assert D[(0, 3)] == D[(3, 0)] == 3.0 and D[(4, 5)] == D[(5, 4)] == -1.5
    check(hip, A, np.array([1.0, 1.0, 2.0, 0.5, 3.0, 3.0]))


def test_x_cap_protocol(hip):
    """x_cap one entry short: RTHX_ERANGE, x_nnz the size needed, x_row_ptr
    written, x_cols and x_vals untouched; the exact x_cap then succeeds."""
    from rthx import abi

    lib = hip.load()
    F, w = SR.synth_sparse(130, seed=8, lens=[5, 70, 2])
    xrp_ref, xci_ref, xv_ref = reference(F, w)
    need = len(xci_ref)
    rp = np.ascontiguousarray(F.indptr, dtype=np.int64)
    ci = np.ascontiguousarray(F.indices, dtype=np.int32)
    vv = np.ascontiguousarray(F.data, dtype=np.float64)
    i64, i32, dp = C.c_int64, C.c_int32, C.c_double

    def call(cap):
        xrp = np.full(131, -1, dtype=np.int64)
        xci = np.full(need, -7, dtype=np.int32)
        xv = np.full(need, -7.0)
        xnnz = C.c_int64(-1)
        rc = lib.rthx_csr_symmetrize(0, 130, abi.ptr(rp, i64), abi.ptr(ci, i32), abi.ptr(vv, dp), abi.ptr(w, dp), cap,
                                     abi.ptr(xrp, i64), abi.ptr(xci, i32), abi.ptr(xv, dp), C.byref(xnnz), None)
        return rc, xnnz.value, xrp, xci, xv

    rc, xnnz, xrp, xci, xv = call(need - 1)
    assert rc == abi.RTHX_ERANGE and xnnz == need
    assert np.array_equal(xrp, xrp_ref)
    assert np.all(xci == -7) and np.all(xv == -7.0)
    rc, xnnz, xrp, xci, xv = call(need)
    assert rc == abi.RTHX_OK and xnnz == need
    assert np.array_equal(xrp, xrp_ref) and np.array_equal(xci, xci_ref)
    assert np.array_equal(xv.view(np.uint64), xv_ref.view(np.uint64))


def test_two_runs_give_identical_bytes(hip):
    from rthx import csr_symmetrize

    F, w = SR.synth_sparse(515, seed=9, lens=[3, 40, 1, 130, 65])
    info = {}
    a, b = csr_symmetrize(F, w), csr_symmetrize(F, w, info=info)
    for x, y in ((a.indptr, b.indptr), (a.indices, b.indices), (a.data, b.data)):
        assert x.tobytes() == y.tobytes()
    assert info["device_ms"] > 0.0


def test_unsorted_rows_equal_sorted_input(hip):
    from rthx import csr_symmetrize

    rng = np.random.default_rng(10)
    F, w = SR.synth_sparse(200, seed=10, lens=[7, 66, 20])
    perm = np.concatenate([F.indptr[i] + rng.permutation(F.indptr[i + 1] - F.indptr[i]) for i in range(200)])
    U = sp.csr_matrix((F.data[perm], F.indices[perm], F.indptr), shape=F.shape)
    assert not U.has_sorted_indices
    a, b = csr_symmetrize(U, w), csr_symmetrize(F, w)
    for x, y in ((a.indptr, b.indptr), (a.indices, b.indices), (a.data, b.data)):
        assert x.tobytes() == y.tobytes()
    check(hip, F, w)
