"""HIP smoothing (rthx_smooth_F) on synthetic matrices at the sizes where its
kernels change path (tests/solver_ref.py: continuous 50 : 1 weights, density 1
or rows of 1 .. 129 entries), against an extended-precision restatement of
the same passes and against oracle/smooth_oracle.py.

Dense sizes (csrc/rthx_smooth_kernels.hip):
  1, 2              below one tile of every kernel
  31, 32, 33        k_pair / k_recover_sym 32 x 32 transposed tiles
  63, 64, 65        k_ap_sym row tile (64 rows), k_ap_sym_reduce workgroup
  255, 256, 257     stride of the row kernels (k_delta_rows, k_rowsum, ...)
  511, 512, 513     k_ap_sym column tile (512); at 513 row tile 8 is the first
                    to start at column tile 1 (sym_jt0) and k_ap_sym_reduce
                    adds one rowpart and nine colpart slabs for row 512
  575, 577          around 9 x 64 rows with two column tiles
  1023, 1024, 1025  from 1024 on k_ap_sym has an unmasked interior tile
                    (rows 0 .. 63, columns 512 .. 1023); stride of k_dot
  1087, 1088, 1089  around 17 x 64
Odd n pads X's leading dimension by one column (the 16-byte pair store of
ap_sym_tile runs into it), even n does not.
Sparse: n = 9 (rows of 1 and 2 entries) and n = 515 (rows of 1, 2, 63, 64, 65,
127, 128, 129 entries before the union with the transpose): not multiples of
the 4 rows a workgroup holds, rows around one and two 64-lane strides.

Tolerance of the fixed-pass comparison (max_iters = 3, k_dykstra = 0: build_X,
hunger, 3 x (scale, hunger), recover_F, no convergence branch): entrywise
relative distance from the extended-precision result, at most 8 times the
distance of the float64 numpy restatement from it, and at least 4 eps.  Both
float64 computations round the same operations and differ only in the order of
the row sums (256-strided lanes and per-tile partials against numpy's pairwise
blocks), chains of 10 to 15 additions at these n; a dropped or doubled entry
moves a row sum by about 1 / n^2 relative, five orders above the bound.
Measured device / numpy ratios: profiles/round12/INDEX.md.  The same runs hold
info.delta_init and info.delta_final, the only outputs of the defect kernels
(k_delta_rows, k_sp_delta_rows) and of k_dot, to the defect of the
extended-precision iterate within solver_ref.defect_bound, a first-order
rounding bound counted from the kernels (about 4e-14 relative here; a row or
column left out of the sum moves the defect by about 1 / n).

Runs to convergence and Dykstra rounds are held to the criterion of
tests/test_gpu_smooth.py (compare, check_props).
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import solver_ref as R
from oracle import smooth_oracle as so
from test_gpu_smooth import check_props, compare

pytestmark = pytest.mark.gpu

DENSE_N = [1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513, 575, 577, 1023, 1024, 1025, 1087, 1088, 1089]
SPARSE = {9: [1, 2], 515: [1, 2, 63, 64, 65, 127, 128, 129]}


def fixed_passes(F, w):
    """Device and numpy results of three fixed passes and their distances (in
    eps) from the extended-precision result."""
    from rthx.smoothing import smooth_F

    n = F.shape[0]
    info = {}
    Fg = smooth_F(F, w, 0, max_iters=3, k_dykstra=0, verbose=False, info=info)
    k = 3 if n > 1 else 0  # (a 1 x 1 matrix has no pair: delta = 0 and no scale pass, on either side)
    assert info["n"] == n and info["k_dykstra"] == 0 and info["ap_iters"] == k
    log = []
    Fo = so.smooth_F(F, w, 0, max_iters=3, k_dykstra=0, log=log)
    assert [x for x in log if x[0] == "ap_done"][0][1] == k
    W = w / w.min()  # smooth_F's renorm, in float64 as there
    # the defect after build_X and at its last evaluation (k_delta_rows / k_sp_delta_rows, k_dot)
    checks = [x for x in log if x[0] == "ap"]
    for label, p, dev in (("delta_init", 0, info["delta_init"]),
                          ("delta_final", checks[-1][1] if checks else 0, info["delta_final"])):
        d, s_norm = R.defect_ld(F, W, p)
        bound = R.defect_bound(n, p, d, s_norm)
        print(f"{label} (after {p} passes) {dev:.17g}: {abs(dev - d):.2e} from extended precision, bound {bound:.2e}")
        assert abs(dev - d) <= bound
    Fl = R.smooth_fixed_ld(F, W, k)
    d_np, d_dev = R.rel_distance(Fo, Fl), R.rel_distance(Fg, Fl)
    tol = max(8.0 * d_np, 4.0)
    kind = "sparse" if sp.issparse(F) else "dense"
    print(f"fixed passes {kind} n {n}: device {d_dev:.2f} eps, numpy {d_np:.2f} eps, "
          f"ratio {d_dev / d_np if d_np else 0.0:.2f}, bound {tol:.1f} eps")
    return Fg, info, d_dev, tol


@pytest.mark.parametrize("n", DENSE_N)
def test_fixed_passes_dense(hip, n):
    F, w = R.synth_dense(n, n)
    Fg, info, d_dev, tol = fixed_passes(F, w)
    assert info["dense"] == 1 and Fg.shape == (n, n)
    assert d_dev <= tol


@pytest.mark.parametrize("n", sorted(SPARSE))
def test_fixed_passes_sparse(hip, n):
    F, w = R.synth_sparse(n, n, SPARSE[n])
    Fg, info, d_dev, tol = fixed_passes(F, w)
    assert info["dense"] == 0 and sp.issparse(Fg)
    # the union pattern of F and F', every row ascending
    U = ((F + F.T) != 0).tocsr()
    U.sort_indices()
    assert info["nnz"] == U.nnz
    assert np.array_equal(Fg.indptr, U.indptr) and np.array_equal(Fg.indices, U.indices)
    assert d_dev <= tol


def test_unsorted_rows_give_the_same_bits(hip):
    """include/rthx.h: rows of rthx_smooth_F's CSR need not be sorted.  (The
    sorted input's result is checked by test_fixed_passes_sparse[515].)"""
    from rthx import abi
    from rthx._lib import check
    from rthx.smoothing import _fetch, _smooth_args

    lib = hip.load()
    n = 515
    F, w = R.synth_sparse(n, n, SPARSE[n])
    sorted_in = (F.indptr.astype(np.int64), F.indices.astype(np.int32), F.data.astype(np.float64))
    reversed_in = R.reverse_rows(F)
    assert np.any(reversed_in[1] != sorted_in[1])
    out = []
    for rp, ci, v in (sorted_in, reversed_in):
        a = _smooth_args(0, 3, 0, False, True, False, False)
        h = C.c_void_p()
        check(lib.rthx_smooth_F(abi.ptr(rp, C.c_int64), abi.ptr(ci, C.c_int32), abi.ptr(v, C.c_double), n,
                                abi.ptr(w, C.c_double), n, 0, C.byref(a), C.byref(h)))
        try:
            inf = abi.SmoothInfo()
            check(lib.rthx_smooth_get_info(h, C.byref(inf)))
            assert inf.dense == 0 and inf.ap_iters == 3
            out.append(_fetch(lib, h, inf))
        finally:
            lib.rthx_smooth_destroy(h)
    A, B = out
    assert np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
    assert np.array_equal(A.data, B.data)


@pytest.mark.parametrize("n,k", [(2, 1), (33, 1), (257, 1), (1025, 1), (33, 6)])
def test_dykstra_rounds(hip, n, k):
    """OP + Dykstra (k_pair<XBAR>, k_rowsum, the PCG kernels, k_op_dykstra,
    k_renorm), then AP.  n = 1 is left out: b = 0 there and the reference's own
    solve_R divides 0 by 0."""
    F, w = R.synth_dense(n, n)
    Fg, info, log = compare(F, w, 0, k_dykstra=k)
    dyk = [x for x in log if x[0] == "dykstra"]
    print(f"n {n}, k_dykstra {k}: rounds {info['k_dykstra']}, PCG {info['pcg_iters']} (numpy {[x[2] for x in dyk]}), "
          f"AP {info['ap_iters']}, delta {info['delta_init']:.3g} -> {info['delta_final']:.3g}")
    assert info["dense"] == 1 and 1 <= info["k_dykstra"] <= k
    assert 0 < info["pcg_iters"] < 200  # the PCG cap is not reached
    check_props(Fg, w)


@pytest.mark.parametrize("n", [65, 513, 1089])
def test_full_ap_dense(hip, n):
    F, w = R.synth_dense(n, n)
    Fg, info, log = compare(F, w, 0)
    print(f"dense n {n}: AP {info['ap_iters']} iterations, delta {info['delta_init']:.3g} -> {info['delta_final']:.3g}")
    assert info["dense"] == 1 and info["k_dykstra"] == 0 and info["converged"] == 1
    check_props(Fg, w)


@pytest.mark.parametrize("n", sorted(SPARSE))
def test_full_ap_sparse(hip, n):
    F, w = R.synth_sparse(n, n, SPARSE[n])
    Fg, info, log = compare(F, w, 0)
    print(f"sparse n {n}: AP {info['ap_iters']} iterations, delta {info['delta_init']:.3g} -> {info['delta_final']:.3g}")
    assert info["dense"] == 0 and sp.issparse(Fg) and info["converged"] == 1
    check_props(Fg, w)
