"""Host side of the spectral GERT solve (include/rthx.h rthx_solve_spectral,
rthx_spectral_apply, rthx_spectral_fractions): argument validation, which
runs before any GPU call; the ctypes mirrors of the three new structs against
gcc; and the numpy restatement the GPU tests compare with
(tests/spectral_ref.py), pinned on an isothermal enclosure."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import spectral_ref as R
from rthx import abi, _lib

HEADER = os.path.join(H.ROOT, "include", "rthx.h")
DP = C.c_double


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


class Problem:
    """A small valid problem (n = 4, K = 3, dense shared F); tests break one
    argument at a time."""

    def __init__(self, n=4, K=3, n_mats=1):
        self.n, self.K, self.n_mats = n, K, n_mats
        self.F = [np.full((n, n), 1.0 / n) for _ in range(n_mats)]
        self.bands = (abi.SpectralBand * n_mats)()
        for k in range(n_mats):
            self.bands[k].dense = abi.ptr(self.F[k], DP)
        self.limits = np.array([1e-6, 3e-6, 8e-6, 1e-3][: K + 1])
        self.b = np.full((K, n), 0.5)
        self.prop = np.full((K, n), 0.5)
        self.size = np.ones(n)
        self.T_in = np.array([1000.0] + [-1.0] * (n - 1))
        self.q_in = np.zeros(n)
        self.args = abi.SpectralArgs()
        self.args.device, self.args.memory, self.args.itmax, self.args.max_outer = 0, 50, 0, 10
        self.args.rtol, self.args.atol, self.args.convergence_tol = 1e-12, 1e-8, 1e-12
        self.out = [np.zeros((K, n)), np.zeros((K, n)), np.zeros(n), np.zeros(n)]

    def solve(self, lib, n=None, K=None, n_mats=None):
        info = abi.SpectralInfo()
        return lib.rthx_solve_spectral(self.bands, self.n_mats if n_mats is None else n_mats,
                                       self.n if n is None else n, self.K if K is None else K,
                                       abi.ptr(self.limits, DP), abi.ptr(self.b, DP), abi.ptr(self.prop, DP),
                                       abi.ptr(self.size, DP), abi.ptr(self.T_in, DP), abi.ptr(self.q_in, DP),
                                       C.byref(self.args), abi.ptr(self.out[0], DP), abi.ptr(self.out[1], DP),
                                       abi.ptr(self.out[2], DP), abi.ptr(self.out[3], DP), C.byref(info))


def test_sizes_rejected(lib):
    p = Problem()
    assert p.solve(lib, n=0) == abi.RTHX_EINVAL
    assert p.solve(lib, K=0) == abi.RTHX_EINVAL
    assert p.solve(lib, n_mats=2) == abi.RTHX_EINVAL  # neither 1 nor n_bands
    assert p.solve(lib, n_mats=0) == abi.RTHX_EINVAL
    assert p.solve(lib, n=1 << 31) == abi.RTHX_ERANGE  # (rejected before any array is read)
    assert b"too large" in lib.rthx_last_error()


@pytest.mark.parametrize("limits", [[0.0, 3e-6, 8e-6, 1e-3], [-1e-6, 3e-6, 8e-6, 1e-3], [1e-6, 3e-6, 3e-6, 1e-3],
                                    [1e-6, 8e-6, 3e-6, 1e-3], [1e-6, 3e-6, np.nan, 1e-3],
                                    [1e-6, 3e-6, 8e-6, np.inf]])
def test_band_limits_rejected(lib, limits):
    p = Problem()
    p.limits = np.array(limits)
    assert p.solve(lib) == abi.RTHX_EINVAL
    assert b"band limits" in lib.rthx_last_error()


@pytest.mark.parametrize("name", ["b", "prop", "size", "T_in", "q_in"])
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_inputs_rejected(lib, name, bad):
    p = Problem()
    getattr(p, name).flat[-1] = bad
    assert p.solve(lib) == abi.RTHX_EINVAL


def test_non_finite_matrix_rejected(lib):
    p = Problem()
    p.F[0][1, 2] = np.nan
    assert p.solve(lib) == abi.RTHX_EINVAL


@pytest.mark.parametrize("bad", [-0.1, 1.5])
def test_b_outside_unit_interval_rejected(lib, bad):
    p = Problem()
    p.b[1, 2] = bad
    assert p.solve(lib) == abi.RTHX_EINVAL
    assert b"[0, 1]" in lib.rthx_last_error()


def test_no_prescribed_temperature_rejected(lib):
    p = Problem()
    p.T_in[:] = -1.0
    assert p.solve(lib) == abi.RTHX_EINVAL
    assert b"prescribed temperature" in lib.rthx_last_error()


def test_band_forms_rejected(lib):
    p = Problem(n_mats=3)
    p.bands[1].dense = C.cast(None, C.POINTER(DP))  # no form
    assert p.solve(lib) == abi.RTHX_EINVAL
    assert b"band 1" in lib.rthx_last_error()
    p = Problem(n_mats=3)
    rp = np.zeros(p.n + 1, dtype=np.int64)
    ci = np.zeros(1, dtype=np.int32)
    vv = np.zeros(1)
    p.bands[2].row_ptr, p.bands[2].cols, p.bands[2].vals = abi.ptr(rp, C.c_int64), abi.ptr(ci, C.c_int32), abi.ptr(vv, DP)
    assert p.solve(lib) == abi.RTHX_EINVAL  # dense and CSR at once
    assert b"band 2" in lib.rthx_last_error()
    p = Problem()
    p.bands[0].dense = C.cast(None, C.POINTER(DP))
    bad_rp = np.array([0, 2, 1, 2, 2], dtype=np.int64)  # not monotone
    ci = np.zeros(2, dtype=np.int32)
    vv = np.ones(2)
    p.bands[0].row_ptr, p.bands[0].cols, p.bands[0].vals = abi.ptr(bad_rp, C.c_int64), abi.ptr(ci, C.c_int32), abi.ptr(vv, DP)
    assert p.solve(lib) == abi.RTHX_EINVAL


def test_kernel_entry_points_validate(lib):
    p = Problem()
    x = np.ones((p.K, p.n))
    g = np.zeros((p.K, p.n))
    none = C.cast(None, C.POINTER(DP))
    no_flags = C.cast(None, C.POINTER(C.c_uint8))
    assert lib.rthx_spectral_apply(p.bands, 1, 0, p.K, 0, abi.ptr(x, DP), none, none, no_flags, abi.ptr(g, DP),
                                   none) == abi.RTHX_EINVAL
    assert lib.rthx_spectral_apply(p.bands, 2, p.n, p.K, 0, abi.ptr(x, DP), none, none, no_flags, abi.ptr(g, DP),
                                   none) == abi.RTHX_EINVAL
    assert lib.rthx_spectral_apply(p.bands, 1, 1 << 31, p.K, 0, abi.ptr(x, DP), none, none, no_flags,
                                   abi.ptr(g, DP), none) == abi.RTHX_ERANGE
    # y asked for without b and f
    assert lib.rthx_spectral_apply(p.bands, 1, p.n, p.K, 0, abi.ptr(x, DP), none, none, no_flags, abi.ptr(g, DP),
                                   abi.ptr(g, DP)) == abi.RTHX_EINVAL
    T = np.full(p.n, 300.0)
    bad = np.array([1e-6, 1e-6, 8e-6, 1e-3])
    assert lib.rthx_spectral_fractions(abi.ptr(bad, DP), p.K, abi.ptr(T, DP), none, p.n, 0, abi.ptr(g, DP),
                                       none) == abi.RTHX_EINVAL
    assert lib.rthx_spectral_fractions(abi.ptr(p.limits, DP), 0, abi.ptr(T, DP), none, p.n, 0, abi.ptr(g, DP),
                                       none) == abi.RTHX_EINVAL


_MIRRORS = [("rthx_spectral_band", abi.SpectralBand), ("rthx_spectral_args", abi.SpectralArgs),
            ("rthx_spectral_info", abi.SpectralInfo)]


def test_spectral_struct_layouts_match_c_compiler(tmp_path):
    """Every field offset and struct size of the three new ctypes mirrors
    equals what gcc computes from include/rthx.h."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {"]
    for c_name, py in _MIRRORS:
        lines.append(f'  printf("{c_name} size %zu\\n", sizeof({c_name}));')
        for f, _ in py._fields_:
            lines.append(f'  printf("{c_name} {f} %zu\\n", offsetof({c_name}, {f}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    got = dict()
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        k1, k2, v = line.split()
        got[(k1, k2)] = int(v)
    for c_name, py in _MIRRORS:
        assert got[(c_name, "size")] == C.sizeof(py), c_name
        for f, _ in py._fields_:
            assert got[(c_name, f)] == getattr(py, f).offset, (c_name, f)


def test_restatement_isothermal_enclosure():
    """spectral_ref on a 3 x 3 square, walls at 1000 K, selective kappa and
    black walls, synthetic reciprocal F per band: the gas takes the wall
    temperature.  Bound 1e-8 K: the sweeps stop at a relative change of
    1e-14 in j, the QR solve is good to eps times the condition of the
    stacked matrix (about 1e2 here), and T = (e / ...)^(1/4) carries a
    quarter of that relative error at 1000 K, about 1e-10 K."""
    K = 5
    limits = np.logspace(-7, -2, K + 1)
    dom = R.spectral_square(3, K, np.linspace(0.5, 1.5, K), 1.0, T_walls=(1000.0,) * 4, limits=limits)
    b, prop, size, T_in, q_in = R.domain_arrays(dom)
    assert b.shape == (K, 12 + 9) and np.all(T_in[:12] == 1000.0) and np.all(T_in[12:] < -0.1)
    rng = np.random.default_rng(5)
    F = [R.reciprocal_F(size * prop[k], rng) for k in range(K)]
    j, T, e, sweeps = R.reference_solve(F, limits, b, prop, size, T_in, q_in)
    assert np.max(np.abs(T - 1000.0)) < 1e-8
    f = R.weighted_fractions(limits, T, prop)
    for k in range(K):  # and the state it returns satisfies the band equations
        g = F[k].T @ j[k]
        assert np.linalg.norm(j[k] - b[k] * g - e * f[k]) <= 1e-12 * np.linalg.norm(e)
