"""The CPU restatement's recorded rays against the analytic laws of emission
and free paths (tests/emission_laws.py), in both sampling modes, and the two
modes' count matrices against each other.

Exact parity holds every device kernel to the restatement; this file holds
the restatement -- which carries the same sampling algebra as the device, so
a mistake in it is common-mode -- to laws that involve no code of the project.
tests/test_gpu_emission_laws.py and tests/test_gpu_sampling_modes.py run the
same cases through the same statistics on the device.

Measured on the restatement (R = 2e5, seeds 5, 7, 9, 11; both modes): the 278
p-values of the laws lie between 2.9e-3 and 0.998; every control is rejected,
tau x 1.03 with p between 2.7e-29 and 1.4e-14, tau against the other emitter
kind's law below 1e-213, alpha against uniform and the barycentric
coordinates against uniform with p = 0.
"""
import numpy as np
import pytest
import scipy.integrate

import emission_laws as EL
import helpers as H
from oracle import oracle


@pytest.mark.parametrize("n", [2, 3])
def test_tau_cdf_tables(n):
    """The tables against direct quadrature, on points other than those
    tau_cdf checks itself with; the moments the laws quote."""
    err = EL.table_error(n, points=50, seed=77)
    print(f"Ki_{n} table: max error {err:.2e}")
    assert err <= 1e-7
    cdf = EL.tau_cdf(n)
    assert abs(cdf(0.0)) < 1e-15 and cdf(1e3) == 1.0 and np.all(np.diff(cdf(np.linspace(0, 45, 2000))) >= -1e-9)
    t = np.linspace(0.0, 40.0, 400_001)
    sf = 1.0 - cdf(t)
    assert abs(scipy.integrate.trapezoid(sf, t) - EL.TAU_MEAN[n]) < 1e-6
    assert abs(2 * scipy.integrate.trapezoid(t * sf, t) - EL.TAU_MEAN[n] ** 2 - EL.TAU_VAR[n]) < 1e-6


def test_statistics_on_synthetic_rays():
    """The statistics themselves, on rays drawn here from the laws with
    numpy's generator in a 1 x 1 cell of a kappa = 60 square: they pass, and
    the controls reject."""
    flat, emitters = EL.law_flat("square")
    rng = np.random.default_rng(3)
    n = EL.R_LAWS
    g = emitters["centre"]
    poly = EL.cell_polygon(flat, g - flat.n_surfaces)
    o = poly[0] + rng.random((n, 2)) * (poly[2] - poly[0])
    mu, phi = rng.uniform(-1, 1, n), rng.uniform(0, 2 * np.pi, n)
    d = np.stack([np.sqrt(1 - mu * mu) * np.cos(phi), mu], axis=1)
    e = o + d * (-np.log(rng.random(n)) / 60.0)[:, None]
    assert min(EL.laws(flat, g, o, e).values()) >= 1e-4
    assert max(EL.controls(flat, g, o, e).values()) < EL.P_BOUND
    g = emitters["wall0"]
    p1, p2 = EL.emitter_wall(flat, g)
    t = (p2 - p1) / np.linalg.norm(p2 - p1)
    o = p1 + rng.random((n, 1)) * (p2 - p1)
    ct, psi = np.sqrt(rng.random(n)), rng.uniform(0, 2 * np.pi, n)
    d = np.outer(np.sqrt(1 - ct * ct) * np.cos(psi), t) + np.outer(ct, [-t[1], t[0]])
    e = o + d * (-np.log(rng.random(n)) / 60.0)[:, None]
    assert min(EL.laws(flat, g, o, e).values()) >= 1e-4
    assert max(EL.controls(flat, g, o, e).values()) < EL.P_BOUND


def test_cases_reach_the_paths_they_name():
    flat, em = EL.law_flat("square")
    assert flat.uniform_beta[0] == 60.0 and len(set(em.values())) == 5 and em["centre"] == flat.n_surfaces + 12
    assert np.allclose(flat.fine_mid.reshape(-1, 2)[12], 0.5)
    flat, em = EL.law_flat("wedge")
    assert [int(flat.fine_nv[g - flat.n_surfaces]) for g in em.values()] == [3, 4, 3] and flat.n_coarse == 8
    flat, em = EL.law_flat("layers")
    assert flat.uniform_beta[0] < -0.1
    beta = flat.beta.reshape(1, -1)[0]
    assert [beta[g - flat.n_surfaces] for g in em.values()] == [20.0, 50.0]
    mid = flat.fine_mid.reshape(-1, 2)
    assert all(abs(mid[g - flat.n_surfaces][0] - 2.0) < 1e-12 for g in em.values())


@pytest.mark.parametrize("flags", [0, EL.FAITHFUL], ids=["default", "faithful"])
@pytest.mark.parametrize("case,key", EL.LAW_EMITTERS, ids=EL.LAW_IDS)
def test_restatement_rays_obey_the_laws(case, key, flags):
    flat, g, _args, _keep = EL.law_args(case, key, flags)
    o, e = EL.restatement_rays(case, key, flags)
    p = EL.laws(flat, g, o, e)
    c = EL.controls(flat, g, o, e)
    print(f"{case} {key} flags {flags}: laws {p}\ncontrols {c}")
    EL.record("cpu", f"laws/{case}/{key}/{'faithful' if flags else 'default'}", {"laws": p, "controls": c})
    for name, v in p.items():
        assert v >= EL.P_BOUND, (name, v)
    for name, v in c.items():
        assert v < EL.P_BOUND, (name, v)


@pytest.mark.parametrize("case", EL.MODE_CPU_CASES)
def test_sampling_modes_agree_count_for_count(case):
    """Default sampling at seed 101 against faithful sampling at seed 202,
    every row at R = 2e5 (emission_laws.compare_modes); faithful sampling
    with every kappa x 1.02 is told apart.  Measured here, z = (X2 - dof) /
    sqrt(2 dof): square5 -1.17, rotated5 -0.12, wedges -0.41, quad_lattice
    -0.20; the controls 12.6, 13.4, 17.9, 11.9."""
    dense = []
    for _name, flat, args, _keep in EL.mode_runs(case):
        rp, cols, cnt, _info, _ = oracle.trace_exchange(flat, args, 8)
        dense.append(H.dense(rp, cols, cnt, flat.n_emitters))
    EL.record("cpu", f"modes/{case}", EL.compare_modes(case, *dense))


def test_open_square_is_the_ray_body_tests_square():
    """emission_laws.open_square(1.0) is test_gpu_ray_body's open-wall square."""
    from test_gpu_ray_body import _open_square

    a, b = EL.open_square().flat(), _open_square().flat()
    for name in ("fine_xy", "fine_nv", "fine_surface", "coarse_solid", "beta", "uniform_beta"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
