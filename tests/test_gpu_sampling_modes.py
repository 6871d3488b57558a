"""Default sampling against faithful sampling on the device, count for count.

The headline kernels cannot record a ray -- the LAT rows and their
closed-lattice copy, kEmitVolRect, the MLAT / CLDS kernels -- and faithful
sampling never runs them, so tests/test_gpu_emission_laws.py does not reach
them.  Here whole small domains are traced twice on the device, with default
sampling at seed 101 and with faithful sampling at seed 202, R = 2e5 rays an
emitter, and all rows of the two count matrices are compared by the
two-sample homogeneity statistic (helpers.homogeneity, min_bin = 40):

    chi2.ppf(1e-7, dof) <= X2 <= chi2.isf(1e-7, dof)

(two independent seeds must not agree too well either).  The control: the
faithful side traced again with every kappa x 1.02 must be told apart.  The
acceptance is emission_laws.compare_modes.

Measured on the CPU restatement, z = (X2 - dof) / sqrt(2 dof) [control]:
square5 -1.17 [12.6], rotated5 -0.12 [13.4], wedges -0.41 [17.9],
quad_lattice -0.20 [11.9], open5 +0.95 [12.2] (lost totals 1142737 and
1141396, 1.0 sigma apart), layered_slab -0.28 [34.4]; dof 1485 to 10840.
The device draws the restatement's rays, so these are its figures too.
"""
import ctypes as C

import pytest

import emission_laws as EL
import helpers as H

pytestmark = pytest.mark.gpu


def _lat_plain(hip, dd):
    """rthx_debug_lat_plain of the domain (tests/test_gpu_closed_lattice.py):
    1 the closed-lattice copy, 0 the general copy, -1 without the lattice."""
    f = hip.load().rthx_debug_lat_plain
    f.argtypes = [C.c_void_p]
    f.restype = C.c_int
    return f(dd.handle)


@pytest.mark.parametrize("case", list(EL.MODE_CASES))
def test_sampling_modes_agree_count_for_count(hip, case):
    dense = []
    for name, flat, args, _keep in EL.mode_runs(case):
        dd = hip.DeviceDomain(flat, 0)
        res = hip.DeviceResult()
        try:
            if case == "square5" and name == "default":
                # the headline path: the case cannot silently move off it
                assert _lat_plain(hip, dd) == 1
            res.trace(dd, args)
            info = res.info()
            assert info["rays_traced"] == flat.n_emitters * EL.R_MODES
            dense.append(H.dense(*res.csr(), flat.n_emitters))
            assert int(dense[-1].sum()) + info["lost_total"] == info["rays_traced"]
        finally:
            res.close()
            dd.close()
    EL.record("gpu", f"modes/{case}", EL.compare_modes(case, *dense, closed=case != "open5"))

