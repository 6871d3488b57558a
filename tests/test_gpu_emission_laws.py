"""The device's recorded rays against the analytic laws of emission and free
paths (tests/emission_laws.py): the cases, seeds and statistics of
tests/test_emission_laws.py, on the rays rthx_result_copy_rays hands back.

Each case also compares the device's rays with the CPU restatement's
(origins to 1e-12, end points to 1e-9, as test_gpu_parity.test_recorder_exact
does), so the device's p-values are the restatement's and a deviation on the
device alone points at the kernel.
"""
import numpy as np
import pytest

import emission_laws as EL

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("flags", [0, EL.FAITHFUL], ids=["default", "faithful"])
@pytest.mark.parametrize("case,key", EL.LAW_EMITTERS, ids=EL.LAW_IDS)
def test_device_rays_obey_the_laws(hip, case, key, flags):
    flat, g, args, _keep = EL.law_args(case, key, flags)
    dd = hip.DeviceDomain(flat, 0)
    res = hip.DeviceResult()
    try:
        res.trace(dd, args)
        info = res.info()
        rp, cols, cnt = res.csr()
        rays = res.rays()
    finally:
        res.close()
        dd.close()
    EL.check_row(flat, g, rp, cols, cnt, info, rays)
    o, e, _g = rays  # (one emitter: in ray order on both sides)
    ro, re = EL.restatement_rays(case, key, flags)
    assert np.allclose(o, ro, rtol=0, atol=1e-12)
    assert np.allclose(e, re, rtol=0, atol=1e-9)
    p = EL.laws(flat, g, o, e)
    c = EL.controls(flat, g, o, e)
    print(f"{case} {key} flags {flags}: laws {p}\ncontrols {c}")
    EL.record("gpu", f"laws/{case}/{key}/{'faithful' if flags else 'default'}", {"laws": p, "controls": c})
    for name, v in p.items():
        assert v >= EL.P_BOUND, (name, v)
    for name, v in c.items():
        assert v < EL.P_BOUND, (name, v)
