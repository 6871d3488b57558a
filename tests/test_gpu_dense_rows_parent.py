"""The dense-row tracers (rthx_trace_exchange_3d, rthx_gasbox_trace) and a
reused 2D result, pinned count for count to a recording
(tests/golden/dense_rows_parent.json).

Both tracers draw from counters (Philox keyed by seed, emitter and ray id), so
one call has one CSR whatever the host does around the launch: row range, row
split, buffer reuse, result reset.  The cases are the smallest shapes on which
each branch of that host sequence runs (split and unsplit rows, 16- and 32-bit
counters, the global tallies, strided and empty emitter ranges, R = 0, a ray
range, a mirrored scene, both sampling modes), and one 2D result traced twice,
the second trace smaller than the first.

Recording anew (on a GPU, by hand, at the commit to pin):
RTHX_RECORD_DENSE_ROWS=1 python -m pytest tests/test_gpu_dense_rows_parent.py
writes what it traced before comparing.  The file notes the ROCm version
it was recorded with: faithful sampling goes through the device math library.
"""
import json
import os

import pytest

import helpers as H
import mirror3d_scenes as M
from rthx import GasBox3D, _lib

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(H.GOLDEN, "dense_rows_parent.json")
INFO = ("nnz", "lost_total", "lost_max_row", "rows_traced", "rays_traced")
SEED = 20261

# name -> (scene, trace keywords, environment knobs)
CASES_3D = {
    "split4_u16": ("cube", dict(R=4096), {}),
    "split4_u16_faithful": ("cube", dict(R=4096, faithful=True), {}),
    "unsplit_u32": ("cube", dict(R=70000), {"RTHX_T3_SPLIT_TARGET": "1"}),
    "ghist": ("cube", dict(R=4096), {"RTHX_T3_GHIST": "1"}),
    "strided": ("cube", dict(R=4096, emitter_begin=3, emitter_stride=5), {}),
    "zero_rows": ("cube", dict(R=4096, emitter_begin=24), {}),
    "zero_rays": ("cube", dict(R=0), {}),
    "mirrored_half": ("half", dict(R=4096), {}),
}
CASES_GAS = {
    "split4_u16": (dict(R=4096), {}),
    "split4_u16_faithful": (dict(R=4096, faithful=True), {}),
    "unsplit_u32": (dict(R=70000), {"RTHX_GASBOX_SPLIT": "1"}),
    "global_tally": (dict(R=16), {}),
    "ray_begin": (dict(R=4096, ray_begin=1000), {}),
    "strided": (dict(R=4096, emitter_begin=3, emitter_end=30, emitter_stride=5), {}),
    "zero_rows": (dict(R=4096, emitter_begin=32), {}),
    "zero_rays": (dict(R=0), {}),
}
GAS_LO, GAS_HI, GAS_N, GAS_BETA = (0.0, 0.0, 0.0), (1.0, 0.9, 0.5), (2, 2, 2), 2.0


def entry(rp, cols, cnt, info):
    return {"row_ptr": [int(x) for x in rp], "cols": [int(x) for x in cols], "counts": [int(x) for x in cnt],
            **{k: int(info[k]) for k in INFO}}


def with_knobs(monkeypatch, knobs, f):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    try:
        return f()
    finally:
        for k in knobs:
            monkeypatch.delenv(k)


def trace_3d(monkeypatch):
    from rthx.trace3d import Scene3D

    xyz, nv, nrm, groups, _n_hull = H.box_scene([[0.0, 0.5, 1.0]] * 3)
    half = M.boxed((0,))
    n = half["n_part"]
    scenes = {"cube": Scene3D(xyz, nv, nrm, groups=groups),
              "half": Scene3D(half["xyz"][:n], half["nv"][:n], half["normals"][:n], mirrors=half["mirrors"])}
    try:
        assert scenes["cube"].n == 24 and scenes["cube"].stats()["hull"]
        assert scenes["half"].mirrors()["n_mirror"] == 1
        out = {}
        for name, (which, kw, knobs) in CASES_3D.items():
            kw = dict(kw)
            R = kw.pop("R")
            out[name] = entry(*with_knobs(monkeypatch, knobs, lambda: scenes[which].trace(R, seed=SEED, **kw)))
        return out
    finally:
        for s in scenes.values():
            s.close()


def trace_gas(monkeypatch):
    box = GasBox3D(GAS_LO, GAS_HI, GAS_N, kappa=GAS_BETA)
    try:
        assert box.num_elements == 32 and box.beta == GAS_BETA
        out = {}
        for name, (kw, knobs) in CASES_GAS.items():
            kw = dict(kw)
            R = kw.pop("R")
            res = with_knobs(monkeypatch, knobs, lambda: box.trace(R, seed=SEED, **kw))
            try:
                out[name] = entry(*res.csr(), res.info())
            finally:
                res.close()
        return out
    finally:
        box.close()


def trace_2d_reused():
    """The 3 x 3 square traced into one result twice: every emitter with a
    recorded ray set, then a strided part of them with none."""
    flat = H.square_domain(ndim=3).flat()
    dd = _lib.DeviceDomain(flat, 0)
    res = _lib.DeviceResult()
    try:
        out = {}
        first, _keep = _lib.make_args(0, 3000, H.NUDGE, SEED, 0, flat.n_emitters, record_ids=[0, 5])
        second, _ = _lib.make_args(0, 1000, H.NUDGE, SEED, 2, 11, 3)
        for name, args in (("first", first), ("second", second)):
            res.trace(dd, args)
            info = res.info()
            out[name] = entry(*res.csr(), info)
            out[name]["n_recorded"] = int(info["n_recorded"])
        return out
    finally:
        res.close()
        dd.close()


def traced(monkeypatch):
    return {"trace3d": trace_3d(monkeypatch), "gasbox": trace_gas(monkeypatch), "trace2d_reused": trace_2d_reused()}


def rocm_version():
    import torch

    return str(torch.version.hip)


@pytest.fixture(scope="module")
def now(hip):
    """Every case traced once; with RTHX_RECORD_DENSE_ROWS=1 also written out
    as the recording (the recorder: run by hand, at the commit to pin)."""
    mp = pytest.MonkeyPatch()
    try:
        got = traced(mp)
    finally:
        mp.undo()
    print(f"recorded with ROCm {H.golden('dense_rows_parent.json')['rocm'] if os.path.exists(GOLDEN) else '-'}, "
          f"running {rocm_version()}")
    if os.environ.get("RTHX_RECORD_DENSE_ROWS") == "1":
        with open(GOLDEN, "w") as fh:
            json.dump({"rocm": rocm_version(), "seed": SEED, **got}, fh, separators=(",", ":"))
            fh.write("\n")
    return got


@pytest.mark.parametrize("family,name", [(f, n) for f, cases in (("trace3d", CASES_3D), ("gasbox", CASES_GAS),
                                                               ("trace2d_reused", ("first", "second")))
                                         for n in cases])
def test_counts_are_the_recorded_ones(now, family, name):
    want, got = H.golden("dense_rows_parent.json")[family][name], now[family][name]
    for k in INFO + (("n_recorded",) if family == "trace2d_reused" else ()):
        assert got[k] == want[k], (k, got[k], want[k])
    assert got["row_ptr"] == want["row_ptr"]
    n_rows = len(want["row_ptr"]) - 1
    for i in range(n_rows):  # (row by row: a failure names the row that moved)
        b, e = want["row_ptr"][i], want["row_ptr"][i + 1]
        assert got["cols"][b:e] == want["cols"][b:e], f"columns of row {i}"
        assert got["counts"][b:e] == want["counts"][b:e], f"counts of row {i}"


def test_the_cases_take_the_branches_they_name(now):
    """Closure and shape of the recorded cases (what each is there for)."""
    t3, gas, d2 = now["trace3d"], now["gasbox"], now["trace2d_reused"]
    assert t3["split4_u16"]["rays_traced"] == 24 * 4096 and t3["unsplit_u32"]["rays_traced"] == 24 * 70000
    assert t3["ghist"]["counts"] == t3["split4_u16"]["counts"] and t3["ghist"]["cols"] == t3["split4_u16"]["cols"]
    assert t3["strided"]["rows_traced"] == len(range(3, 24, 5))
    assert t3["zero_rows"]["rows_traced"] == 0 and t3["zero_rows"]["nnz"] == 0
    assert t3["zero_rays"]["rays_traced"] == 0 and t3["zero_rays"]["nnz"] == 0
    assert t3["mirrored_half"]["rows_traced"] == 60 and t3["mirrored_half"]["lost_total"] == 0
    assert gas["split4_u16"]["rays_traced"] == 32 * 4096 and sum(gas["split4_u16"]["counts"]) == 32 * 4096
    assert sum(gas["unsplit_u32"]["counts"]) == 32 * 70000 and sum(gas["global_tally"]["counts"]) == 32 * 16
    assert gas["ray_begin"]["counts"] != gas["split4_u16"]["counts"]
    assert gas["strided"]["rows_traced"] == len(range(3, 30, 5))
    assert gas["zero_rows"]["rows_traced"] == 0 and gas["zero_rays"]["nnz"] == 0
    assert d2["first"]["n_recorded"] > 0 and d2["second"]["n_recorded"] == 0
    assert d2["second"]["rows_traced"] == len(range(2, 11, 3)) and d2["second"]["rays_traced"] == 3 * 1000
