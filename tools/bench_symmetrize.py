"""Device time of the CSR symmetrisation (rthx_csr_symmetrize)
and of the sparse smoothing set-up built on it, against the HBM copy bound.

  python tools/bench_symmetrize.py [--reps 5] [--only synth,traced] [--ndim 301] [--rays 1e8] [--out FILE]
  RTHX_LIB=<librthx.so> python tools/bench_symmetrize.py --only traced [--reps 1]

One JSON line per case:
  synth   `device_ms` (hipEvents around the transpose and symmetrise kernels,
          with the read of X's size between them) of rthx_csr_symmetrize at
          the synthetic case of profiles/round10/transpose.json: n = 20000,
          1200 distinct random columns per row (density 6 %), random weights;
          median and spread of --reps after one warm-up call.
  traced  rthx_smooth_F_result on a traced sparse case of user size: the
          --ndim x --ndim grey square (default 301: N = 91,805)
          at --rays rays, whole matrix, traced once and smoothed --reps times:
          `x_build_ms` (the X build alone), `ms_ap` (the build and AP) and
          `ms_total` of every repeat, and the CRC-32 of the last repeat's
          F_smooth (row offsets, columns, value bytes).  With RTHX_LIB naming
          an older library that lacks rthx_smooth_get_build (its X is built on
          the host) the line carries ms_ap and ms_total only -- run once per
          library in the same GPU call to compare two builds.
The bound of either is the minimum traffic -- A read once (a column and a
payload per entry: 12 B for values, 8 B for counts) and X written once (12 B
per entry), and both offset arrays -- at the device's measured copy rate
(profiles/round1/hbm_probe.json "copy", 4.8 TB/s); `share_of_copy_bound` is
bound / measured.
"""
import argparse
import ctypes as C
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "raytraceheattransfer.jl_amd"), os.path.join(ROOT, "tests"), ROOT]

COPY_TBS = 4.8  # profiles/round1/hbm_probe.json, pattern "copy"
NUDGE = 10_000 * np.finfo(np.float64).eps


def lib_name():
    from rthx import _lib

    return os.path.relpath(os.environ.get("RTHX_LIB", _lib.LIB_PATH), ROOT)


def spread(ts):
    return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
            "spread_ms": round(max(ts) - min(ts), 4)}


def case_synth(reps, n=20000, per_row=1200):
    from rthx import _lib, abi

    lib = _lib.load()
    rng = np.random.default_rng(41)
    ci = np.empty((n, per_row), dtype=np.int32)
    for r0 in range(0, n, 500):  # per_row distinct columns per row, ascending
        keys = rng.random((min(500, n - r0), n))
        ci[r0:r0 + 500] = np.sort(np.argpartition(keys, per_row, axis=1)[:, :per_row], axis=1)
    ci = ci.ravel()
    rp = np.arange(0, n * per_row + 1, per_row, dtype=np.int64)
    vv = rng.random(n * per_row)
    w = np.exp(rng.uniform(0.0, np.log(50.0), n))
    nnz = int(rp[-1])
    cap = 2 * nnz
    xrp = np.empty(n + 1, np.int64)
    xci = np.empty(cap, np.int32)
    xv = np.empty(cap)
    xnnz, ms = C.c_int64(0), C.c_double(0.0)
    ts = []
    for it in range(reps + 1):
        _lib.check(lib.rthx_csr_symmetrize(0, n, abi.ptr(rp, C.c_int64), abi.ptr(ci, C.c_int32),
                                           abi.ptr(vv, C.c_double), abi.ptr(w, C.c_double), cap,
                                           abi.ptr(xrp, C.c_int64), abi.ptr(xci, C.c_int32), abi.ptr(xv, C.c_double),
                                           C.byref(xnnz), C.byref(ms)))
        if it:
            ts.append(ms.value)
    k = xnnz.value
    assert xrp[0] == 0 and xrp[-1] == k and nnz <= k <= cap and np.all(np.diff(xrp) > 0)
    min_bytes = 12 * nnz + 12 * k + 16 * (n + 1)
    bound_ms = min_bytes / (COPY_TBS * 1e12) * 1e3
    out = {"case": "synth_n20000_density_6pct", "lib": lib_name(), "build_id": _lib.build_id(), "n": n, "nnz": nnz,
           "x_nnz": k, "reps": reps, "device_ms": [round(t, 4) for t in ts]}
    out.update(spread(ts))
    out.update({"min_bytes": min_bytes, "copy_bound_ms": round(bound_ms, 4),
                "share_of_copy_bound": round(bound_ms / float(np.median(ts)), 4)})
    return out


def case_traced(reps, ndim, rays):
    import bench
    from rthx import _lib, abi
    from rthx.smoothing import get_w

    lib = _lib.load()
    dom = bench.build_domain(ndim)
    flat = dom.flat()
    N = flat.n_emitters
    R = max(int(rays) // N, 1)
    args, _k = _lib.make_args(0, R, NUDGE, 1, 0, N, 1, flags=abi.RTHX_FLAG_DEVICE_ONLY)
    dd = _lib.DeviceDomain(flat, 0)
    res = _lib.DeviceResult()
    w = np.ascontiguousarray(get_w(dom))
    has_build = hasattr(lib, "rthx_smooth_get_build")
    rows, crc = [], None
    try:
        res.trace(dd, args)
        nnz = res.info()["nnz"]
        for _ in range(reps):
            a = abi.SmoothArgs()
            a.device, a.max_iters, a.k_dykstra, a.renorm = 0, 1000, -1, 1
            h = C.c_void_p()
            _lib.check(lib.rthx_smooth_F_result(res.handle, N, abi.ptr(w, C.c_double), N, dom.num_surfaces,
                                                C.byref(a), C.byref(h)))
            inf = abi.SmoothInfo()
            on, bms = C.c_int32(0), C.c_double(0.0)
            try:
                _lib.check(lib.rthx_smooth_get_info(h, C.byref(inf)))
                if has_build:
                    _lib.check(lib.rthx_smooth_get_build(h, C.byref(on), C.byref(bms)))
                if not inf.dense and len(rows) == reps - 1:  # the last repeat's F_smooth, for its checksum
                    orp = np.empty(N + 1, np.int64)
                    oci = np.empty(max(inf.nnz, 1), np.int32)
                    ov = np.empty(max(inf.nnz, 1))
                    _lib.check(lib.rthx_smooth_copy_csr(h, abi.ptr(orp, C.c_int64), abi.ptr(oci, C.c_int32),
                                                        abi.ptr(ov, C.c_double)))
                    crc = zlib.crc32(ov, zlib.crc32(oci, zlib.crc32(orp)))
            finally:
                lib.rthx_smooth_destroy(h)
            assert not inf.dense
            rows.append((inf.ms_total, inf.ms_ap, bms.value, on.value, inf.nnz, inf.ap_iters, inf.converged))
    finally:
        res.close()
        dd.close()
    x_nnz = int(rows[0][4])
    min_bytes = 8 * nnz + 12 * x_nnz + 16 * (N + 1)
    bound_ms = min_bytes / (COPY_TBS * 1e12) * 1e3
    out = {"case": "traced_square%d" % ndim, "lib": lib_name(), "build_id": _lib.build_id(), "N": N,
           "rays_per_emitter": R, "rays": R * N, "nnz": int(nnz), "x_nnz": x_nnz, "ap_iters": int(rows[0][5]),
           "converged": int(rows[0][6]), "f_smooth_crc32": crc,
           "x_on_device": int(rows[0][3]) if has_build else None, "reps": reps,
           "ms_total": [round(r[0], 3) for r in rows], "ms_ap": [round(r[1], 3) for r in rows]}
    out.update({"ms_total_" + k: v for k, v in spread([r[0] for r in rows]).items()})
    if has_build:
        xb = [r[2] for r in rows]
        out["x_build_ms"] = [round(t, 3) for t in xb]
        out.update({"x_build_" + k: v for k, v in spread(xb).items()})
        out.update({"min_bytes": min_bytes, "copy_bound_ms": round(bound_ms, 4),
                    "share_of_copy_bound": round(bound_ms / float(np.median(xb)), 4)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="synth,traced")
    ap.add_argument("--ndim", type=int, default=301)
    ap.add_argument("--rays", type=float, default=1e8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for name in a.only.split(","):
        line = case_synth(a.reps) if name == "synth" else case_traced(a.reps, a.ndim, a.rays)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
