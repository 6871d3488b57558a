"""Device time of the CSR transpose (rthx_csr_transpose) against
the HBM copy bound, and the seam's device transpose alone for A/B runs.

  python tools/bench_transpose.py [--reps 5] [--only c2,smooth] [--out FILE]
  RTHX_LIB=<librthx.so> python tools/bench_transpose.py --seam [--reps 9]

Default: `device_ms` (hipEvents around the transpose kernels alone) of
rthx_csr_transpose at two sizes, median and spread of --reps after one
warm-up call:
  c2      F_raw of BASELINE config C2 (the 101x101 grey square at 1e8 rays:
          N = 10605, about 3.05e7 nonzeros), copied from a trace;
  smooth  a sparse F_smooth the size of a large domain's: the density of
          H.square_domain(41)'s at 200 000 rays (6 %) scaled up to n = 20000
          (1200 random columns per row, ascending).
The bound is the minimum traffic -- every entry (a column and a value, 12 B)
read once and written once, and the offsets written -- at the device's
measured copy rate (profiles/round1/hbm_probe.json "copy", 4.8 TB/s).  The
kernels move more than that (`moved_bytes`: per pass a 4-byte digit read for
the histogram, the records read and written, and the sorted columns for the
offsets), so the JSON gives both.  One JSON line per case.

--seam: rthx_result_copy_F_csc with NULL outputs (the device transpose of the
seam alone, as tools/host_boundary_cost.py --gpu times it) on a C2 trace at
1e8 rays, every repeat listed, for the library named by RTHX_LIB -- run once
per library in the same GPU call to compare two builds.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "raytraceheattransfer.jl_amd"), os.path.join(ROOT, "tests"), ROOT]

COPY_TBS = 4.8  # profiles/round1/hbm_probe.json, pattern "copy"
NUDGE = 10_000 * np.finfo(np.float64).eps


def c2_trace():
    import bench
    from rthx import _lib

    flat = bench.build_domain(101).flat()
    N = flat.n_emitters
    args, _k = _lib.make_args(0, 100_000_000 // N, NUDGE, 1, 0, N, 1, flags=_lib.abi.RTHX_FLAG_DEVICE_ONLY)
    dd = _lib.DeviceDomain(flat, 0)
    res = _lib.DeviceResult()
    res.trace(dd, args)
    return dd, res, N


def seam(reps):
    from rthx import _lib

    lib = _lib.load()
    dd, res, N = c2_trace()
    try:
        nnz = res.info()["nnz"]
        ts = []
        for it in range(reps + 1):  # (the first call sizes the buffers)
            t = time.perf_counter()
            _lib.check(lib.rthx_result_copy_F_csc(res.handle, 1, None, None, None))
            if it:
                ts.append((time.perf_counter() - t) * 1e3)
    finally:
        res.close()
        dd.close()
    return {"case": "seam_csc_device_transpose", "lib": os.path.relpath(os.environ.get("RTHX_LIB", _lib.LIB_PATH), ROOT),
            "build_id": _lib.build_id(), "N": N, "nnz": nnz, "reps": reps, "ms": [round(t, 4) for t in ts],
            "median_ms": round(float(np.median(ts)), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
            "spread_ms": round(max(ts) - min(ts), 4)}


def passes_of(n_cols):
    bits = max(int(n_cols - 1).bit_length(), 1)
    return (bits + 7) // 8


def time_transpose(name, n_rows, n_cols, rp, ci, vv, reps):
    from rthx import _lib, abi

    lib = _lib.load()
    nnz = int(rp[-1])
    trp = np.empty(n_cols + 1, np.int64)
    tci = np.empty(max(nnz, 1), np.int32)
    tv = np.empty(max(nnz, 1))
    ms = C.c_double(0.0)
    ts = []
    for it in range(reps + 1):
        _lib.check(lib.rthx_csr_transpose(0, n_rows, n_cols, abi.ptr(rp, C.c_int64), abi.ptr(ci, C.c_int32),
                                          abi.ptr(vv, C.c_double), abi.ptr(trp, C.c_int64), abi.ptr(tci, C.c_int32),
                                          abi.ptr(tv, C.c_double), C.byref(ms)))
        if it:
            ts.append(ms.value)
    assert trp[0] == 0 and trp[-1] == nnz and np.all(np.diff(trp) >= 0)
    p = passes_of(n_cols)
    min_bytes = 24 * nnz + 8 * (n_cols + 1)
    rec = 16  # column, row, value between passes
    # per pass 4 B for the histogram; CSR read 12 B, records 16 B; the last pass writes row 4, value 8, column 4
    moved = nnz * (4 * p + 12 + 2 * rec * (p - 1) + 16 + 4) + 8 * (n_cols + 1)
    bound_ms = min_bytes / (COPY_TBS * 1e12) * 1e3
    med = float(np.median(ts))
    return {"case": name, "n_rows": n_rows, "n_cols": n_cols, "nnz": nnz, "passes": p, "reps": reps,
            "device_ms": [round(t, 4) for t in ts], "median_ms": round(med, 4),
            "spread_ms": round(max(ts) - min(ts), 4), "min_bytes": min_bytes, "moved_bytes": moved,
            "copy_bound_ms": round(bound_ms, 4), "share_of_copy_bound": round(bound_ms / med, 4),
            "moved_tb_per_s": round(moved / med / 1e9, 3)}


def case_c2(reps):
    dd, res, N = c2_trace()
    try:
        rp, ci, vv = res.F()
        rp, ci, vv = rp.copy(), np.ascontiguousarray(ci), np.ascontiguousarray(vv)
    finally:
        res.close()
        dd.close()
    return time_transpose("c2_F_raw", N, N, rp, ci, vv, reps)


def case_smooth(reps, n=20000, per_row=1200):
    rng = np.random.default_rng(41)
    ci = np.sort(rng.integers(0, n, size=(n, per_row), dtype=np.int32), axis=1).ravel()
    rp = np.arange(0, n * per_row + 1, per_row, dtype=np.int64)
    vv = rng.random(n * per_row)
    return time_transpose("sparse_F_smooth_n20000_density_6pct", n, n, rp, ci, vv, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="c2,smooth")
    ap.add_argument("--seam", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    if a.seam:
        lines.append(seam(max(a.reps, 5)))
    else:
        for name in a.only.split(","):
            lines.append({"c2": case_c2, "smooth": case_smooth}[name](a.reps))
    for line in lines:
        print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
