"""Device time of rthx_result_accumulate against the HBM copy bound.

  python tools/bench_accumulate.py [--rays 1e8] [--steps 5] [--only C2,C5] [--out FILE]

C2: the 101x101 grey square, two halves of --rays / 2 (ray ids [0, R/2) and
[R/2, R) of every emitter); C5: band 0 of the 201x201 8-band greenhouse, the
same two halves.  Each step traces the first half anew and adds the
second half's result to it; the time is the accumulate's own (hipEvents around
its kernels, rthx_result_accumulate_ms), best of --steps.

The bound: the sum must read both operands and write the result once, 8 B per
entry (a column and a count), at the device's measured copy rate
(profiles/round1/hbm_probe.json "copy", 4.8 TB/s; k_shard_copy reaches 3.9
TB/s).  The kernels move more than that minimum -- the columns
are read twice and a 4-byte rank per added entry is written and read -- so
the JSON gives both: `min_bytes` / `share_of_copy_bound` for the minimum
traffic, and `moved_bytes` for what the three passes actually move.
One JSON line per case.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "raytraceheattransfer.jl_amd"), os.path.join(ROOT, "tests"), ROOT]
import helpers as H  # noqa: E402
from rthx import _lib  # noqa: E402

COPY_TBS = 4.8  # profiles/round1/hbm_probe.json, pattern "copy"


def run(name, dom, bin0, R, steps):
    flat = dom.flat()
    N = flat.n_emitters
    dd = _lib.DeviceDomain(flat, 0)
    half = R // 2
    flags = _lib.abi.RTHX_FLAG_DEVICE_ONLY
    a0, _k0 = _lib.make_args(bin0, half, H.NUDGE, 1, 0, N, 1, flags=flags)
    a1, _k1 = _lib.make_args(bin0, R - half, H.NUDGE, 1, 0, N, 1, flags=flags)
    first, second = _lib.DeviceResult(), _lib.DeviceResult()
    try:
        second.trace(dd, a1, ray_begin=half)
        nnz_b = second.info()["nnz"]
        best = None
        for _ in range(steps + 1):  # (the first step sizes the buffers)
            first.trace(dd, a0)
            nnz_a = first.info()["nnz"]
            first.accumulate(second)
            ms = first.accumulate_ms()
            best = ms if best is None else min(best, ms)
        nnz = first.info()["nnz"]
        err = first.sampling_error()
    finally:
        first.close()
        second.close()
        dd.close()
    min_bytes = 8 * (nnz_a + nnz_b + nnz)
    moved = 4 * (nnz_a + nnz_b) + 4 * nnz_b + 8 * (nnz_a + nnz_b) + 4 * nnz_b + 8 * nnz
    bound_ms = min_bytes / (COPY_TBS * 1e12) * 1e3
    return {"case": name, "n_emitters": N, "rays_per_emitter": R, "nnz_a": nnz_a, "nnz_b": nnz_b, "nnz_sum": nnz,
            "accumulate_ms": round(best, 4), "min_bytes": min_bytes, "moved_bytes": moved,
            "achieved_tb_per_s_min_bytes": round(min_bytes / (best * 1e-3) / 1e12, 3),
            "achieved_tb_per_s_moved_bytes": round(moved / (best * 1e-3) / 1e12, 3),
            "bound": f"HBM copy at {COPY_TBS} TB/s over min_bytes (read both operands, write the sum, 8 B per entry)",
            "bound_ms": round(bound_ms, 4), "share_of_copy_bound": round(bound_ms / best, 3),
            "rms_sampling_error": err[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=float, default=1e8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--only", default="C2,C5")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []
    if "C2" in a.only:
        dom = H.square_domain(101)
        lines.append(run("C2 two halves", dom, 0, int(a.rays) // dom.flat().n_emitters, a.steps))
    if "C5" in a.only:
        dom = H.greenhouse_domain()
        lines.append(run("C5 band 0 two halves", dom, 0, int(a.rays) // dom.flat().n_emitters, a.steps))
    for ln in lines:
        print(json.dumps(ln), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
