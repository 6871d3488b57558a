"""Spectral GERT solve on the device (rthx_solve_spectral):
whole-solve time and iteration counts, and the banded operator's time per
call against the same K products as K launches of the grey operator (what a
caller had before the banded apply), for K = 8 distinct dense band matrices
and for one shared matrix, on the 41x41 (n = 1845) and 101x101 (n = 10605)
unit squares.  Writes profiles/round8/spectral_solve.json.

  python tools/bench_spectral_solve.py [--ndims 41 101] [--rays 1e8] [--reps 30]

Apply times are HIP-event times of single calls after warm-up (median and
interquartile range); rates are against the 4.8 TB/s copy rate of
profiles/round1/hbm_probe.json.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytraceheattransfer.jl_amd"))

from rthx import PolyVolume2D, RayTracingDomain2D, abi  # noqa: E402
from rthx._lib import check, load  # noqa: E402
from rthx.equilibrium import _band_struct, populate_workspace, solve_spectral  # noqa: E402

K = 8
LIMITS = np.logspace(-7, -3, K + 1)
COPY_RATE = 4.8e12  # B/s, profiles/round1/hbm_probe.json "copy"


def square(ndim, kappa, eps):
    face = PolyVolume2D([(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)], [True] * 4, K,
                        np.broadcast_to(np.asarray(kappa, dtype=np.float64), (K,)).copy(), np.zeros(K))
    face.epsilon = [np.broadcast_to(np.asarray(eps, dtype=np.float64), (K,)).copy() for _ in range(4)]
    face.T_in_w = [1000.0, 300.0, 300.0, 300.0]
    face.T_in_g = -1.0
    dom = RayTracingDomain2D([face], [(ndim, ndim)])
    dom.wavelength_band_limits = LIMITS
    return dom


def arrays(dom):
    wss = [populate_workspace(dom, k) for k in range(1, K + 1)]
    b = np.array([np.concatenate([1.0 - ws["epsw"], ws["omega_g"]]) for ws in wss])
    prop = np.array([np.concatenate([ws["epsw"], ws["kappa_g"]]) for ws in wss])
    size = np.concatenate([wss[0]["Area"], 4.0 * wss[0]["Volume"]])
    return b, prop, size, np.concatenate([wss[0]["Tw"], wss[0]["Tg"]]), np.concatenate([wss[0]["qw"], wss[0]["qg"]])


def dense(F):
    return np.ascontiguousarray(F.toarray() if hasattr(F, "toarray") else F, dtype=np.float64)


def apply_times(mats, n, n_bands, mode, reps):
    """HIP-event ms of `reps` single calls: mode 0 the banded apply, mode 1
    n_bands launches of the grey operator (rthx_debug_spectral_apply_times)."""
    lib = load()
    lib.rthx_debug_spectral_apply_times.argtypes = [C.POINTER(abi.SpectralBand), C.c_int32, C.c_int64, C.c_int32,
                                                    C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                    C.POINTER(C.c_double)]
    keep = []
    bands = (abi.SpectralBand * len(mats))(*[_band_struct(m, n, None, keep) for m in mats])
    ms = np.zeros(reps)
    check(lib.rthx_debug_spectral_apply_times(bands, len(mats), n, n_bands, 0, mode, 5, reps, abi.ptr(ms, C.c_double)))
    q1, med, q3 = np.percentile(ms, [25, 50, 75])
    return {"median_ms": float(med), "q1_ms": float(q1), "q3_ms": float(q3), "calls": reps}


def solve(mats, dom):
    b, prop, size, T_in, q_in = arrays(dom)
    t = time.perf_counter()
    j, g, T, e, info = solve_spectral(mats, LIMITS, b, prop, size, T_in, q_in)
    wall = time.perf_counter() - t
    return {"wall_ms": wall * 1e3, "library_ms": info["ms_total"], "apply_ms": info["ms_apply"],
            "outer_iterations": info["outer_iterations"], "gmres_iterations": info["gmres_iterations"],
            "converged": info["converged"], "change": info["change"], "residual": info["residual"],
            "T_gas_min": float(T[dom.num_surfaces:].min()), "T_gas_max": float(T[dom.num_surfaces:].max())}


def rate(entry, n, passes):
    entry["bytes"] = passes * n * n * 8
    entry["tb_per_s"] = entry["bytes"] / (entry["median_ms"] * 1e-3) / 1e12
    entry["of_copy_rate"] = entry["tb_per_s"] * 1e12 / COPY_RATE
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ndims", type=int, nargs="+", default=[41, 101])
    ap.add_argument("--rays", type=float, default=1e8)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "round8", "spectral_solve.json"))
    a = ap.parse_args()
    out = {"K": K, "limits": LIMITS.tolist(), "rays_per_band": a.rays, "copy_rate_tb_per_s": COPY_RATE / 1e12,
           "sizes": []}
    for ndim in a.ndims:
        # K distinct matrices: kappa_k spread over the bands, reflecting walls
        dom = square(ndim, np.geomspace(0.3, 3.0, K), 0.8)
        dom(int(a.rays), seed=1, verbose=False)
        n = dom.num_emitters
        mats = [dense(F)[:n, :n] for F in dom.F_smooth]
        dom.F_smooth = None
        rec = {"ndim": ndim, "n": n, "distinct": {"solve": solve(mats, dom)}}
        d = rec["distinct"]
        d["banded_apply"] = rate(apply_times(mats, n, K, 0, a.reps), n, K)
        d["sequential_grey_applies"] = rate(apply_times(mats, n, K, 1, a.reps), n, K)
        d["banded_not_slower"] = bool(d["banded_apply"]["q1_ms"] <= d["sequential_grey_applies"]["q3_ms"])
        print(json.dumps({"ndim": ndim, "n": n, "distinct": d}), flush=True)
        del mats
        # one shared matrix: uniform kappa, band-selective walls
        dom = square(ndim, 1.0, np.linspace(0.3, 0.9, K))
        dom(int(a.rays), seed=2, verbose=False)
        shared = [dense(dom.F_smooth[0])[:n, :n]]
        dom.F_smooth = None
        s = rec["shared"] = {"solve": solve(shared[0], dom)}
        s["banded_apply"] = rate(apply_times(shared, n, K, 0, a.reps), n, 1)
        s["one_grey_apply"] = rate(apply_times(shared, n, 1, 1, a.reps), n, 1)
        s["sequential_grey_applies"] = rate(apply_times(shared, n, K, 1, a.reps), n, K)
        s["banded_not_slower"] = bool(s["banded_apply"]["q1_ms"] <= s["sequential_grey_applies"]["q3_ms"])
        t1, tK, tb = (s[k]["median_ms"] for k in ("one_grey_apply", "sequential_grey_applies", "banded_apply"))
        s["reads_F_once"] = bool(abs(tb - t1) < abs(tb - tK))  # closer to one grey apply than to K
        print(json.dumps({"ndim": ndim, "n": n, "shared": s}), flush=True)
        out["sizes"].append(rec)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
