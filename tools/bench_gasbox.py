"""Throughput of the 3D gas-box exchange tracer (diagnostic,
bench.py's headline is the 2D tracer).  One MI355X.

A cube of n^3 voxels (32: N = 6144 + 32768 = 38912 elements), the whole
matrix, optical thickness beta * L = 1, --rays-per-emitter rays an emitter
(1000).  Blocking device-only calls into one reused result, so the buffers are
sized once; per call the kernel time from the call's device events (trace_ms:
the trace kernel alone), the time of the kernels that turn the dense rows into
the CSR (pack_ms) and the host wall time of the whole call (total_ms, which
also holds the clearing of the dense rows).  Medians over --steps calls after
--warmup.  Grays/s = rays traced / time.

--field times the per-voxel tracer (rthx_gasbox_trace_field)
beside it in the same process: the uniform kernel, then the lattice walk
through a uniform array of the same beta (the same rays: what the walk itself
costs), then through a 10:1 checkerboard (beta and beta / 10 in alternate
voxels).  One JSON line with the three timings and the walk's ratios to the
uniform kernel.

  python tools/bench_gasbox.py [--n 32] [--rays-per-emitter 1000] [--field] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytraceheattransfer.jl_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--rays-per-emitter", type=int, default=1000)
    ap.add_argument("--optical-thickness", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--faithful", action="store_true")
    ap.add_argument("--field", action="store_true", help="also time the per-voxel tracer (uniform array, 10:1 checkerboard)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from rthx import GasBox3D, VoxelGasBox3D, _lib

    _lib.load().rthx_device_synchronize(0)
    R = args.rays_per_emitter

    def timed(box, **kw):
        """Medians over --steps blocking calls after --warmup, into one reused result."""
        res = None
        for _ in range(args.warmup):
            res = box.trace(R, seed=1, faithful=args.faithful, result=res, **kw)
        ms = {"trace_ms": [], "pack_ms": [], "total_ms": []}
        for step in range(args.steps):
            res = box.trace(R, seed=2 + step, faithful=args.faithful, result=res, **kw)
            info = res.info()
            for k in ms:
                ms[k].append(info[k])
        rays = info["rays_traced"]
        med = {k: float(np.median(v)) for k, v in ms.items()}
        res.close()
        return {"rays": rays, "nnz": info["nnz"], "lost_total": info["lost_total"],
                **{k: round(v, 4) for k, v in med.items()},
                "trace_ms_min_max": [round(min(ms["trace_ms"]), 4), round(max(ms["trace_ms"]), 4)],
                "grays_per_s_kernel": round(rays / med["trace_ms"] / 1e6, 3),
                "grays_per_s_call": round(rays / med["total_ms"] / 1e6, 3)}

    box = GasBox3D((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (args.n,) * 3, kappa=args.optical_thickness)
    out = {"n": args.n, "n_elements": box.num_elements, "rays_per_emitter": R, "beta": box.beta,
           "faithful": bool(args.faithful), "build_id": _lib.build_id(), "steps": args.steps, "warmup": args.warmup}
    uniform = timed(box)
    box.close()
    if not args.field:
        out.update(uniform)
    else:
        cx, cy, cz = np.meshgrid(*[np.arange(args.n)] * 3, indexing="ij")
        checker = np.where((cx + cy + cz) % 2 == 0, args.optical_thickness, 0.1 * args.optical_thickness)
        vox = VoxelGasBox3D((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (args.n,) * 3, kappa=args.optical_thickness)
        fields = {"walk_uniform_array": timed(vox), "walk_checkerboard_10_to_1": timed(vox, beta=checker)}
        vox.close()
        for f in fields.values():
            f["kernel_time_over_uniform_kernel"] = round(f["trace_ms"] / uniform["trace_ms"], 3)
            f["call_time_over_uniform_kernel"] = round(f["total_ms"] / uniform["total_ms"], 3)
        out.update({"uniform_kernel": uniform, **fields})
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
