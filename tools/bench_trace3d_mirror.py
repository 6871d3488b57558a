"""What a symmetry-plane model costs on the 3D trace alone (DESIGN.md §7k;
diagnostic, bench.py's headline is the 2D tracer).  One MI355X.

The empty unit cube, ndim x ndim quads per face (11: 726 quads), with face
groups:
  whole   traced whole on its fast path (the box hull);
  half    its x <= 0.5 half behind one mirror (the cells the plane cuts become
          half cells);
  octant  its x, y, z <= 0.5 octant behind three mirrors.
Every leg traces the same rays per emitter (rays / n_whole), blocking
device-only calls; kernel time from the call's device events (trace_ms),
median over --steps calls after --warmup, the legs visited --visits times in
turn.  Grays/s = rays traced / kernel time.

  python tools/bench_trace3d_mirror.py [--ndim 11] [--rays 1e8] [--out FILE.json]
      [--parent-lib PATH/librthx.so]   # the whole cube again with another build of
                                       # the library, in a child process of this call
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytraceheattransfer.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import helpers as H  # noqa: E402


def part_scene(ndim, axes):
    """The cube's part at x_k <= 0.5 (k in axes): the box over the cut lattice
    lines without its faces on the cutting planes, and one oversized mirror
    quad per plane."""
    full = np.linspace(0.0, 1.0, ndim + 1)
    cut = np.append(full[full < 0.5 - 1e-12], 0.5)
    xyz, nv, nrm, g, _nh = H.box_scene([cut if k in axes else full for k in range(3)])
    keep = np.ones(len(nv), dtype=bool)
    mirrors = []
    for k in axes:
        keep &= ~np.all(xyz[:, :, k] == 0.5, axis=1)
        u, v = (k + 1) % 3, (k + 2) % 3
        q = np.zeros((4, 3))
        q[:, k] = 0.5
        q[:, u] = [-0.25, 1.25, 1.25, -0.25]
        q[:, v] = [-0.25, -0.25, 1.25, 1.25]
        mirrors.append(q)
    mir = (np.array(mirrors), np.full(len(mirrors), 4, dtype=np.int32)) if mirrors else None
    return np.ascontiguousarray(xyz[keep]), nv[keep], np.ascontiguousarray(nrm[keep]), g[keep], mir


LEGS = {"whole": (), "half": (0,), "octant": (0, 1, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ndim", type=int, default=11)
    ap.add_argument("--rays", type=float, default=1e8, help="rays of the whole cube (sets the rays per emitter)")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--visits", type=int, default=2)
    ap.add_argument("--legs", default="whole,half,octant")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from rthx import _lib
    from rthx.trace3d import Scene3D

    _lib.load().rthx_device_synchronize(0)
    R = int(args.rays) // (6 * args.ndim * args.ndim)
    out = {"ndim": args.ndim, "rays_per_emitter": R, "build_id": _lib.build_id(), "legs": {}}
    scenes = {}
    for leg in args.legs.split(","):
        xyz, nv, nrm, g, mir = part_scene(args.ndim, LEGS[leg])
        kw = {} if mir is None else {"mirrors": mir}  # (a parent library's Scene3D path takes no mirrors)
        s = Scene3D(xyz, nv, nrm, groups=g, **kw)
        scenes[leg] = s
        out["legs"][leg] = {"n": len(nv), "mirrors": 0 if mir is None else len(mir[1]), "rays": len(nv) * R,
                            "hull_mode": s.stats().get("hull_mode"), "trace_ms": [], "grays_per_s": []}
    for _visit in range(args.visits):
        for leg, s in scenes.items():
            for _ in range(args.warmup):
                s.trace(R, device_only=True)
            ms = []
            for _ in range(args.steps):
                _, _, _, info = s.trace(R, device_only=True)
                ms.append(info["trace_ms"])
            rec = out["legs"][leg]
            k = float(np.median(ms))
            rec["trace_ms"].append(round(k, 4))
            rec["grays_per_s"].append(round(rec["rays"] / k / 1e6, 3))
            rec["lost_total"] = int(info["lost_total"])
    for s in scenes.values():
        s.close()
    if args.parent_lib:  # the whole cube with the other build, in a fresh process
        env = dict(os.environ, RTHX_LIB=os.path.abspath(args.parent_lib))
        cmd = [sys.executable, os.path.abspath(__file__), "--ndim", str(args.ndim), "--rays", str(args.rays), "--steps",
               str(args.steps), "--warmup", str(args.warmup), "--visits", str(args.visits), "--legs", "whole"]
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            raise SystemExit(f"the parent-library run failed ({p.returncode}): {p.stderr[-2000:]}")
        out["parent"] = json.loads(p.stdout.strip().splitlines()[-1])
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
