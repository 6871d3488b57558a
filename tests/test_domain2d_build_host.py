"""The 2D tracer's host-side domain build (csrc/rthx_domain2d_build.h) without
a GPU: tests/domain2d_host_check.cpp, compiled together with
csrc/rthx_domain2d_build.cpp and csrc/rthx_grid.cpp for the host with
AddressSanitizer and UBSan and run as a program.  It checks by brute force what
the kernels' fast paths rely on -- the inverse maps, the padded polygons, the
grids' bookkeeping, the three LDS layouts and their blobs, the lattices'
cell-to-polygon maps, the mirror masks -- and every refusal but one, and prints
one fingerprint a domain.

The fingerprints in tests/golden/domain2d_build.json were recorded when the
builder was still the body of rthx_domain_create moved verbatim into its own
file, before its helpers were merged and it was cut into steps: they pin "the
same domain as before the split"."""
import json
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytraceheattransfer.jl_amd", "csrc")

LINE = re.compile(r"^domain (\S+) hash ([0-9a-f]{16}) single (\d) axis (\d) lat (\d+) (\d+) (-?\d) "
                  r"ml (\d+) (\d+) (\d+) (\d+) (\d+) cl (\d+) cells (\d+)$", re.M)
KEYS = ("single", "axis", "lat_nx", "lat_ny", "lat_identity", "ml_nx", "ml_ny", "ml_ncx", "ml_ncy", "ml_bytes",
        "cl_bytes", "cells")


def test_domain_build_invariants_and_fingerprints(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "domain2d_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "domain2d_host_check.cpp"),
                    os.path.join(CSRC, "rthx_domain2d_build.cpp"),
                    os.path.join(CSRC, "rthx_grid.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout.strip())
    assert out.returncode == 0, out.stdout + out.stderr
    assert "domain2d check ok" in out.stdout and "FAIL" not in out.stdout
    assert 'not provoked: "grids too large"' in out.stdout
    got = {}
    for m in LINE.finditer(out.stdout):
        got[m.group(1)] = dict(hash=m.group(2), **{k: int(v) for k, v in zip(KEYS, m.groups()[2:])})
    with open(os.path.join(ROOT, "tests", "golden", "domain2d_build.json")) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name

    # the path each domain is there for: LAT ("identity" / "map" / None), MLAT, the coarse mesh staged in LDS (CLDS)
    def path(name):
        g = got[name]
        lat = None if g["lat_identity"] < 0 else ("identity" if g["lat_identity"] else "map")
        return lat, g["ml_bytes"] > 0, g["cl_bytes"] > 0

    assert path("lat_3x2") == path("lat_3x2_guess_half") == ("identity", False, False)
    assert path("lat_3x2_permuted") == ("map", False, False)
    for name in ("lat_3x2_interior_wall", "lat_split_cell", "lat_3x2_no_lat", "single_triangle", "single_nonconvex_quad"):
        assert path(name) == (None, False, False), name
    assert (got["lat_3x2"]["lat_nx"], got["lat_3x2"]["lat_ny"]) == (3, 2)
    assert got["single_triangle"]["single"] == 1 and got["single_nonconvex_quad"]["single"] == 0
    assert got["single_triangle"]["axis"] == 0 and got["lat_3x2_no_lat"]["axis"] == 1
    assert path("fan_4") == path("fan_16") == (None, False, True)
    assert got["fan_16"]["axis"] == 0
    for name in ("mlat_2x3_of_4x3", "mlat_2x3_coarse_permuted", "mlat_column_3_layers", "mlat_column_2_bins_mixed"):
        assert path(name) == (None, True, True), name
    g = got["mlat_2x3_of_4x3"]
    assert (g["ml_nx"], g["ml_ny"], g["ml_ncx"], g["ml_ncy"]) == (8, 9, 2, 3)
    g = got["mlat_column_3_layers"]
    assert (g["ml_nx"], g["ml_ny"], g["ml_ncx"], g["ml_ncy"]) == (5, 6, 1, 3)
    for name in ("mlat_2x3_no_mlat", "mlat_2x3_box_missing", "mlat_2x3_y_fastest"):
        assert path(name) == (None, False, True) and got[name]["axis"] == 1, name
    assert path("mlat_10x10_of_1x1") == (None, True, False)
    assert path("mlat_32x32_of_1x1") == (None, False, False)


def test_builder_sources_are_free_of_hip_and_the_environment():
    for name in ("rthx_domain2d.h", "rthx_domain2d_build.h", "rthx_domain2d_build.cpp"):
        txt = open(os.path.join(CSRC, name)).read()
        for word in ("hip_runtime", "rthx_kernels.h", "rthx_common.h", "knob(", "fail(", "getenv"):
            assert word not in txt, (name, word)
