"""wave_word_range (csrc/rthx_partition.h), the share of a row's histogram
words that each wave of a workgroup compacts: tests/partition_check.cpp built
for the host with AddressSanitizer and UBSan, and run."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wave_ranges_tile_the_histogram(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "partition_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "raytraceheattransfer.jl_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "partition_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "partition ok: %d cases" % (3 * (6001 + 64)) in out.stdout
