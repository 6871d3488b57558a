"""bench.py's own contract: a plain run reports the headline only, --full adds
every other leg, --dump-outputs writes the last timed step's count matrix.
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H

DUMP_FILES = ("col_totals", "row_ptr", "row_totals", "sample_counts", "sample_rows")
FULL_ONLY = ("roofline", "roofline_fp64", "roofline_valu", "pack_ms", "blocking_ms_per_step", "faithful_sampling",
             "philox10", "e2e_with_d2h_mrays_s", "e2e_F_with_d2h_mrays_s", "cpu_baseline")
SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--prewarm-s", "0", "--rays-per-gpu", "2000000"]


def _bench_line(argv):
    out = subprocess.run([sys.executable, os.path.join(H.ROOT, "bench.py")] + argv, capture_output=True, text=True,
                         timeout=240, cwd=H.ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    assert sorted(os.listdir(d)) == [n + ".npy" for n in DUMP_FILES]
    a = {n: np.load(os.path.join(d, n + ".npy")) for n in DUMP_FILES}
    assert all(x.dtype == np.float64 for x in a.values())
    assert sum(x.nbytes for x in a.values()) <= 64e6
    return a


def test_dump_outputs_writes_the_csr_of_a_shard(tmp_path):
    """dump_outputs on the oracle's CSR of a strided shard (rows 1, 3, 5, ...
    of an 11x11 square): whole row pointers, row and column totals of every
    row, and the sampled rows -- all of this shard, fewer than DUMP_ROWS --
    dense, entry for entry."""
    import bench
    from oracle import oracle
    from rthx import _lib

    flat = H.square_domain(11).flat()
    n = flat.n_emitters
    args, _k = _lib.make_args(0, 500, H.NUDGE, 1, 1, n, 2)
    rp, cols, cnt, info, _ = oracle.trace_exchange(flat, args, 0)

    class Res:
        def csr(self):
            return rp, cols, cnt

    bench.dump_outputs(str(tmp_path / "a"), Res(), 1, 2)
    bench.dump_outputs(str(tmp_path / "b"), Res(), 1, 2)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert all(np.array_equal(a[k], b[k]) for k in DUMP_FILES)
    C = H.counts_matrix(rp, cols, cnt, n).toarray()
    assert np.array_equal(a["row_ptr"], rp)
    assert np.array_equal(a["row_totals"], C.sum(axis=1)) and a["row_totals"].sum() == info["rays_traced"] - info["lost_total"]
    assert np.array_equal(a["col_totals"], C.sum(axis=0))
    assert np.array_equal(a["sample_rows"], np.arange(1, n, 2))
    assert np.array_equal(a["sample_counts"], C[1::2])


@pytest.fixture(scope="module")
def runs(hip, tmp_path_factory):
    """One plain and one --full run (a 1 s CPU sample) with the same
    arguments, each dumping its outputs: (plain line, full line, plain
    arrays, full arrays)."""
    d = tmp_path_factory.mktemp("bench")
    plain = _bench_line(SMALL + ["--dump-outputs", str(d / "plain")])
    full = _bench_line(SMALL + ["--dump-outputs", str(d / "full"), "--full", "--faithful-steps", "2",
                                "--philox10-steps", "2", "--cpu-budget", "1"])
    return plain, full, _load(d / "plain"), _load(d / "full")


@pytest.mark.gpu
def test_plain_bench_reports_the_headline_only(runs):
    """A plain run times exactly --steps steps, every one checked, and reports
    none of the --full legs; value and ms_per_step agree (ms_per_step is
    rounded to 1e-4 ms: 0.5 % of a step of this size)."""
    for line in runs[:2]:
        assert line["steps"] == 3 and line["steps_checked"] == 3 and line["pipelined_step_faults"] == 0
        assert line["value"] > 0 and line["unit"] == "Mrays/s" and line["higher_is_better"] is True
        assert line["dtype"] == "f64" and line["ms_per_step"] > 0
        assert line["value"] == pytest.approx(line["config"]["rays_per_step"] / line["ms_per_step"] / 1e3, rel=0.01)
    assert not set(FULL_ONLY) & set(runs[0])


@pytest.mark.gpu
def test_full_bench_reports_every_leg(runs):
    """--full: the plain line plus the rooflines, the blocking steps, the
    faithful and Philox-10 legs, the PCIe-inclusive passes and the CPU
    baseline."""
    line = runs[1]
    assert set(FULL_ONLY) <= set(line)
    assert line["roofline"]["avg_kernel_ms"] > 0 and line["blocking_ms_per_step"] > 0
    assert line["faithful_sampling"]["value"] > 0 and line["philox10"]["value"] > 0
    assert line["e2e_with_d2h_mrays_s"] > 0 and line["e2e_F_with_d2h_mrays_s"] > 0
    assert line["cpu_baseline"]["value"] > 0


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_step(runs):
    """Two runs with the same arguments dump identical arrays (the --full
    legs that follow do not touch them), which hold the counts of the step
    that was timed: every row's length and total, 256 distinct sampled rows
    dense, and all but at most 1e-6 of the step's rays tallied (a ray ending
    within an ulp of a corner can be lost, as in the reference)."""
    plain, _full, a, b = runs
    assert all(np.array_equal(a[k], b[k]) for k in DUMP_FILES)
    c = plain["config"]
    n = c["n_emitters"]
    assert a["row_ptr"].shape == (n + 1,) and a["row_ptr"][-1] == c["nnz_per_step"]
    assert a["sample_counts"].shape == (256, n)
    rows = a["sample_rows"].astype(np.int64)
    assert len(np.unique(rows)) == 256 and rows.min() >= 0 and rows.max() < n
    assert np.array_equal(a["sample_counts"].sum(axis=1), a["row_totals"][rows])
    assert np.array_equal(np.count_nonzero(a["sample_counts"], axis=1), np.diff(a["row_ptr"])[rows])
    assert a["row_totals"].sum() == a["col_totals"].sum()
    assert 0 <= c["rays_per_step"] - a["row_totals"].sum() <= 1e-6 * c["rays_per_step"]
