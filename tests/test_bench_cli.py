"""bench.py's command line beyond the headline: --dump-outputs (what the last timed step computed, for comparing two builds
output for output) and the plain run that leaves the --full measurements out."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

DUMPED = ("depth_last_step", "flow_last_step", "hydrograph_last_step", "newton_iterations_last_step")


def bench_module():
    sp = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(sp)
    sp.loader.exec_module(bench)
    return bench


class _Rows:
    """[B, N] with entry (r, i) = r N + i, built only for the rows asked for (the benchmark's state is gigabytes)"""
    def __init__(self, N, sign):
        self.N, self.sign = N, sign

    def __getitem__(self, rows):
        return self.sign * (np.asarray(rows)[:, None] * float(self.N) + np.arange(self.N))


class _StateOnly:
    """the part of PreissmannBatch that dump_outputs reads"""
    def __init__(self, B, N):
        self.B, self.N = B, N

    def state(self):
        return _Rows(self.N, 1.0), _Rows(self.N, -1.0)


@pytest.mark.parametrize("B,N,R", [(128, 300, 128), (65536, 4096, 65536), (8192, 16384, 8192), (600000, 64, 1200000)])
def test_dump_is_bounded_float_and_the_same_sample_every_time(B, N, R, tmp_path):
    bench = bench_module()
    row = torch.arange(4 * R, dtype=torch.float64).reshape(4, R)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), row, _StateOnly(B, N), np.arange(B, dtype=np.int32) % 7)
    total = 0
    for name in DUMPED:
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b)
        total += os.path.getsize(tmp_path / "a" / f"{name}.npy")
    assert total <= 64e6
    assert sorted(os.listdir(tmp_path / "a")) == sorted(f"{n}.npy" for n in DUMPED)
    h, hyd = np.load(tmp_path / "a" / "depth_last_step.npy"), np.load(tmp_path / "a" / "hydrograph_last_step.npy")
    assert h.shape[1] == N and hyd.shape[0] == 4
    assert h.shape[0] == (B if B * N <= 1 << 21 else (1 << 21) // N)
    assert hyd.shape[1] == min(R, 1 << 19)
    rows = (h[:, 0] // N).astype(np.int64)                            # which reaches the sample holds: in order, no repeats
    assert np.all(np.diff(rows) > 0) and rows[-1] < B


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step_the_same_twice(tmp_path):
    """Two plain runs of the same arguments write the same outputs bit for bit; the hydrograph row is the last row of the timed
    hydrographs and the boundary nodes of the dumped state; the line has ms_per_step and none of the --full measurements."""
    args = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--nodes", "300", "--reaches", "128", "--steps", "3",
            "--warmup", "1"]
    lines = []
    for d, extra in (("a", ["--dump-hydrographs", str(tmp_path / "hyd.npy")]), ("b", [])):
        r = subprocess.run(args + extra + ["--dump-outputs", str(tmp_path / d)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        out = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(out) == 1, r.stdout[-2000:]
        lines.append(json.loads(out[0]))
    for line in lines:
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["config"]["all_converged"]
        assert abs(line["value"] - 128 * 3 / (line["ms_per_step"] * 3e-3)) <= 1e-6 * line["value"]
        assert not any(k.startswith("cpu_baseline") for k in line) and "workloads" not in line
    for name in DUMPED:
        assert np.array_equal(np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")), name
    hyd = np.load(tmp_path / "a" / "hydrograph_last_step.npy")
    h, Q = np.load(tmp_path / "a" / "depth_last_step.npy"), np.load(tmp_path / "a" / "flow_last_step.npy")
    its = np.load(tmp_path / "a" / "newton_iterations_last_step.npy")
    assert hyd.shape == (4, 128) and h.shape == Q.shape == (128, 300) and its.shape == (128,) and np.all(its >= 1)
    assert np.array_equal(hyd, np.load(tmp_path / "hyd.npy")[-1])
    assert np.array_equal(hyd, np.stack([h[:, 0], Q[:, 0], h[:, -1], Q[:, -1]]))
