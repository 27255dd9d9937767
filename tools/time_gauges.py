#!/usr/bin/env python3
"""What station series inside the reach cost, the parent's way and on the device, on the C4 ensemble (cases/gerd_roseires, a Manning-n
ensemble that keeps its history; the sizes of tools/time_envelope.py: 1 024 and 8 192 members x 385 levels), for four gauges spread
along the reach:

  (a) host:   PreissmannBatch.derive of stage and velocity - two [levels][B][N] arrays over the bus - then the numpy pick of the two
              nodes around each gauge, the interpolation, and np.quantile of each gauge's two series across the members
  (b) device: PreissmannBatch.gauges over the whole range (the gather kernel's own time from last_step_ms), gauge_bands with three
              quantiles and gauge_score of the stage against a record, per gauge; only bands and scores cross the bus
  (c) PreissmannBatch.reach_integrals over the same range, kernel time only: the yardstick for ONE streamed pass over the depth history

The legs are timed in alternating rounds on one batch after one untimed round (wall clock around calls that synchronise; kernel times
are HIP events); the report holds every sample, the median and min .. max, and the cache lines the gather touches against those a
streamed pass reads.  Every size runs in a child process of its own under a time limit; a child that fails ends the run.  One JSON
line per size on stdout, the list of them written to --out.

    python3 tools/time_gauges.py --out profiles/round15/gauges_timing.json"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "flow-sim_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

QUANTILES = (0.05, 0.5, 0.95)
N_GAUGES = 4


def measure(B, L, rounds):
    import numpy as np
    import bench
    from flowsim_amd import _abi as A
    from time_envelope import history_batch
    batch, N = history_batch(B, L)
    t0 = time.perf_counter()
    batch.step(L - 1)
    step_s = time.perf_counter() - t0
    ok = batch.status() == 0
    # four gauges spread along the reach, between two nodes each
    node = np.array([(g + 1) * (N - 1) // (N_GAUGES + 1) for g in range(N_GAUGES)], dtype=np.int32)
    weight = np.array([0.25, 0.5, 0.75, 0.125])
    batch.set_gauges(node=node, weight=weight)
    batch.gauges(0, L)
    record = np.stack([np.nanmedian(batch.gauge_rows(g, 0, L)[:, A.GAUGE_ROWS.index("stage")][:, ok], axis=1) for g in range(N_GAUGES)])
    record[:, ::7] = np.nan                                # (a record with gaps)
    kernel_ms = {}

    def host_path():
        d = batch.derive(0, L, fields=("level", "velocity"))
        kernel_ms.setdefault("a_derive_kernel", []).append(batch.last_step_ms())
        t1 = time.perf_counter()
        rows, q = [], []
        for g in range(N_GAUGES):
            i, w = int(node[g]), float(weight[g])
            series = np.stack([a[:, :, i] + w * (a[:, :, i + 1] - a[:, :, i]) for a in (d["level"], d["velocity"])], axis=1)      # [L, 2, B]
            rows.append(series)
            q.append(np.quantile(series[:, :, ok], QUANTILES, axis=2))
        return dict(rows=np.stack(rows), q=np.stack(q)), t1

    def device_path():
        batch.gauges(0, L)
        kernel_ms.setdefault("b_gauge_gather_kernel", []).append(batch.last_step_ms())
        bands, scores = [], []
        for g in range(N_GAUGES):
            bands.append(batch.gauge_bands(g, QUANTILES, 0, L))
            kernel_ms.setdefault("b_members_and_bands_kernels_per_gauge", []).append(batch.last_step_ms())
            scores.append(batch.gauge_score(g, "stage", record[g], 0, L))
            kernel_ms.setdefault("b_score_kernel_per_gauge", []).append(batch.last_step_ms())
        return dict(q=np.stack([np.moveaxis(bd["quantiles"], 2, 0) for bd in bands]), rmse=np.stack([s["rmse"] for s in scores])), None

    def streamed_pass():
        batch._lib.fs_batch_reach_integrals(batch._h, 0, L, None, 0)
        batch.sync()
        kernel_ms.setdefault("c_reach_integrals_kernel", []).append(batch.last_step_ms())
        return None, None

    legs = {"a_host_derive_download_numpy": host_path, "b_device_gauges_bands_scores": device_path, "c_streamed_pass": streamed_pass}
    samples = {k: [] for k in legs}
    download_s, results = [], {}
    for rnd in range(rounds + 1):                          # round 0 warms every path up (first-use allocations, page faults)
        for name, leg in legs.items():
            t0 = time.perf_counter()
            res, t1 = leg()
            dt = time.perf_counter() - t0
            if rnd > 0:
                samples[name].append(dt)
                if t1 is not None:
                    download_s.append(t1 - t0)
            results[name] = res
        if rnd == 0:
            kernel_ms.clear()
    a, b = results["a_host_derive_download_numpy"], results["b_device_gauges_bands_scores"]
    dev_rows = np.stack([batch.gauge_rows(g, 0, L) for g in range(N_GAUGES)])
    same = dict(stage_and_velocity_rows=bool(np.array_equal(a["rows"][:, :, :, ok], dev_rows[:, :, 2:, ok], equal_nan=True)),
                quantiles_max_abs_difference=float(np.nanmax(np.abs(a["q"] - b["q"][:, :, :, 2:]))))

    def stats(v, scale=1e3):
        v = np.array(v) * scale
        return dict(median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()), samples_ms=[round(float(x), 3) for x in v])
    lines_streamed = L * B * N * 8 // 128                  # one pass over the depth history
    lines_gathered_at_most = L * B * N_GAUGES * 2 * 2      # per gauge: depth and flow, a line each for node and node + 1 at most
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    report = dict(tool="tools/time_gauges.py", date=time.strftime("%Y-%m-%d"), commit=commit, library_sha256=bench.library_sha256(),
                  reaches=B, nodes=int(N), levels=L, rounds=rounds, gauges=dict(node=node.tolist(), weight=weight.tolist()),
                  step_all_levels_s=step_s, members_failed=int(np.sum(~ok)), device_equals_host=same,
                  pcie_bytes=dict(a_host=2 * L * B * N * 8, b_device=N_GAUGES * (L * 4 * (4 + len(QUANTILES)) * 8 + L * 4 + L * 8 + len(A.GS_ROWS) * B * 8)),
                  cache_lines=dict(streamed_depth_history=lines_streamed, gathered_at_most=lines_gathered_at_most,
                                   gauge_block_written=L * B * N_GAUGES * 4 * 8 // 128),
                  download_only=stats(download_s), wall={k: stats(v) for k, v in samples.items() if not k.startswith("c_")},
                  kernels={k: stats(v, 1.0) for k, v in kernel_ms.items()})
    batch.close()
    return report


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reaches", type=int, nargs="+", default=[1024, 8192])
    ap.add_argument("--levels", type=int, default=385)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--limit", type=int, default=420, help="seconds a size may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args.reaches[0], args.levels, args.rounds)), flush=True)
        return 0
    reports = []
    for B in args.reaches:                                 # a fresh process per size, under its own time limit; the first failure ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reaches", str(B), "--levels", str(args.levels), "--rounds", str(args.rounds)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(f"time_gauges: {B} members did not finish within {args.limit} s", file=sys.stderr)
            return 124
        if r.returncode != 0:
            print(r.stderr[-3000:], file=sys.stderr)
            return r.returncode if r.returncode > 0 else 1
        reports.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(reports[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(reports) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
