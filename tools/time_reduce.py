#!/usr/bin/env python3
"""What the ensemble post-processing costs, on the device and on the host, at the C4 ensemble's size (bench.py --workload c4:
cases/gerd_roseires, a Manning-n ensemble; by default 32 768 members and all 385 levels):

  (a) host:   PreissmannBatch.hydrographs() - the whole [levels][4][B] block over the bus - and then the per-member np.interp
              loop of cases/gerd_roseires/n_calibrate.py: rmse_curve
  (b) device: PreissmannBatch.lookup with a target (levels at the gauge flows and RMSE; [n_q + 1][B] come back)
  (c) device: PreissmannBatch.summaries
  (d) device: PreissmannBatch.bands with three quantiles

The four are timed in alternating rounds on one batch after one untimed round (wall clock around calls that synchronise); the
report holds every sample, the medians and the spread.  One JSON line on stdout, also written to --out.

    python3 tools/time_reduce.py --out profiles/round7/reduce_timing.json"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "flow-sim_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reaches", type=int, default=32768)
    ap.add_argument("--levels", type=int, default=385)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import bench
    from cases.gerd_roseires.n_calibrate import H_target, Q_gauge
    from flowsim_amd import _abi as A

    B, L = args.reaches, args.levels
    batch, N, *_ = bench.build_batch("c4", "f64", B, None, L, 0, 0)
    t0 = time.perf_counter()
    batch.step(L - 1)
    step_s = time.perf_counter() - t0
    status = batch.status()
    z0 = 489.0          # bed level of the first section (cases/gerd_roseires: sections[0].z_min): depth -> stage

    def host_path():
        hyd = batch.hydrographs(0, L)
        t1 = time.perf_counter()
        out = np.empty(B)
        for i in range(B):
            levels = np.interp(x=Q_gauge, xp=hyd[:, 1, i], fp=hyd[:, 0, i] + z0)
            out[i] = np.mean((levels - H_target) ** 2) ** 0.5
        return out, t1

    legs = {
        "a_host_download_and_interp_loop": host_path,          # (returns its result and when the download ended)
        "b_device_lookup_rmse": lambda: batch.lookup(A.ROW_Q_IN, A.ROW_H_IN, Q_gauge, y_offset=z0, target=H_target, first=0, n=L)["rmse"],
        "c_device_summaries": lambda: batch.summaries(0, L)["q_net"],
        "d_device_bands_3_quantiles": lambda: batch.bands((0.05, 0.5, 0.95), 0, L)["quantiles"],
    }
    samples = {k: [] for k in legs}
    download_s = []
    results = {}
    for rnd in range(args.rounds + 1):                     # round 0 warms every path up (first-use allocations, page faults)
        for name, leg in legs.items():
            t0 = time.perf_counter()
            res, t1 = leg() if leg is host_path else (leg(), None)
            dt = time.perf_counter() - t0
            if rnd > 0:
                samples[name].append(dt)
                if t1 is not None:
                    download_s.append(t1 - t0)
            results[name] = res
    ok = status == 0
    mono = batch.lookup(A.ROW_Q_IN, A.ROW_H_IN, Q_gauge, first=0, n=L)["monotone"]
    both = ok & mono
    agree = float(np.max(np.abs(results["a_host_download_and_interp_loop"][both] - results["b_device_lookup_rmse"][both]))) if np.any(both) else None

    def stats(v):
        v = np.array(v)
        return dict(median_ms=float(np.median(v) * 1e3), min_ms=float(v.min() * 1e3), max_ms=float(v.max() * 1e3),
                    samples_ms=[round(float(x) * 1e3, 3) for x in v])
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    report = dict(tool="tools/time_reduce.py", date=time.strftime("%Y-%m-%d"), commit=commit, library_sha256=bench.library_sha256(),
                  reaches=B, nodes=int(N), levels=L, rounds=args.rounds, step_all_levels_s=step_s,
                  members_failed=int(np.sum(~ok)), members_with_descending_inflow=int(np.sum(~mono)),
                  max_abs_rmse_difference_host_vs_device=agree,
                  hydrograph_block_mb=L * 4 * B * 8 / 1e6, download_only=stats(download_s),
                  **{k: stats(v) for k, v in samples.items()})
    line = json.dumps(report)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
