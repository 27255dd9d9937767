#!/usr/bin/env python3
"""What reach storage and the discrete water balance cost, the parent's way and on the device, on the C4 ensemble (cases/gerd_roseires,
a Manning-n ensemble that keeps its history; by default 8 192 members x 385 levels, and one smaller size):

  (a) host:   PreissmannBatch.derive of area and top width - two [levels][B][N] arrays over the bus - then the numpy trapezoid sums,
              the balance from them and the hydrograph block, and np.quantile of the volume across the members
  (b) device: PreissmannBatch.reach_integrals + water_balance + integral_bands (no threshold)
  (c) kernel times only, by HIP events (PreissmannBatch.last_step_ms): the integral kernel over the whole history, the balance walk,
      the bands

The legs are timed in alternating rounds on one batch after one untimed round (wall clock around calls that synchronise); the report
holds every sample, the medians and the spread, the bytes each way moves over PCIe and the integral kernel's HBM rate - it reads the
depth history once, 8 B per node and level - next to the rates recorded for kernels that read the same bytes: derive_fields_kernel
(profiles/round4/derive.json) and the envelope's stage-only walk (profiles/round11/envelope_timing.json).

--flagship adds one line for a batch WITHOUT history, bench.py's C3 shape (65 536 x 4 096 fp64): the current-state evaluation (a
"mark") against one level of stepping, kernel times from the same run.

One JSON line per size on stdout, the list of them written to --out.

    python3 tools/time_balance.py --flagship --out profiles/round12/balance_timing.json"""
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


def stats(v, scale=1e3):
    import numpy as np
    v = np.array(v) * scale
    return dict(median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()), samples_ms=[round(float(x), 4) for x in v])


def recorded_rates():
    """TB/s of the kernels that read the same bytes, from the project's records (None: the record does not hold the figure)"""
    out = dict(derive_fields_kernel=5.92)                  # profiles/round4/derive.json, as tools/time_envelope.py quotes it
    try:
        reports = json.load(open(os.path.join(ROOT, "profiles", "round11", "envelope_timing.json")))
        out["envelope_stage_alone"] = {str(r["reaches"]): r["envelope_kernel_tb_per_s"].get("c_envelope_kernel_stage_alone_unroll4") for r in reports}
    except (OSError, KeyError, ValueError):
        out["envelope_stage_alone"] = None
    return out


def measure(B, L, rounds):
    import numpy as np
    import bench
    from time_envelope import history_batch
    batch, N = history_batch(B, L)
    from cases.gerd_roseires.model import build as build_gerd
    solver, _ = build_gerd(inflow_hyd_func=None, sim_duration=(L - 1) * 3600)       # history_batch's solver: the scheme it hands the batch
    theta, dt, dx = float(solver.theta), float(solver.time_step), float(solver.spatial_step)
    t0 = time.perf_counter()
    batch.step(L - 1)
    step_s = time.perf_counter() - t0
    ok = batch.status() == 0
    w = np.ones(N)
    w[0] = w[-1] = 0.5
    kernel_ms = {}

    def host_path():
        d = batch.derive(0, L, fields=("area", "top_width"))
        kernel_ms.setdefault("a_derive_kernel", []).append(batch.last_step_ms())
        hyd = batch.hydrographs(0, L)
        t1 = time.perf_counter()
        V, S = dx * (d["area"] @ w), dx * (d["top_width"] @ w)
        net = hyd[:, 1] - hyd[:, 3]
        res = np.zeros_like(V)
        res[1:] = (V[1:] - V[:-1]) - dt * (theta * net[1:] + (1.0 - theta) * net[:-1])
        q = np.quantile(V[:, ok], QUANTILES, axis=1).T
        return dict(volume=V, surface=S, balance=res, q=q), t1

    def device_path():
        rows = batch.reach_integrals(0, L)
        kernel_ms.setdefault("b_reach_integrals_kernel", []).append(batch.last_step_ms())
        rows, totals = batch.water_balance(0, L)
        kernel_ms.setdefault("b_balance_kernel", []).append(batch.last_step_ms())
        bands = batch.integral_bands(QUANTILES, 0, L)
        kernel_ms.setdefault("b_bands_kernel", []).append(batch.last_step_ms())
        return dict(volume=rows["volume"], surface=rows["surface"], balance=rows["balance"], q=bands["quantiles"][:, 0], totals=totals), None

    def kernel_records():
        """the integral kernel alone, nothing downloaded: one row (the current state) and the whole history"""
        batch.reach_integrals(current=True)
        batch.sync()
        kernel_ms.setdefault("c_reach_integrals_kernel_current_state", []).append(batch.last_step_ms())
        batch._lib.fs_batch_reach_integrals(batch._h, 0, L, None, 0)
        batch.sync()
        kernel_ms.setdefault("c_reach_integrals_kernel_whole_history", []).append(batch.last_step_ms())
        return None, None

    legs = {"a_host_derive_download_numpy": host_path, "b_device_integrals_balance_bands": device_path, "c_kernel_records": kernel_records}
    samples = {k: [] for k in legs}
    download_s, results = [], {}
    for rnd in range(rounds + 1):                          # round 0 warms every path up (first-use allocations, page faults)
        for name, leg in legs.items():
            t0 = time.perf_counter()
            res, t1 = leg()
            took = time.perf_counter() - t0
            if rnd > 0:
                samples[name].append(took)
                if t1 is not None:
                    download_s.append(t1 - t0)
            results[name] = res
        if rnd == 0:
            kernel_ms.clear()
    a, b = results["a_host_derive_download_numpy"], results["b_device_integrals_balance_bands"]
    scale = np.maximum(np.abs(a["volume"][:, ok]), 1.0)
    agree = dict(volume_max_rel=float(np.max(np.abs(a["volume"][:, ok] - b["volume"][:, ok]) / scale)),
                 surface_max_rel=float(np.max(np.abs(a["surface"][:, ok] - b["surface"][:, ok]) / np.maximum(np.abs(a["surface"][:, ok]), 1.0))),
                 balance_max_abs_difference_m3=float(np.max(np.abs(a["balance"][:, ok] - b["balance"][:, ok]))),
                 quantiles_max_rel=float(np.max(np.abs(a["q"] - b["q"]) / np.maximum(np.abs(a["q"]), 1.0))))
    worst = b["totals"]["worst"][ok]
    bound = dt * dx * np.sqrt(N - 1) * 1e-6
    BN = B * N
    read_bytes = L * BN * 8
    rate = {k: (read_bytes if "whole" in k or k.startswith("b_") else BN * 8) / (float(np.median(v)) * 1e-3) / 1e12
            for k, v in kernel_ms.items() if "reach_integrals_kernel" in k}
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    report = dict(tool="tools/time_balance.py", date=time.strftime("%Y-%m-%d"), commit=commit, library_sha256=bench.library_sha256(),
                  reaches=B, nodes=int(N), levels=L, rounds=rounds, step_all_levels_s=step_s, members_failed=int(np.sum(~ok)),
                  device_against_host=agree,
                  closure=dict(worst_residual_m3=float(np.max(worst)), bound_dt_dx_sqrt_cells_tolerance_m3=float(bound), worst_ratio=float(np.max(worst) / bound)),
                  pcie_bytes=dict(a_host=(2 * L * BN + 4 * L * B) * 8, b_device=(4 * L * B + 10 * B + 4 * L * (4 + len(QUANTILES))) * 8 + L * 4),
                  history_bytes_read_by_integral_kernel=read_bytes, integral_kernel_tb_per_s=rate, recorded_tb_per_s=recorded_rates(),
                  download_only=stats(download_s), wall={k: stats(v) for k, v in samples.items() if not k.startswith("c_")},
                  kernels={k: stats(v, 1.0) for k, v in kernel_ms.items()})
    batch.close()
    return report


def flagship(B, N, rounds):
    """a batch without history: one level of stepping against one mark of the current state, kernel times by HIP events"""
    import numpy as np
    import bench
    levels = 2 * (rounds + 1) + 4
    batch, N, *_ = bench.build_batch("c3", "f64", B, N, levels, 0, 0)
    step_ms, mark_ms = [], []
    for rnd in range(rounds + 1):
        batch.step(1)
        if rnd > 0:
            step_ms.append(batch.last_step_ms())
        batch.reach_integrals(current=True)
        batch.sync()
        if rnd > 0:
            mark_ms.append(batch.last_step_ms())
    rows, totals = batch.water_balance(0, batch.level + 1)
    ok = batch.status() == 0
    report = dict(tool="tools/time_balance.py", workload="flagship C3 without history", reaches=B, nodes=int(N), rounds=rounds,
                  members_failed=int(np.sum(~ok)), step_one_level_kernel=stats(step_ms, 1.0), mark_current_state_kernel=stats(mark_ms, 1.0),
                  mark_over_step=float(np.median(mark_ms) / np.median(step_ms)),
                  mark_tb_per_s=B * N * 8 / (float(np.median(mark_ms)) * 1e-3) / 1e12,
                  worst_closure_m3=float(np.nanmax(totals["worst"][ok])), bound_m3=float(600.0 * 250.0 * np.sqrt(N - 1) * 1e-6))
    batch.close()
    return report


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reaches", type=int, nargs="+", default=[1024, 8192])
    ap.add_argument("--levels", type=int, default=385)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--flagship", action="store_true", help="add the line of a 65 536 x 4 096 batch without history")
    ap.add_argument("--flagship-reaches", type=int, default=65536)
    ap.add_argument("--flagship-nodes", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    reports = []
    for B in args.reaches:
        reports.append(measure(B, args.levels, args.rounds))
        print(json.dumps(reports[-1]), flush=True)
    if args.flagship:
        reports.append(flagship(args.flagship_reaches, args.flagship_nodes, args.rounds))
        print(json.dumps(reports[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(reports) + "\n")


if __name__ == "__main__":
    main()
