#!/usr/bin/env python3
"""What the flood envelopes along the reach cost, the parent's way and on the device, on the C4 ensemble (cases/gerd_roseires, a
Manning-n ensemble that keeps its history; by default 8 192 members x 385 levels, and one smaller size):

  (a) host:   PreissmannBatch.derive of stage and velocity - two [levels][B][N] arrays over the bus - then numpy max / argmax over
              the levels, the threshold counts of the stage, and np.quantile of the peak stage across the members
  (b) device: PreissmannBatch.envelope (stage and velocity, a stage threshold) + PreissmannBatch.profile_bands of the peak stage;
              the envelope kernel with four levels' loads in flight per thread and (b1) with one
  (c) kernel times only, results left on the device: all six quantities; the stage alone with 1, 4 and 8 levels' loads in flight

The legs are timed in alternating rounds on one batch after one untimed round (wall clock around calls that synchronise; kernel times
are HIP events, PreissmannBatch.last_step_ms); the report holds every sample, the medians and the spread, the bytes each way moves
over PCIe and the envelope kernel's HBM rate: 16 B per element and level read (2 B N levels values; the stage alone reads the depth
history only, 8 B), against derive_fields_kernel's recorded rate (profiles/round4/derive.json).  One JSON line per size on stdout, the list of them written to --out.

    python3 tools/time_envelope.py --out profiles/round11/envelope_timing.json"""
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

QUANTILES = (0.05, 0.5, 0.95)


def history_batch(B, levels):
    """bench.py's C4 members in a batch that keeps its history"""
    import numpy as np
    from cases.gerd_roseires.model import build as build_gerd
    from flowsim_amd import PreissmannBatch
    from flowsim_amd import _abi as A
    from flowsim_amd.ensemble import gvf_profiles
    from flowsim_amd.hydromodel.preissmann import boundary_to_spec
    solver, _ = build_gerd(inflow_hyd_func=None, sim_duration=(levels - 1) * 3600)
    ch, N = solver.channel, solver.number_of_nodes
    n_members = 0.020 + 0.040 * np.random.default_rng(20260215).random(B)
    batch = PreissmannBatch(B, N, levels, dtype="f64", section_mode="table", history=True)
    batch.set_scheme(solver.theta, float(solver.time_step), solver.spatial_step, 1e-6, 100)
    batch.set_geometry_table(ch.node_geometry, n_main_override=n_members)
    batch.set_boundary(A.UPSTREAM, boundary_to_spec(ch.upstream_boundary, levels, float(solver.time_step)))
    batch.set_boundary(A.DOWNSTREAM, boundary_to_spec(ch.downstream_boundary, levels, float(solver.time_step)))
    ic = gvf_profiles(ch, n_members)
    batch.set_state(ic[:, :, 0], ic[:, :, 1])
    return batch, N


def measure(B, L, rounds):
    import numpy as np
    import bench
    from flowsim_amd import _abi as A
    batch, N = history_batch(B, L)
    t0 = time.perf_counter()
    batch.step(L - 1)
    step_s = time.perf_counter() - t0
    ok = batch.status() == 0
    # the threshold: per node, the median over the members of the peak stage (half of them reach it)
    first = batch.envelope(("stage",))
    thr = np.median(first["stage"]["max"][ok], axis=0)
    kernel_ms = {}

    def host_path():
        d = batch.derive(0, L, fields=("level", "velocity"))
        kernel_ms.setdefault("a_derive_kernel", []).append(batch.last_step_ms())
        t1 = time.perf_counter()
        peak, when = d["level"].max(axis=0), d["level"].argmax(axis=0)
        vmax, vwhen = d["velocity"].max(axis=0), d["velocity"].argmax(axis=0)
        count = (d["level"] >= thr[None, None, :]).sum(axis=0)
        q = np.quantile(peak[ok], QUANTILES, axis=0)
        return dict(peak=peak, when=when, vmax=vmax, vwhen=vwhen, count=count, q=q.T), t1

    def device_path(unroll):
        def leg():
            os.environ["FS_ENVELOPE_UNROLL"] = str(unroll)
            env = batch.envelope(("stage", "velocity"), threshold=thr)
            kernel_ms.setdefault(f"b_envelope_kernel_unroll{unroll}", []).append(batch.last_step_ms())
            pb = batch.profile_bands("stage", "max", QUANTILES)
            kernel_ms.setdefault("b_transpose_and_profile_bands_kernels", []).append(batch.last_step_ms())
            return dict(peak=env["stage"]["max"], when=env["stage"]["max_level"], vmax=env["velocity"]["max"], vwhen=env["velocity"]["max_level"],
                        count=env["crossing"]["count"], q=pb["quantiles"]), None
        return leg

    def kernel_records():
        """kernel times only, results left on the device: all six quantities; the stage alone with 1, 4, 8 levels in flight"""
        os.environ["FS_ENVELOPE_UNROLL"] = "4"
        batch.envelope_device(A.ENV_QUANTITIES, threshold=thr)
        kernel_ms.setdefault("c_envelope_kernel_all_six_quantities", []).append(batch.last_step_ms())
        for u in (1, 4, 8):
            os.environ["FS_ENVELOPE_UNROLL"] = str(u)
            batch.envelope_device(("stage",), threshold=thr)
            kernel_ms.setdefault(f"c_envelope_kernel_stage_alone_unroll{u}", []).append(batch.last_step_ms())
        return None, None

    legs = {"a_host_derive_download_numpy": host_path, "b_device_envelope_profile_bands": device_path(4),
            "b1_device_envelope_one_level_in_flight": device_path(1), "c_kernel_records": kernel_records}
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
    os.environ.pop("FS_ENVELOPE_UNROLL", None)
    a, b = results["a_host_derive_download_numpy"], results["b_device_envelope_profile_bands"]
    same = {k: bool(np.array_equal(a[k][ok], b[k][ok])) for k in ("peak", "when", "vmax", "vwhen", "count")}
    same["quantiles_max_abs_difference"] = float(np.max(np.abs(a["q"] - b["q"])))

    def stats(v, scale=1e3):
        v = np.array(v) * scale
        return dict(median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()), samples_ms=[round(float(x), 3) for x in v])
    BN = B * N
    read_bytes = 2 * L * BN * 8                            # (the stage alone reads the depth history only)
    rate = {k: read_bytes / (2 if "stage_alone" in k else 1) / (float(np.median(v)) * 1e-3) / 1e12
            for k, v in kernel_ms.items() if "_envelope_kernel" in k}
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    report = dict(tool="tools/time_envelope.py", date=time.strftime("%Y-%m-%d"), commit=commit, library_sha256=bench.library_sha256(),
                  reaches=B, nodes=int(N), levels=L, rounds=rounds, step_all_levels_s=step_s, members_failed=int(np.sum(~ok)),
                  device_equals_host=same,
                  pcie_bytes=dict(a_host=2 * L * BN * 8, b_device=(2 * 4 + 3) * BN * 8 + B * 4 + N * (4 + len(QUANTILES) + 1) * 8 + N * 4 + N * 8),
                  history_bytes_read_by_envelope_kernel=read_bytes, envelope_kernel_tb_per_s=rate,
                  derive_fields_kernel_tb_per_s_recorded=5.92, download_only=stats(download_s),
                  wall={k: stats(v) for k, v in samples.items() if not k.startswith("c_")}, kernels={k: stats(v, 1.0) for k, v in kernel_ms.items()})
    batch.close()
    return report


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reaches", type=int, nargs="+", default=[1024, 8192])
    ap.add_argument("--levels", type=int, default=385)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    reports = []
    for B in args.reaches:
        reports.append(measure(B, args.levels, args.rounds))
        print(json.dumps(reports[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(reports) + "\n")


if __name__ == "__main__":
    main()
