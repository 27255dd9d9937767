#!/usr/bin/env python3
"""What building a scenario ensemble's upstream forcing costs, on the host and on the device, at the C4 ensemble's size (by default
32 768 members and all 385 levels; cases/gerd_roseires: the tabulated inflow routed through the GERD reservoir):

  (a) host:   the mirror's GerdHydrograph.build (cases/gerd_roseires/gerd_discharge.py) per member - timed on --sample members and
              scaled to the batch - plus PreissmannBatch.set_boundary with the [levels][B] target (packed on the host, 100 MB
              over the bus), which is timed at full size
  (b) device: PreissmannBatch.set_boundary_sampled + route_pool (which returns its per-member flags, so it synchronises)

The members differ in inflow scale (0.25 .. 3) and initial pool level (625 .. 643 m).  The forcing does not depend on the reach, so
the batch is one of short rectangular reaches.  The two are timed in alternating rounds after one untimed round (wall clock around
calls that synchronise); the report holds every sample, the medians and the spread.  One JSON line on stdout, also written to --out.

    python3 tools/time_forcing.py --out profiles/round8/forcing_timing.json"""
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
    ap.add_argument("--sample", type=int, default=8, help="members the host routing is timed on in every round")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import bench
    from cases.gerd_roseires import settings as S
    from cases.gerd_roseires.gerd_discharge import GerdHydrograph
    from cases.gerd_roseires.inputs import import_hydrograph
    from flowsim_amd import _abi as A
    from flowsim_amd.batch import BoundarySpec, PreissmannBatch
    from flowsim_amd.hydromodel.hydrograph import Hydrograph

    B, L, dt = args.reaches, args.levels, S.time_step
    table = import_hydrograph(S.inflow_hyd_path)
    spec = GerdHydrograph.pool_spec()
    rng = np.random.default_rng(8)
    scale, level = rng.uniform(0.25, 3.0, B), rng.uniform(625.0, 643.0, B)
    flow = BoundarySpec(A.BC_FLOW_HYDROGRAPH)
    batch = PreissmannBatch(B, 30, L, section_mode="rect_uniform")
    batch.set_scheme(0.6, dt, 1000.0, 1e-6, 100)
    target = np.empty((L, B))
    sample = np.linspace(0, B - 1, args.sample).astype(int)

    def host_path():
        """-> (routing seconds on the sample, upload seconds at full size)"""
        t0 = time.perf_counter()
        for r in sample:
            inflow = Hydrograph(function=lambda t, r=r: scale[r] * float(np.interp(t, table[:, 0], table[:, 1])))
            rel = GerdHydrograph()
            try:
                rel.build(inflow_hydrograph=inflow, time_step=dt, duration=(L - 1) * dt, initial_stage=level[r])
                target[:, r] = rel.sample(L, dt)
            except ValueError:                   # no bracket: the reference stops here, and so does this member's cost
                target[:, r] = np.nan
        t1 = time.perf_counter()
        batch.set_boundary(A.UPSTREAM, BoundarySpec(A.BC_FLOW_HYDROGRAPH, {}, target))
        batch.sync()
        return t1 - t0, time.perf_counter() - t1

    def device_path():
        t0 = time.perf_counter()
        batch.set_boundary_sampled(A.UPSTREAM, flow, table[:, 0], table[:, 1], scale=scale)
        info = batch.route_pool(A.UPSTREAM, spec, level)
        return time.perf_counter() - t0, info

    route_s, upload_s, device_s = [], [], []
    info = None
    for rnd in range(args.rounds + 1):                     # round 0 warms both paths up (first-use allocations, page faults)
        a, u = host_path()
        d, info = device_path()
        if rnd > 0:
            route_s.append(a); upload_s.append(u); device_s.append(d)
    # the members the host routed, against the device's columns
    release = batch.bc_target(A.UPSTREAM)
    done = [r for r in sample if np.all(np.isfinite(target[:, r]))]
    agree = float(max(np.max(np.abs(release[:, r] - target[:, r]) / np.abs(target[:, r])) for r in done)) if done else None
    batch.close()

    def stats(v):
        v = np.array(v)
        return dict(median_ms=float(np.median(v) * 1e3), min_ms=float(v.min() * 1e3), max_ms=float(v.max() * 1e3),
                    samples_ms=[round(float(x) * 1e3, 3) for x in v])
    per_member = np.array(route_s) / len(sample)
    host_total = per_member * B + np.array(upload_s)
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    report = dict(tool="tools/time_forcing.py", date=time.strftime("%Y-%m-%d"), commit=commit, library_sha256=bench.library_sha256(),
                  reaches=B, levels=L, rounds=args.rounds, host_sample_members=len(sample), target_mb=L * B * 8 / 1e6,
                  members_without_bracket=int(np.sum(info["flags"] != 0)),
                  max_rel_release_difference_host_vs_device_on_the_sample=agree,
                  a_host_routing_per_member=stats(per_member), a_host_upload=stats(upload_s),
                  a_host_routing_scaled_to_batch_plus_upload=stats(host_total), b_device_sample_and_route=stats(device_s))
    line = json.dumps(report)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
