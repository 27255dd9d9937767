#!/usr/bin/env python3
"""Wall time of initial conditions on the device against the host paths they replace.

    python3 tools/time_init_state.py [--members 32768] [--reaches 4096] [--runs 5] [--host-sample 16]

1. The C4 shape: cases/gerd_roseires (121 nodes, compound sections, curvature) shared by `members` Manning-n members, TABLE mode with
   the per-reach override.  Alternating, `runs` times each: today's path - flowsim_amd.ensemble.gvf_profiles (numpy, vectorised over
   the members) + set_state (2 B N doubles over the bus) - and init_state('GVF_equation') followed by a sync.
2. A batch of `reaches` reaches with a table of their own each (the gerd channel with widths drawn per reach): nothing vectorises
   this on the host, today's path is one Channel set-up per reach as cases/gerd_roseires/n_calibrate.py does it.  That loop is timed on
   `host-sample` reaches and scaled to the batch (it is a plain loop); the device path is timed whole, `runs` times.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "flow-sim_amd")):
    sys.path.insert(0, p)


def spread(ts):
    return dict(median_s=statistics.median(ts), min_s=min(ts), max_s=max(ts), runs=len(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=32768)
    ap.add_argument("--reaches", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--host-sample", type=int, default=16)
    a = ap.parse_args()
    from cases.gerd_roseires.model import build as build_gerd
    from cases.gerd_roseires.n_calibrate import member_setup
    from flowsim_amd import PreissmannBatch
    from flowsim_amd import _abi as A
    from flowsim_amd.ensemble import gvf_profiles
    solver, _ = build_gerd(inflow_hyd_func=None, sim_duration=16 * 3600)
    ch, N = solver.channel, solver.number_of_nodes
    Q, h_ds = ch.initial_flow_rate, ch.downstream_boundary.initial_depth
    rng = np.random.default_rng(20260215)
    out = dict(nodes=N)

    B = a.members
    n_members = 0.020 + 0.040 * rng.random(B)
    host, dev = [], []
    with PreissmannBatch(B, N, 4, section_mode="table", monitor=False) as b:
        b.set_scheme(solver.theta, float(solver.time_step), solver.spatial_step, 1e-6, 100)
        b.set_geometry_table(ch.node_geometry, n_main_override=n_members)
        b.init_state("GVF_equation", Q, depth_ds=h_ds)          # (first launch: code object load)
        for _ in range(a.runs):
            t0 = time.perf_counter()
            ic = gvf_profiles(ch, n_members)
            b.set_state(ic[:, :, 0], ic[:, :, 1])
            b.sync()
            host.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            b.init_state("GVF_equation", Q, depth_ds=h_ds)
            b.sync()
            dev.append(time.perf_counter() - t0)
        h, _ = b.state()
        out["c4"] = dict(members=B, host_gvf_profiles_set_state=spread(host), device_init_state=spread(dev),
                         max_abs_difference_m=float(np.max(np.abs(h - ic[:, :, 0]))))

    B = a.reaches
    widths = 0.9 + 0.2 * rng.random(B)
    n_members = 0.020 + 0.040 * rng.random(B)
    geo = {k: np.broadcast_to(np.asarray(ch.node_geometry[k], dtype=np.float64), (B, N)).copy() for k in A.GEO_ROWS}
    geo["b_main"] *= widths[:, None]
    t0 = time.perf_counter()
    for k in range(a.host_sample):
        member_setup(float(n_members[k]))
    per_reach = (time.perf_counter() - t0) / a.host_sample
    dev = []
    with PreissmannBatch(B, N, 4, section_mode="table", monitor=False) as b:
        b.set_scheme(solver.theta, float(solver.time_step), solver.spatial_step, 1e-6, 100)
        b.set_geometry_table(geo, n_main_override=n_members)
        b.init_state("GVF_equation", Q, depth_ds=h_ds)
        for _ in range(a.runs):
            t0 = time.perf_counter()
            b.init_state("GVF_equation", Q, depth_ds=h_ds)
            b.sync()
            dev.append(time.perf_counter() - t0)
    out["per_reach_tables"] = dict(reaches=B, host_loop_s_per_reach=per_reach, host_loop_sample=a.host_sample,
                                   host_loop_scaled_s=per_reach * B, device_init_state=spread(dev))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
