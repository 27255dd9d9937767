#!/usr/bin/env python3
"""What setting up a geometry ensemble of one polyline channel costs, on the host and on the device, at the size of the benchmark's
polyline ensemble (bench.py --workload irr: 8 192 members x 128 nodes, 8 - 15 stations per section) and at 40 stations per section
with fewer members (the stage tables stay under FS_POLY_TABLE_MAX_BYTES):

  (a) host:   flowsim_amd._pack.member_sections (numpy) + PreissmannBatch.set_geometry_irregular per reach: the library builds every
              member's stage tables on the host (fs::plan_irregular), stages them and uploads them
  (b) device: PreissmannBatch.set_geometry_irregular_members (it returns when the members are built)

Every member has its own bed shifts (|dz| <= 0.3 m per strip and node) and roughness factors.  The two are timed in alternating
rounds after one untimed round, wall clock around calls that synchronise; the report holds every sample, the medians and the
spread, the bytes each path sends over the bus, the peak resident memory of the process after (b) alone and after (a) (first size only), the HIP-event
time of the two kernels of (b) and the store bandwidth that comes to, and a sample of nodes whose tables the two paths must agree
on bit for bit.  One JSON line per size on stdout, the list of them written to --out.

    python3 tools/time_geometry.py --out profiles/round10/geometry_timing.json"""
import argparse
import json
import os
import resource
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "flow-sim_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK_GBS = 8000.0        # MI355X: 8 TB/s HBM3E


def bench_channel(np):
    """node geometry of the benchmark's polyline channel (bench.py: build_batch, workload irr)"""
    from flowsim_amd.hydromodel import Boundary, Channel, Hydrograph, IrregularSection, PreissmannSolver
    Lc, S0c = 63500.0, 3e-4
    xa = np.array([0, 10, 14, 30, 34, 60, 66, 80.0]); za = np.array([8, 3.0, 0.4, 0.0, 0.6, 2.5, 2.8, 8.0])
    xb = np.array([0, 12, 18, 33, 41, 58, 70, 90.0]); zb = np.array([7.5, 2.6, 0.3, 0.0, 0.5, 2.0, 2.6, 7.5])
    secs = []
    for f, xx, zz in ((1.0, xa, za), (0.5, xb, zb), (0.0, xa * 1.1, za * 0.95)):
        s_ = IrregularSection(x=xx, z=S0c * Lc * f + zz, n=0.03, bed_slope=S0c)
        s_.set_roughness_para((0.05, 0.03, 0.06, xx[2], xx[5]))
        secs.append(s_)
    hyd = Hydrograph(table=np.array([[0.0, 45.0], [3000.0, 45.0]]))
    us = Boundary(condition='flow_hydrograph', bed_level=S0c * Lc, chainage=0, hydrograph=hyd, initial_depth=1.9)
    ds = Boundary(condition='normal_depth', bed_level=0.0, chainage=Lc, initial_depth=1.9)
    ch = Channel(initial_flow=45.0, upstream_boundary=us, downstream_boundary=ds, interpolation_method='steady-state')
    ch.set_cross_sections([0.0, 0.5 * Lc, Lc], secs)
    PreissmannSolver(channel=ch, theta=0.7, time_step=300, spatial_step=500, simulation_time=3000)
    return ch.node_geometry


def densify(np, geo, P):
    """the same channel surveyed at P stations per node: stations added evenly across each section, elevations on the polyline plus a
    ripple of a millimetre (distinct elevations: as many breakpoints as stations)"""
    N = len(geo["irr_npts"])
    X, Z = np.empty((N, P)), np.empty((N, P))
    for i in range(N):
        c = int(geo["irr_npts"][i])
        x, z = geo["irr_x"][i, :c], geo["irr_z"][i, :c]
        extra = np.linspace(x[0], x[-1], P - c + 2)[1:-1] + 0.013
        xs = np.sort(np.concatenate([x, extra]))
        X[i], Z[i] = xs, np.interp(xs, x, z) + 1e-3 * np.sin(np.arange(P) * 1.7 + i)
    out = dict(geo, irr_x=X, irr_z=Z, irr_npts=np.full(N, P, dtype=np.int32))
    out["z_bed"] = Z.min(axis=1)
    return out


def time_size(np, geo, B, rounds, label, first):
    from flowsim_amd import _pack
    from flowsim_amd.batch import PreissmannBatch
    N, P = geo["irr_x"].shape
    rng = np.random.default_rng(10)
    dzl, dzm, dzr = (rng.uniform(-0.3, 0.3, (B, N)) for _ in range(3))
    ns = rng.uniform(0.8, 1.25, (3, B))
    host, dev = (PreissmannBatch(B, N, 4, section_mode="irregular", monitor=False) for _ in range(2))

    def host_path():
        t0 = time.perf_counter()
        sections = _pack.member_sections(geo, B, dzl, dzm, dzr, ns)
        t1 = time.perf_counter()
        host.set_geometry_irregular(sections)
        host.sync()
        return t1 - t0, time.perf_counter() - t1

    def device_path():
        t0 = time.perf_counter()
        dev.set_geometry_irregular_members(geo, dzl, dzm, dzr, ns)
        dev.sync()
        return time.perf_counter() - t0, dev.last_step_ms()

    rss = lambda: resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0       # MiB (Linux: KiB)
    device_path()
    rss_device = rss()
    host_path()
    rss_host = rss()
    pack_s, set_s, dev_s, kern_ms = [], [], [], []
    for _ in range(rounds):
        a, u = host_path()
        d, k = device_path()
        pack_s.append(a); set_s.append(u); dev_s.append(d); kern_ms.append(k)
    assert host.poly_tables() == 1 and dev.poly_tables() == 1
    pick = [(int(r), int(i)) for r, i in zip(rng.integers(0, B, 64), rng.integers(0, N, 64))] + [(B - 1, N - 1)]
    same = all(np.array_equal(host.stage_table(r, i).view(np.uint64), dev.stage_table(r, i).view(np.uint64)) for r, i in pick)
    same = same and np.array_equal(host.bed_levels().view(np.uint64), dev.bed_levels().view(np.uint64))
    host.close(); dev.close()

    def stats(v, scale=1e3):
        v = np.array(v) * scale
        return dict(median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()), samples_ms=[round(float(x), 3) for x in v])
    stride = ((P + 16) & ~15) + 32 * P
    shared = (2 * P * N + 2 * N + 21 * N) * 8 + 4 * N
    up_host = B * (N * stride * 8 + shared)
    up_dev = shared + 3 * B * N * 8 + 3 * B * 8
    stored = B * (N * stride + 2 * P * N + 2 * N + 21 * N) * 8 + B * N * 4
    total_a = np.array(pack_s) + np.array(set_s)
    spread = max(total_a.max() - total_a.min(), max(dev_s) - min(dev_s))
    k_med = float(np.median(kern_ms))
    return dict(size=label, members=B, nodes=N, stations=P, rounds=rounds, table_doubles_per_node=stride,
                a_host_member_sections=stats(pack_s), a_host_set_geometry_irregular_per_reach=stats(set_s), a_host_total=stats(total_a),
                b_device_set_geometry_irregular_members=stats(dev_s), b_device_kernels=stats(kern_ms, 1.0),
                speedup_median=float(np.median(total_a) / np.median(dev_s)), spread_ms=float(spread * 1e3),
                b_clearly_faster=bool(np.median(total_a) - np.median(dev_s) > 3 * spread),
                uploaded_mb=dict(a_host=up_host / 1e6, b_device=up_dev / 1e6), device_bytes_stored_mb=stored / 1e6,
                kernels_store_gb_per_s=stored / 1e9 / (k_med * 1e-3), hbm_peak_gb_per_s=HBM_PEAK_GBS,
                kernels_store_fraction_of_hbm_peak=stored / 1e9 / (k_med * 1e-3) / HBM_PEAK_GBS,
                # (the peak is the process's: only the first size of a run can tell the two paths apart)
                peak_rss_mib=dict(after_device_path_only=rss_device, after_host_path=rss_host) if first else None,
                tables_of_65_sampled_nodes_and_all_bed_levels_bit_equal=bool(same))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--members", type=int, default=8192)
    ap.add_argument("--members40", type=int, default=2048, help="members of the 40-station size (0: leave it out)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import bench
    geo = bench_channel(np)
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    head = dict(tool="tools/time_geometry.py", date=time.strftime("%Y-%m-%d"), commit=commit, library_sha256=bench.library_sha256())
    reports = []
    for label, g, B in (("bench polyline ensemble", geo, args.members), ("40 stations", densify(np, geo, 40), args.members40)):
        if B > 0:
            reports.append(dict(head, **time_size(np, g, B, args.rounds, label, not reports)))
            print(json.dumps(reports[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(reports, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
