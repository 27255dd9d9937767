#!/usr/bin/env python3
"""What one ensemble Kalman analysis (fs_batch_assimilate) costs on the device, against the copy rate of the card.

Two sizes, both fp64, RECT_UNIFORM members of one channel with a random positive state (the kernels' time does not depend on the
values): 32 768 members x 121 nodes with 4 observations, and 8 192 members x 4 096 nodes with 16.  The time is the handle's own -
fs_batch_last_step_ms after the call: HIP events around the moments, combine and update kernels, without the gather, the host part
and the transfers - over --repeats calls after --warmup untimed ones; the report holds every sample, the median and min .. max.

Algorithmic bytes, counted from the shapes: the state (h and Q, B N values each) read once for the moments; hk, hg, Qk and Qg read
and written once each by the update (the state read and written twice); the partial sums [chunks][2][m + 2][N] written by the
moments and read by the combine.  (S, Z, the taper and the outputs are smaller by a factor of B or more and are left out.)  The
fraction is those bytes over the time over 6.29 TB/s, the float4 copy rate measured on the MI355X.

Every size runs in a child process of its own under a time limit; a child that fails ends the run.  One line per size on stdout, the
report written to --out as text.

    python3 tools/assim_rate.py --out profiles/round16/assim_rate.txt"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "flow-sim_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

COPY_RATE = 6.29e12                                      # bytes / s
SIZES = [(32768, 121, 4), (8192, 4096, 16)]


def algorithmic_bytes(B, N, m, esz=8):
    chunks = -(-B // 256)
    state = 2 * B * N * esz
    return dict(moments_read=state, update_read_write=4 * state, partials=2 * chunks * 2 * (m + 2) * N * 8)


def measure(B, N, m, warmup, repeats):
    import numpy as np
    from flowsim_amd import _abi as A
    from flowsim_amd.assimilation import Observation, perturbations
    from flowsim_amd.batch import BoundarySpec, PreissmannBatch
    rng = np.random.default_rng(1)
    with PreissmannBatch(B, N, 2, dtype="f64", section_mode="rect_uniform") as b:
        b.set_scheme(0.6, 600.0, 250.0)
        b.set_geometry_uniform(np.full(B, 50.0), 0.03 * rng.uniform(0.8, 1.6, B), np.full(B, 2e-4 * 250.0 * (N - 1)), np.zeros(B))
        b.set_boundary(A.UPSTREAM, BoundarySpec(A.BC_FLOW_HYDROGRAPH, {}, np.full((2, B), 60.0)))
        b.set_boundary(A.DOWNSTREAM, BoundarySpec(A.BC_NORMAL_DEPTH, dict(bed_slope=np.full(B, 2e-4), bed_level=np.zeros(B))))
        h = 2.5 + 0.3 * rng.standard_normal((B, 1)) + 0.05 * rng.standard_normal((B, N))
        Q = 60.0 + 5.0 * rng.standard_normal((B, 1)) + 0.5 * rng.standard_normal((B, N))
        b.set_state(np.maximum(h, 0.2), Q)
        del h, Q
        G = min(m, 16)
        node = np.array([(g + 1) * (N - 1) // (G + 1) for g in range(G)], dtype=np.int32)
        b.set_gauges(node=node, weight=np.full(G, 0.25))
        signals = ("stage", "flow", "depth", "velocity")
        variance = dict(stage=0.01, flow=4.0, depth=0.01, velocity=0.0025)
        b.gauges(current=True)
        obs = []
        for j in range(m):
            s = signals[j % 4]
            obs.append(Observation(j % G, s, float(np.mean(b.gauge_rows(j % G, 0, 1)[0][A.GAUGE_ROWS.index(s)])), variance[s]))
        pert = perturbations(2, [o.variance for o in obs], B)
        ms, n_active = [], None
        for k in range(warmup + repeats):
            out = b.assimilate(obs, pert)
            n_active = out["n_active"]
            if k >= warmup:
                ms.append(b.last_step_ms())
    parts = algorithmic_bytes(B, N, m)
    total = sum(parts.values())
    med = statistics.median(ms)
    return dict(B=B, N=N, m=m, dtype="f64", n_active=n_active, warmup=warmup, repeats=repeats, kernels_ms=ms, median_ms=med, min_ms=min(ms), max_ms=max(ms),
                bytes=parts, total_bytes=total, rate_TB_s=total / (med * 1e-3) / 1e12, fraction_of_copy_rate=total / (med * 1e-3) / COPY_RATE)


def line(r):
    return (f"{r['B']} members x {r['N']} nodes, {r['m']} observations, {r['dtype']}: moments + combine + update {r['median_ms']:.3f} ms median of "
            f"{r['repeats']} ({r['min_ms']:.3f} .. {r['max_ms']:.3f}) after {r['warmup']} warm-up calls; {r['total_bytes'] / 1e9:.3f} GB algorithmic "
            f"-> {r['rate_TB_s']:.2f} TB/s = {100 * r['fraction_of_copy_rate']:.0f} % of the 6.29 TB/s copy rate; {r['n_active']} active members")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--child", nargs=3, type=int, default=None, metavar=("B", "N", "M"))
    ap.add_argument("--timeout", type=float, default=240.0)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(*a.child, a.warmup, a.repeats)))
        return 0
    lines = []
    for B, N, m in SIZES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(B), str(N), str(m), "--warmup", str(a.warmup), "--repeats",
                            str(a.repeats)], capture_output=True, text=True, timeout=a.timeout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-3000:])
            return r.returncode or 1
        res = json.loads(r.stdout.strip().splitlines()[-1])
        lines += [line(res), "  samples (ms): " + " ".join(f"{v:.3f}" for v in res["kernels_ms"]),
                  "  bytes: " + ", ".join(f"{k} {v}" for k, v in res["bytes"].items())]
        print(lines[-3], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("tools/assim_rate.py: fs_batch_assimilate, kernel time from fs_batch_last_step_ms (HIP events)\n" + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
