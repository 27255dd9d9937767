#!/usr/bin/env python3
"""Level-pool routing of the GERD reservoir, from the reference itself.

    python3 tools/gen_pool_routing_golden.py --reference DIR      (DIR: a checkout of cve-mohd/flow-sim)

Runs the reference's GerdHydrograph.build (cases/gerd_roseires/gerd_discharge.py:12-56) on the shipped inflow table, scaled, shifted
and started from different pool levels, and writes tests/golden/pool_routing.npz - data only: per member the release table, the pool
stage and brentq's evaluation count of every level.  The reference keeps neither stage nor count: both are taken where its own code
produces them, by handing its module a brentq that calls scipy's with full_output and passes the root on.  One member is chosen such
that the reference raises ValueError (no bracket); the level at which it does is recorded.  Every member is routed a second time with
every outlet evaluation disturbed by up to 4 eps; a member whose release moves by 1e-13 or more under that is not kept."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
INFLOW = "cases/gerd_roseires/data/inflow_hydrograph.csv"
DT, LEVELS = 3600, 385

# (inflow scale, shift [s], initial level [m]); the last one is the member without a bracket
MEMBERS = [(1.0, 0.0, 637.0), (0.25, 0.0, 637.0), (0.5, 5400.0, 640.0), (0.75, -5400.0, 630.0), (1.0, 5400.0, 625.0),
           (1.25, 0.0, 628.0), (1.5, -5400.0, 634.0), (1.75, 0.0, 639.5), (2.0, 5400.0, 641.0), (2.25, 0.0, 642.5),
           (2.5, -5400.0, 643.0), (3.0, 0.0, 643.0), (3.0, 5400.0, 637.0), (2.75, 0.0, 632.0), (0.25, -5400.0, 643.0),
           (0.5, 0.0, 626.0), (1.0, -5400.0, 641.5), (1.5, 5400.0, 636.0), (2.0, 0.0, 625.0), (0.75, 0.0, 638.0),
           (1.25, 5400.0, 642.0), (2.5, 0.0, 640.0), (3.0, -5400.0, 631.0), (0.25, 0.0, 625.0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("FLOWSIM_REFERENCE"), help="checkout of the reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "pool_routing.npz"))
    a = ap.parse_args()
    if not a.reference or not os.path.isdir(os.path.join(a.reference, "src", "hydromodel")):
        sys.exit("--reference DIR (or FLOWSIM_REFERENCE) must name a checkout of the reference")
    out_path = os.path.abspath(a.out)
    sys.dont_write_bytecode = True
    os.chdir(a.reference)
    sys.path.insert(0, os.path.abspath(a.reference))
    import pandas
    import scipy.optimize
    real_read = pandas.read_csv

    def read_csv(path, *args, **kw):          # the case modules name their tables with '\\' (oracle/gen_golden.py does the same)
        return real_read(path.replace("\\", "/") if isinstance(path, str) else path, *args, **kw)

    import cases.gerd_roseires.gerd_discharge as gd
    import cases.gerd_roseires.custom_functions as cf
    from src.hydromodel.hydrograph import Hydrograph
    gd.read_csv = read_csv
    cf.read_csv = read_csv
    assert gd.__file__.startswith(os.path.abspath(a.reference)), "the reference, not the mirror"
    table = cf.import_hydrograph(INFLOW)
    curve = real_read("cases/gerd_roseires/data/gerd_vol_curve.csv", header=None).to_numpy(dtype=np.float64)
    record = []

    def brentq(f, a, b):
        root, r = scipy.optimize.brentq(f, a, b, full_output=True)
        record.append((root, r.function_calls))
        return root

    gd.brentq = brentq

    def route(scale, shift, level, noise=None):
        """(release [n], stage [n], evals [n], first level without a bracket or -1)"""
        del record[:]
        hyd = gd.GerdHydrograph()
        if noise is not None:
            clean = hyd.effective_capacity
            hyd.effective_capacity = lambda WL, **kw: clean(WL, **kw) * (1.0 + 4 * EPS * noise.uniform(-1.0, 1.0))
        inflow = Hydrograph(function=lambda t: scale * float(np.interp(t - shift, table[:, 0], table[:, 1])))
        failed = -1
        try:
            hyd.build(inflow_hydrograph=inflow, time_step=DT, duration=(LEVELS - 1) * DT, initial_stage=level)
        except ValueError:
            failed = len(record) + 1
        n = LEVELS if failed < 0 else failed
        stage = np.array([level] + [r[0] for r in record])[:n]
        evals = np.array([0] + [r[1] for r in record])[:n]
        return hyd.table[:n, 1].copy(), stage, evals, failed

    rng = np.random.default_rng(20260213)
    release = np.full((LEVELS, len(MEMBERS)), np.nan)
    stage = np.full((LEVELS, len(MEMBERS)), np.nan)
    evals = np.zeros((LEVELS, len(MEMBERS)), dtype=np.int32)
    spread = np.zeros(len(MEMBERS))
    failed = np.full(len(MEMBERS), -1, dtype=np.int32)
    tags = []
    kept = []
    for m, (scale, shift, level) in enumerate(MEMBERS):
        # a member whose release moves by 1e-13 or more under the noise, or whose evaluation path the noise changes, is replaced: the
        # same inflow from a pool 0.125 m higher, until one holds
        for attempt in range(8):
            q, z, ev, failed[m] = route(scale, shift, level)
            qn, zn, evn, fn = route(scale, shift, level, noise=rng)
            steady = fn == failed[m] and np.array_equal(evn, ev)
            spread[m] = np.max(np.abs(qn - q) / np.abs(q)) if steady else np.inf
            if spread[m] < 1e-13:
                break
            print(f"  member {m:2d} at level {level}: {'release moves by %.1e' % spread[m] if steady else 'the noise changes the path'} - replaced")
            level += 0.125
        assert spread[m] < 1e-13, f"member {m}: no replacement found"
        kept.append((scale, shift, level))
        n = len(q)
        release[:n, m], stage[:n, m], evals[:n, m] = q, z, ev
        above = z > level
        tag = ("no_bracket" if failed[m] >= 0 else "holds" if not above.any() else
               "crosses" if np.any(above[1:] & ~above[:-1]) and np.any(~above[1:] & above[:-1]) else "rises")
        tags.append(tag + ("+emergency" if np.nanmax(z) > 642.0 else ""))
        print(f"  member {m:2d}: scale {scale:4.2f} shift {shift:7.0f} level {level:5.1f}  {tags[-1]:22s} stage {np.nanmin(z):.3f} .. "
              f"{np.nanmax(z):.3f}  evals {int(ev.sum())}  noise {spread[m]:.1e}  no bracket at {failed[m]}")
    for need in ("holds", "crosses", "emergency", "no_bracket"):
        assert any(need in t for t in tags), need
    assert np.sum(failed >= 0) == 1 and failed[-1] >= 2
    meta = dict(kind="pool_routing", generator="tools/gen_pool_routing_golden.py", reference="cve-mohd/flow-sim snapshot 2026-02-13",
                source="GerdHydrograph.build on " + INFLOW, dt=DT, levels=LEVELS, tags=tags)
    params = np.array(kept, dtype=np.float64)
    np.savez_compressed(out_path, meta=np.array(json.dumps(meta)), inflow_table=table, curve_volume=curve[:, 0], curve_stage=curve[:, 1],
                        scale=params[:, 0], shift=params[:, 1], initial_stage=params[:, 2], release=release, stage=stage, evals=evals,
                        noise_spread=spread, no_bracket_level=failed)
    print(f"wrote {out_path} ({os.path.getsize(out_path) / 1024:.1f} KiB): {len(MEMBERS)} members")


if __name__ == "__main__":
    main()
