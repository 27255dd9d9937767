#!/usr/bin/env python3
"""Backwater initial conditions of the sweep's polyline channels, from the reference itself.

    python3 tools/gen_init_state_golden.py --reference DIR      (DIR: a checkout of cve-mohd/flow-sim)

tests/golden/random_sweep.npz holds 12 channels of polyline sections, none of which starts from a backwater profile (their recipes
drew 'steady-state' or 'linear').  This runs the reference's Channel.initialize_conditions on those 12 recipes with the method forced
to 'GVF_equation' and stores only the resulting initial_conditions [N, 2] per case, under the case's index in the sweep, in
tests/golden/init_state_polyline.npz - geometry, grid and flow are the sweep's own.  tests/test_gpu_init_state.py holds the device
march to this file (stage tables and edge walk), tests/test_init_state_host.py the host mirror."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("FLOWSIM_REFERENCE"), help="checkout of the reference (its src/hydromodel is imported)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "init_state_polyline.npz"))
    a = ap.parse_args()
    if not a.reference or not os.path.isdir(os.path.join(a.reference, "src", "hydromodel")):
        sys.exit("--reference DIR (or FLOWSIM_REFERENCE) must name a checkout of the reference")
    out_path = os.path.abspath(a.out)
    sys.dont_write_bytecode = True
    os.environ.setdefault("MPLBACKEND", "Agg")
    # (the repository root stays off sys.path: its src/ is a regular package and would shadow the reference's namespace package)
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_random_sweep", os.path.join(ROOT, "oracle", "gen_random_sweep.py"))
    sweep_gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sweep_gen)
    build_from_recipe = sweep_gen.build_from_recipe
    sweep = json.loads(str(np.load(os.path.join(ROOT, "tests", "golden", "random_sweep.npz"))["meta"]))["cases"]
    cases = [(i, m) for i, m in enumerate(sweep) if m["family"] == "polyline"]
    os.chdir(a.reference)
    sys.path.insert(0, os.path.abspath(a.reference))         # `src.hydromodel` is the reference's
    arrays, metas = {}, []
    for i, m in cases:
        recipe = dict(m["recipe"], ic="GVF_equation")
        sol, _, _ = build_from_recipe(recipe)
        assert type(sol).__module__.startswith("src."), "the reference, not the mirror"
        assert sol.number_of_nodes == m["N"]
        if not sol.channel.conditions_initialized:
            sol.channel.initialize_conditions(sol.number_of_nodes)
        ic = np.asarray(sol.channel.initial_conditions, dtype=np.float64)
        assert ic.shape == (m["N"], 2) and np.all(np.isfinite(ic))
        arrays[f"c{i:02d}_initial_conditions"] = ic
        metas.append(dict(case=i, N=m["N"], dx=m["dx"], Qb=m["Qb"]))
        print(f"  case {i:02d}: N={m['N']:4d} depth {ic[:, 0].min():.3f} .. {ic[:, 0].max():.3f}")
    meta = dict(generator="tools/gen_init_state_golden.py", reference="cve-mohd/flow-sim snapshot 2026-02-13",
                source="tests/golden/random_sweep.npz: the polyline recipes, ic forced to GVF_equation", cases=metas)
    np.savez_compressed(out_path, meta=np.array(json.dumps(meta)), **arrays)
    print(f"wrote {out_path} ({os.path.getsize(out_path) / 1024:.1f} KiB): {len(metas)} cases")


if __name__ == "__main__":
    main()
