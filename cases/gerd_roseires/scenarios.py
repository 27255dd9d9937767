"""python -m cases.gerd_roseires.scenarios  -  a scenario sweep of the GERD -> Roseires reach: the tabulated inflow into GERD scaled
0.5 .. 2, from initial GERD levels of 630 .. 642 m, every combination one member of a device batch.  Each member's release is
routed through its own pool on the device (flowsim_amd.ensemble.run_scenario_ensemble); the script prints the cross-member bands of
the Roseires outflow and of the volume stored in the reach, and how well every member's discrete water balance closed (the state is
marked every `every` levels: PreissmannBatch.reach_integrals / water_balance).  The reference runs such a study one member at a time (gerd_discharge.py:12-56, then model.py:36-113)."""
import argparse

import numpy as np

import src  # noqa: F401  (puts the flowsim_amd package on the import path)
from flowsim_amd import _abi as A
from flowsim_amd.ensemble import run_scenario_ensemble

from . import settings
from .gerd_discharge import GerdHydrograph
from .inputs import import_hydrograph
from .model import build


def sweep(n_scales=8, n_levels=8, hours=None, every=24, quantiles=(0.05, 0.5, 0.95)):
    """(result of run_scenario_ensemble, inflow scales [B], initial levels [B])"""
    table = import_hydrograph(settings.inflow_hyd_path)
    duration = int(table[-1, 0]) if hours is None else int(hours * 3600)
    solver, _ = build(inflow_hyd_func=None, sim_duration=duration)
    scales, levels = np.meshgrid(np.linspace(0.5, 2.0, n_scales), np.linspace(630.0, 642.0, n_levels), indexing="ij")
    scales, levels = scales.ravel(), levels.ravel()
    res = run_scenario_ensemble(solver, GerdHydrograph.pool_spec(), table, inflow_scale=scales, pool_level=levels,
                                tolerance=settings.tolerance, bands=quantiles, summaries=True, hydrographs=False,
                                balance=dict(every=every, quantiles=quantiles))
    return res, scales, levels


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scales", type=int, default=8, help="inflow scales between 0.5 and 2")
    ap.add_argument("--levels", type=int, default=8, help="initial GERD levels between 630 and 642 m")
    ap.add_argument("--hours", type=float, default=None, help="simulated time (default: the inflow table's)")
    ap.add_argument("--every", type=int, default=24, help="print every n-th level")
    a = ap.parse_args()
    q = (0.05, 0.5, 0.95)
    res, scales, levels = sweep(a.scales, a.levels, a.hours, a.every, q)
    ok = np.isin(res["status"], (A.OK, A.ILL_CONDITIONED))
    print(f"{len(scales)} members: inflow x {scales.min():g} .. {scales.max():g}, GERD at {levels.min():g} .. {levels.max():g} m; "
          f"{int(np.sum(~ok))} failed, {int(np.sum(res['pool']['flags'] != 0))} pools left their bracket")
    print(f"release at t = 0: {res['initial_flow'].min():.1f} .. {res['initial_flow'].max():.1f} m3/s; "
          f"peak Roseires outflow {np.nanmin(res['summaries']['peak_q_out'][ok]):.1f} .. {np.nanmax(res['summaries']['peak_q_out'][ok]):.1f} m3/s")
    bands = res["bands"]
    print("Roseires outflow across the members [m3/s]")
    print(f"{'hour':>6} {'members':>8} {'min':>10} " + " ".join(f"{'q%02d' % round(100 * x):>10}" for x in q) + f" {'max':>10} {'mean':>10}")
    dt_h = settings.time_step / 3600.0
    for k in range(0, len(bands["n_members"]), a.every):
        row = bands["quantiles"][k, A.ROW_Q_OUT]
        print(f"{k * dt_h:6.0f} {bands['n_members'][k]:8d} {bands['min'][k, A.ROW_Q_OUT]:10.1f} " + " ".join(f"{v:10.1f}" for v in row) +
              f" {bands['max'][k, A.ROW_Q_OUT]:10.1f} {bands['mean'][k, A.ROW_Q_OUT]:10.1f}")
    bal = res["balance"]
    vol, i_vol = bal["bands"], A.INT_ROWS.index("volume")
    print("volume stored in the reach across the members [1e6 m3]")
    print(f"{'hour':>6} {'members':>8} {'min':>10} " + " ".join(f"{'q%02d' % round(100 * x):>10}" for x in q) + f" {'max':>10} {'mean':>10}")
    for k in range(0, len(vol["n_members"]), a.every):      # (the levels at which the state was marked)
        row = vol["quantiles"][k, i_vol] / 1e6
        print(f"{k * dt_h:6.0f} {vol['n_members'][k]:8d} {vol['min'][k, i_vol] / 1e6:10.3f} " + " ".join(f"{v:10.3f}" for v in row) +
              f" {vol['max'][k, i_vol] / 1e6:10.3f} {vol['mean'][k, i_vol] / 1e6:10.3f}")
    tot = bal["totals"]
    if np.any(ok & (tot["spans"] > 0)):
        worst = np.where(ok & (tot["spans"] > 0), tot["worst"], -np.inf)
        r = int(np.argmax(worst))
        print(f"water balance over {int(tot['spans'][r])} spans of {a.every} levels: worst closure {worst[r]:.3g} m3 (member {r}, span ending at hour "
              f"{tot['worst_level'][r] * dt_h:.0f}; its inflow volume {tot['inflow'][r]:.4g} m3, summed residual {tot['residual'][r]:.3g} m3)")


if __name__ == "__main__":
    main()
