"""The dispatch table (TABLE) and the case that exercises each of its entries, shared by the instantiation suite
(tests/test_gpu_instantiations.py), the failure and iterate recipes built on it (tests/failure_recipes.py, tests/iterate_recipes.py)
and the GPU tests that run those.

The case for an entry follows from its attributes: section mode -> channel family, (cells per lane x waves per reach,
full / ragged) -> node count (full chunks: exactly the capacity; ragged: a few cells short of it, so the padding and
the lane that owns the last node move around), boundary class -> the boundary pair it was compiled for (class -1: the
general reservoir row it exists for; class 0 / 1: a different pair per shape so that every closed-form row and every
upstream kind runs somewhere)."""
import os

import numpy as np

from conftest import GOLDEN
from flowsim_amd import _abi as A
from kernel_harness import capacity, kernel_table
from oracle import c_oracle as CO
from oracle import preissmann_oracle as O
from synth import akbari_shape, normal_depth_rect, normal_depth_trap

TABLE = kernel_table()


def nodes(e):
    cap = capacity(e, one_grid=True)
    if e.get("team"):
        return 3 * cap if e["full"] else 2 * cap + cap // 5 + e["index"] % 9            # a team of three workgroups (ragged: the last one mostly padding)
    if e.get("long_reach"):
        return 2 * cap + cap // 3 + e["index"] % 7            # the multi-pass kernel (fs_long.hpp): three passes, the last one ragged
    if e["full"]:
        return cap
    n = max(2, cap - 1 - e["index"] % 5)             # ragged: 1..5 rows short of the capacity
    while e.get("tail", -1) >= 0 and (n - 1) % e["cells_per_thread"] != e["tail"]:
        n -= 1                                       # tail-only form: the boundary row sits in local row `tail` of its lane
    return n


# boundary pairs for the general classes, rotated over the entries: (upstream, downstream)
LIGHT_PAIRS = [("flow", "normal"), ("stage", "fixed"), ("flow", "poly"), ("fixed", "flow_ds"), ("normal_us", "stage_ds"),
               ("rating_us", "stage_ds"), ("flow", "storage"), ("flow", "blend")]
GENERAL_PAIRS = LIGHT_PAIRS + [("flow", "power")]


def hydrograph(Qb, nt, dt, amp=1.0):
    return np.array([akbari_shape(Qb, amp * Qb, 4 * dt, 12 * dt, k * dt) for k in range(nt)])


def prismatic_problem(e, pair, trapezoid, n_steps=4):
    """rectangular / simple trapezoidal prismatic reach with the boundary pair `pair`, started near uniform flow"""
    N = nodes(e)
    rng = np.random.default_rng(1000 + e["index"])
    b = rng.uniform(40, 120); n = rng.uniform(0.025, 0.035); S0 = rng.uniform(2e-4, 5e-4); m = rng.uniform(1, 2.5) if trapezoid else 0.0
    Qb = rng.uniform(1.0, 3.0) * b
    dx = 400.0 if N < 600 else 250.0
    dt = 900.0 if N < 600 else 600.0
    L = (N - 1) * dx
    geo = {k: np.zeros(N) for k in O.GEO_KEYS}
    geo["b_main"][:] = b; geo["m_main"][:] = m
    geo["n_main"][:] = n; geo["n_left"][:] = n; geo["n_right"][:] = n
    geo["z_bed"] = S0 * L * (1 - np.arange(N) / (N - 1))
    hn = normal_depth_trap(b, m, n, S0, Qb) if trapezoid else normal_depth_rect(b, n, S0, Qb)
    nt = n_steps + 1
    us_k, ds_k = pair
    if ds_k == "storage" and N > 130:
        # the reservoir row starts with the reference's level-1 quirk (vol_in forced to 0: the outflow reverses,
        # boundary.py:104-108), a transient Newton only gets through on short reaches
        ds_k = "normal"
    zu = S0 * L
    if us_k == "flow":
        us = O.BC("flow_hydrograph", bed_level=zu, target=hydrograph(Qb, nt, dt))
    elif us_k == "stage":
        us = O.BC("stage_hydrograph", bed_level=zu, target=zu + hn + 0.25 * hn * (hydrograph(1.0, nt, dt) - 1.0))
    elif us_k == "fixed":
        us = O.BC("fixed_depth", bed_level=zu, initial_depth=hn)
    elif us_k == "normal_us":
        us = O.BC("normal_depth", bed_level=zu, bed_slope=S0)
    elif us_k == "rating_us":        # head-dependent inflow: falls as the upstream stage rises
        us = O.BC("rating_curve", bed_level=zu, rc_type="polynomial", rc=dict(a=0.0, b=-0.2 * Qb, c=Qb + 0.2 * Qb * (zu + hn), shift=0.0))
    else:
        raise KeyError(us_k)
    if ds_k == "normal":
        ds = O.BC("normal_depth", bed_level=0.0, bed_slope=S0)
    elif ds_k == "fixed":
        ds = O.BC("fixed_depth", bed_level=0.0, initial_depth=hn)
    elif ds_k == "poly":
        ds = O.BC("rating_curve", bed_level=0.0, rc_type="polynomial", rc=dict(a=0.15 * Qb / hn ** 2, b=0.85 * Qb / hn, c=0.0, shift=0.0))
    elif ds_k == "power":
        ds = O.BC("rating_curve", bed_level=0.0, rc_type="power", rc=dict(a=Qb / hn ** 1.6, b=1.6, shift=0.0))
    elif ds_k == "flow_ds":          # gate closing: the outflow dips
        ds = O.BC("flow_hydrograph", bed_level=0.0, target=Qb * (1.0 - 0.3 * (hydrograph(1.0, nt, dt) - 1.0)))
    elif ds_k == "stage_ds":
        ds = O.BC("stage_hydrograph", bed_level=0.0, target=hn + 0.2 * hn * (hydrograph(1.0, nt, dt) - 1.0))
    elif ds_k == "storage":
        ds = O.BC("fixed_depth", bed_level=0.0, initial_depth=hn,
                  storage=dict(area=40.0 * b * L / 50.0, min_stage=0.5 * hn, Y_min=0.0, Y_max=50.0 * hn))
    elif ds_k == "blend":            # two quadratics blended over half a metre above the initial stage
        lo = [0.0, 0.9 * Qb / hn, 0.1 * Qb / hn ** 2]
        ds = O.BC("rating_curve", bed_level=0.0, rc_type="blend",
                  rc=dict(initial_stage=hn, buffer=0.5, low=lo, high=[2 * v for v in lo], dY=1e-3))
    else:
        raise KeyError(ds_k)
    return O.Problem(geo=geo, h0=np.full(N, hn), Q0=np.full(N, Qb), us=us, ds=ds, theta=0.65, dt=dt, dx=dx, nt=nt, tol=1e-6)


def fixture_problem(name, n_steps=None, member=None):
    fx, meta = O.load_fixture(os.path.join(GOLDEN, name + ".npz"))
    p = O.problem_from_fixture(fx, meta, member)
    if n_steps is not None:
        p.nt = min(p.nt, n_steps + 1)
    return p


def case_for(e):
    """(problem, section mode of the batch, n_main override) for a dispatch-table entry"""
    sec, bck, cap = e["section_mode"], e["boundary_class"], capacity(e, one_grid=True)
    if sec in (A.SEC_RECT_UNIFORM, A.SEC_TRAP_UNIFORM):
        trap = sec == A.SEC_TRAP_UNIFORM
        if bck >= 2:
            pair = ("flow", {A.BC_NORMAL_DEPTH: "normal", A.BC_RATING_POWER: "power", A.BC_RATING_BLEND: "blend"}[bck - 2])
        elif bck == 1:
            pair = LIGHT_PAIRS[e["index"] % len(LIGHT_PAIRS)]
        elif bck == 0:
            pair = GENERAL_PAIRS[e["index"] % len(GENERAL_PAIRS)]
        else:
            raise KeyError("no recipe: uniform-geometry kernels of class -1 do not exist")
        return prismatic_problem(e, pair, trap), ("trap_uniform" if trap else "rect_uniform"), None
    if sec == A.SEC_TABLE and e.get("long_reach"):
        # a long prismatic reach described as a table (the trapezoid-family code path of the multi-pass kernel, three passes)
        return prismatic_problem(e, GENERAL_PAIRS[e["index"] % len(GENERAL_PAIRS)], e["index"] % 2 == 0), "table", None
    if sec == A.SEC_TABLE:
        if bck == -1:      # the class exists for the general reservoir row: three reference fixtures, by capacity
            name = ("storage_curve_poly_losses", "storage_curve_power_trap", "storage_curve_closed")[e["index"] % 3]
            return fixture_problem(name, 10), "table", None
        if bck >= 2:
            assert bck - 2 == A.BC_RATING_BLEND and cap >= 120
            if e.get("tail", -1) == 1:      # an even node count: a prismatic trapezoid described as a table, blended rating curve downstream
                return prismatic_problem(e, ("flow", "blend"), True), "table", None
            return fixture_problem("gerd", 6), "table", None
        # class 0: compound sections going over bank where the capacity allows, else the table of a plain trapezoid
        # (fp32 cannot take the central difference of the Roseires gate curve: 1 mm on a stage of 487 m is 30 ulp)
        if cap >= 120 and e["index"] % 2 and e["dtype"] == A.F64:
            return fixture_problem("gerd", 5), "table", None
        return fixture_problem("bc_compound_normal" if e["index"] % 3 else "bc_trap_poly", 8), "table", None
    if sec == A.SEC_IRREGULAR:
        if bck == -1:
            return fixture_problem("irr_storage", 10), "irregular", None
        if bck >= 2:
            assert bck - 2 == A.BC_NORMAL_DEPTH
            return fixture_problem(("irr_single", "irr_mixed")[e["index"] % 2], 8), "irregular", None
        return fixture_problem(("irr_levee", "irr_mixed", "irr_single")[e["index"] % 3], 8), "irregular", None
    raise KeyError(f"no recipe for section mode {sec}")


def oracle_run(p):
    """C oracle where it applies (trapezoid family, closed-form boundaries), the numpy one otherwise"""
    general_storage = p.ds.storage is not None and any(p.ds.storage.get(k) is not None for k in ("curve", "rc", "losses"))
    if "irr_npts" in p.geo or general_storage:
        return O.newton_run(p)
    return CO.run(p)


# ---- a SECOND recipe for the entries whose node evaluation is the intricate one (tables, polylines) ----
# Round 3's (8, 1) polyline kernel was right or wrong depending on code the case never executed: one case per entry is a thin net
# for a miscompile.  The second case comes from the reference's own random sweep (tests/golden/random_sweep.npz: the reference
# built these channels and ran them; compared here with ITS histories, not an oracle's): other sections, other boundary kinds,
# other node counts than the first recipe's.
SWEEP = {i: (fx, m) for i, fx, m in O.sweep_cases(os.path.join(GOLDEN, "random_sweep.npz"))}
SECOND_POLY = {-1: [58, 50, 52, 55], 0: [50, 52, 53, 58, 55, 48], 2: [54, 57]}           # by boundary class (2: flow upstream, normal depth downstream)
SECOND_TABLE = {-1: [61, 62, 65, 70, 68, 60], 0: [78, 79, 8, 10, 24, 3, 75, 21, 12]}      # general storages; compound sections, bends


def second_case_for(e):
    """(problem, mode, reference arrays or None) - None: compare with the oracle"""
    sec, bck = e["section_mode"], e["boundary_class"]
    cap = capacity(e)            # (no table or polyline entry is a team entry)
    if sec == A.SEC_TABLE and e.get("long_reach"):
        pair = GENERAL_PAIRS[(e["index"] + 4) % len(GENERAL_PAIRS)]
        return prismatic_problem(e, pair, e["index"] % 2 == 1, n_steps=3), "table", None
    if sec == A.SEC_TABLE and bck >= 2:
        if e.get("tail", -1) == 1:
            return prismatic_problem(dict(e, index=e["index"] + 2), ("flow", "blend"), False, n_steps=5), "table", None
        return fixture_problem("gerd_ensemble", 5, member=e["index"] % 8), "table", None
    pool = (SECOND_TABLE if sec == A.SEC_TABLE else SECOND_POLY)[min(bck, 2)]
    fits = [i for i in pool if SWEEP[i][1]["N"] <= cap]
    if e["dtype"] == A.F32:       # fp32 follows a flood wave, not one that stalls and reverses (a stage-driven case of the sweep does): those stay with fp64
        fits = [i for i in fits if float(np.min(SWEEP[i][0]["flow"])) > 0.3 * SWEEP[i][1]["Qb"]] or fits
    i = fits[e["index"] % len(fits)]
    fx, m = SWEEP[i]
    return O.problem_from_fixture(fx, m), ("table" if sec == A.SEC_TABLE else "irregular"), (fx, m)
