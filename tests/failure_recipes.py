"""Data-only recipes that drive a reach into each failure exit of the step kernels (FS_NAN, FS_MAX_ITER,
FS_STORAGE_RANGE) at a level chosen by the test - shared by tests/test_failure_recipes.py, which checks on the CPU oracle
that every recipe fails where and how it is meant to, with margins, and tests/test_gpu_failure_exits.py, which runs them.

The cases are those of tests/entry_recipes.py (case_for: the smallest reach that fits each dispatch-table entry).
Every constant below was picked with the oracle alone; the margins it produced are written next to it and asserted by
tests/test_failure_recipes.py for every entry."""
import copy
import functools

import numpy as np

from entry_recipes import TABLE, case_for, fixture_problem, oracle_run, prismatic_problem  # noqa: F401
from flowsim_amd import _abi as A
from kernel_harness import entry_id, f32_of, find_entry  # noqa: F401
from oracle import preissmann_oracle as O

K_STAR = 2            # the failing level: level 1 converges before it, levels 3.. would follow in the same launch
MARGIN = 100.0        # the factor the issue sets: decisions of the oracle that fp32 has to repeat are off the threshold by this much
STATUS = {"nan": 2, "maxiter": 1, "storage": 3}


def suite_case(e):
    """the instantiation suite's case for the entry, with its fp32 tolerance"""
    p, mode, override = case_for(e)
    if f32_of(e):
        p.tol = 1e-3 if p.N <= 600 else 2e-2
    return p, mode, override


def target_side(p):
    """the boundary whose hydrograph the recipe edits: upstream if it has one"""
    side = "us" if p.us.target is not None else "ds"
    assert getattr(p, side).target is not None, "the case has no hydrograph at either end"
    return side


def edited(p, k, value):
    """a copy of the problem whose target hydrograph holds `value` at level k"""
    q = copy.deepcopy(p)
    bc = getattr(q, target_side(q))
    bc.target = np.array(bc.target, dtype=np.float64)
    bc.target[k] = value
    return q


# ---- FS_NAN: the target is NaN at K_STAR; the residual norm of the first iteration of that level is NaN ----
def nan_case(e):
    p, mode, override = suite_case(e)
    return p, edited(p, K_STAR, np.nan), mode, override


# ---- FS_MAX_ITER: a finite jump of the target at K_STAR, max_iter = the largest count of the levels before ----
# Newton's convergence on the prismatic and the mixed-polyline cases is quadratic: ||R|| falls 2e1 -> 5e-3 -> 5e-7 -> the rounding
# floor (<= 3e-11 at 12 288 nodes), so a tolerance can sit a factor 100 away from the norms on both sides of it.
# fp64: 1e-8 - every level before K_STAR then takes 4 iterations, its last norm is <= 3e-3 tol (worst: the 12 288-node team entry)
#       and the one before >= 10 tol.
# fp32: the norm cannot be resolved below ~1e-3 at 4 096 nodes (6e-8 |Q| sqrt(2N)), which rules out the gap 5e-3 .. 5e-7 for it;
#       2.0 sits in the gap above: level 1 takes 2 iterations, its last norm is <= 6e-3 tol and its first >= 2.5 tol.
MAXITER_TOL = {"f64": 1e-8, "f32": 2.0}
# the jump: an inflow hydrograph is multiplied, an outflow hydrograph (gate) is cut, a stage hydrograph is raised by a multiple of
# the depth there.  With them the norm of iteration max_iter at K_STAR is >= MARGIN tol for every entry (margins: see
# tests/test_failure_recipes.py, which prints them with -s), and every iterate up to there is finite.
JUMP_INFLOW = {"f64": 5.0, "f32": 60.0}           # target *= this
JUMP_OUTFLOW = {"f64": 0.2, "f32": 0.2}           # target *= this
JUMP_STAGE = {"f64": 2.0, "f32": 2.0}             # target += this * depth at that end


# Why the max-iter exit of an entry does not run the suite's own case, by what that case is (the NaN exit runs it on every entry).
# Where the reference's own Newton converges linearly - its Jacobian is inexact there, ||R|| falls by 0.3 .. 0.6 per iteration - NO
# tolerance is a factor 100 away from the norms on both sides, so the entry runs a case of the same section mode that converges
# quadratically: a prismatic channel with an inflow hydrograph (tables: a trapezoid described as a table), polylines the mixed fixture.
SUBSTITUTED = {
    "polyline": "levee sections converge linearly; the single-polyline fixture's third norm, 8e-9, sits on the fp64 tolerance",
    "reservoir": "the first level of every reservoir converges linearly (17 .. 94 iterations)",
    "fixture table": "compound sections and the Roseires gate curve converge linearly",
    "fp32 from downstream": "fp32 and no hydrograph upstream: the first norm of a level is too small for the fp32 tolerance to sit below it",
    "fp32 stage": "fp32 and a stage hydrograph upstream: the first norm of a level is 8e-2 (metres), likewise",
}


def substituted(e):
    """the key of SUBSTITUTED that applies to the entry's suite case, or None: the max-iter exit runs that case"""
    p, _, _ = suite_case(e)
    if e["section_mode"] == A.SEC_IRREGULAR:
        return "polyline"
    if p.ds.storage is not None:
        return "reservoir"
    if e["section_mode"] == A.SEC_TABLE:
        compound = bool(np.any(p.geo["is_compound"] > 0.5))
        if compound or np.ptp(p.geo["b_main"]) != 0:
            return "fixture table"
    if f32_of(e) and p.us.target is None:
        return "fp32 from downstream"
    if f32_of(e) and p.us.kind == "stage_hydrograph":
        return "fp32 stage"
    return None


def maxiter_base(e):
    """(problem, mode, override) the max-iter exit runs on: the suite's case or its substitute, at the max-iter tolerance"""
    p, mode, override = suite_case(e)
    sec, why = e["section_mode"], substituted(e)
    if why == "polyline":
        p = fixture_problem("irr_mixed", 8)
    elif why is not None:
        if e["boundary_class"] >= 2:           # the pair the kernel was compiled for
            downstream = {A.BC_NORMAL_DEPTH: "normal", A.BC_RATING_POWER: "power", A.BC_RATING_BLEND: "blend"}[e["boundary_class"] - 2]
        else:
            downstream = ("normal", "poly", "power", "blend")[e["index"] % 4]
        p = prismatic_problem(e, ("flow", downstream), sec != A.SEC_RECT_UNIFORM)
        mode = {A.SEC_RECT_UNIFORM: "rect_uniform", A.SEC_TRAP_UNIFORM: "trap_uniform", A.SEC_TABLE: "table"}[sec]
    p.tol = MAXITER_TOL["f32" if f32_of(e) else "f64"]
    return p, mode, override


def jumped(p, dtype):
    side = target_side(p)
    bc = getattr(p, side)
    t = float(bc.target[K_STAR])
    if bc.kind == "flow_hydrograph":
        v = t * (JUMP_INFLOW if side == "us" else JUMP_OUTFLOW)[dtype]
    else:
        v = t + JUMP_STAGE[dtype] * float(p.h0[0 if side == "us" else -1])
    return edited(p, K_STAR, v)


@functools.lru_cache(maxsize=None)
def _maxiter_count(index):
    e = TABLE[index]
    p, _, _ = maxiter_base(e)
    ref = oracle_run(_upto(p, K_STAR))
    assert ref["status"] == 0
    return int(max(ref["iters"][1:K_STAR]))


def _upto(p, k):
    q = copy.copy(p)
    q.nt = min(p.nt, k + 1)
    return q


def maxiter_case(e):
    """(failure-free problem, failing problem, mode, override): both run with the tolerance above; the failing one with
    max_iter = the largest count the oracle needs before K_STAR"""
    p, mode, override = maxiter_base(e)
    bad = jumped(p, "f32" if f32_of(e) else "f64")
    bad.max_iter = _maxiter_count(e["index"])
    return p, bad, mode, override


def case(e, exit_):
    return {"nan": nan_case, "maxiter": maxiter_case}[exit_](e)


# ---- FS_STORAGE_RANGE: the bracket [Y_min, Y_max] of the reservoir is tightened so that the stage leaves it at a known iteration ----
def _plain(dtype, sec, M, W, bck, **more):
    return find_entry(dtype=A.F64 if dtype == "f64" else A.F32, section_mode=sec, cells_per_thread=M, waves_per_reach=W, boundary_class=bck,
                      diag=1, long_reach=0, team=0, **more)


def closed_form_reservoir(e):
    """the suite's prismatic rectangle of the entry's size behind the suite's closed-form reservoir (prismatic_problem swaps the
    reservoir out above 130 nodes because its first level does not converge there - which this exit does not need)"""
    p = prismatic_problem(e, ("flow", "normal"), False)
    hn, b, L = float(p.h0[0]), float(p.geo["b_main"][0]), (p.N - 1) * p.dx
    p.ds = O.BC("fixed_depth", bed_level=0.0, initial_depth=hn, storage=dict(area=40.0 * b * L / 50.0, min_stage=0.5 * hn, Y_min=0.0, Y_max=50.0 * hn))
    return p


# Y_max per case, and what the oracle's reservoir stage does around it (tests/test_failure_recipes.py asserts these margins; the
# parity tolerance is 1e-8, so MARGIN asks for 1e-6 relative):
STORAGE_Y_MAX = {
    # short reach, tolerance 1e-3 (level 1 takes 94 iterations, the later ones 4): every stage of levels 1 - 2 is <= 3.90116, level 3
    # evaluates 3.92490 (inside by 1.3e-3) and then 3.93567 (outside by 1.4e-3): level 3, iteration 2
    "one_wave": 3.930,
    # 4 095 nodes: level 1 does not converge, its stages climb by 1.66e-3 per iteration: 2.616271 (inside by 3.2e-4), 2.617936 (outside by 3.2e-4): level 1, iteration 3
    "multi_wave": 2.6171,
    # 4 096 nodes, the shape of the compiled flow / normal-depth pair kernels: 2.438619 inside by 4.0e-4, 2.440562 outside by 3.9e-4: level 1, iteration 3
    "pair_excluded": 2.4396,
    # 9 013 nodes, a team of three workgroups: 1.364727 inside by 1.3e-4, 1.365063 outside by 1.2e-4: level 1, iteration 3
    "team": 1.3649,
    # 4 781 nodes in three passes: 2.120268 inside by 3.9e-4, 2.122017 outside by 4.3e-4: level 1, iteration 3
    "long": 2.1211,
    # general reservoir (area curve, rated outflow, losses) behind a trapezoid table: stages of level 1 <= 5.038562, level 2 evaluates
    # 5.004400 and then has its root at 5.043852, outside by 4.7e-4: no sign change in the bracket at level 2, iteration 2
    "curve_table": 5.0415,
    # the same behind polyline sections: stages of levels 1 - 8 <= 2.358436, level 9 evaluates 2.365983 (inside by 1.3e-3) and then has
    # its root at 2.371894, outside by 1.2e-3: level 9, iteration 2
    "curve_polyline": 2.369,
}


def storage_case(name):
    """dict(good, bad: problems; mode; entry: the dispatch-table entry to force (None: the library's own choice); env)"""
    R = A.SEC_RECT_UNIFORM
    env, mode = {}, "rect_uniform"
    if name == "one_wave":
        entry = _plain("f64", R, 2, 1, 0, full=0)
        seed = next(e for e in TABLE if e["section_mode"] == R and case_for(e)[0].ds.storage is not None)      # the suite's ("flow", "storage") recipe
        good = prismatic_problem(seed, ("flow", "storage"), False, n_steps=5)
        good.tol = 1e-3
    elif name == "multi_wave":
        entry = _plain("f64", R, 16, 4, 0, full=0)
        good = closed_form_reservoir(entry)
    elif name == "pair_excluded":
        entry = None
        good = closed_form_reservoir(_plain("f64", R, 16, 4, 2 + A.BC_NORMAL_DEPTH, full=1))
    elif name == "team":
        entry = find_entry(dtype=A.F64, section_mode=R, team=1, boundary_class=1)
        good = closed_form_reservoir(entry)
    elif name == "long":
        entry = find_entry(dtype=A.F64, section_mode=R, long_reach=1)
        good = closed_form_reservoir(entry)
        env = {"FS_NO_TEAM": "1"}
    elif name == "curve_table":
        entry = find_entry(dtype=A.F64, section_mode=A.SEC_TABLE, boundary_class=-1, long_reach=0, cells_per_thread=2)
        good, mode, _ = case_for(entry)
    elif name == "curve_polyline":
        entry = find_entry(dtype=A.F64, section_mode=A.SEC_IRREGULAR, boundary_class=-1, long_reach=0, cells_per_thread=2)
        good, mode, _ = case_for(entry)
    else:
        raise KeyError(name)
    bad = copy.deepcopy(good)
    bad.ds.storage["Y_max"] = STORAGE_Y_MAX[name]
    return dict(name=name, good=good, bad=bad, mode=mode, entry=entry, env=env)


STORAGE_CASES = tuple(STORAGE_Y_MAX)
