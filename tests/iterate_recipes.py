"""Data-only recipes that make the Newton ITERATES of every step kernel comparable with the oracle's - shared by
tests/test_iterate_recipes.py, which checks on the numpy oracle alone that every recipe moves, is sensitive to each Jacobian
ingredient and is stable to rounding, and tests/test_gpu_newton_iterates.py, which runs them on the device.

Why: Newton's method corrects its own Jacobian.  A derivative that is off by 1e-3 leaves the fixed point where it was (to 1e-8 ..
1e-10) and the iteration counts unchanged, so the converged rows and the counts - all the rest of the suite compares - cannot see
it.  The first iterate x1 = x0 - J^-1 R(x0) can: with max_iter = m a level ends in FS_MAX_ITER after exactly m updates and
fs_batch_get_guess holds x_m (include/flowsim_abi.h), which O.newton_run(max_iter_at={level: m}) returns as x_next.

The cases are those of tests/entry_recipes.py (case_for: the smallest reach that uses each dispatch-table entry's
structure), shortened to two levels, as B = 3 reaches of the same channel whose initial states are off the fixed point at EVERY
node, each reach with its own seed:
    h0 (1 + a_h sin(2 pi k_h x) + 0.2 a_h xi),   Q0 (1 + a_q cos(2 pi k_q x) + 0.2 a_q xi),   x = i / (N - 1), xi ~ N(0, 1)
(the suite's prismatic recipes start exactly at uniform flow: their interior rows have a zero right-hand side); the two end nodes
take fixed multiples of the amplitudes instead of the wave, see OFFSETS.

Compound and polyline fixtures: the offsets reach over bankfull and across vertices without further help.  gerd has nodes on both
sides of bankfull at x0 and nodes that change sides between the reaches of a launch or between x0 and x1; bc_compound_normal is over
bank at every node throughout (1.20 .. 1.25 h_bf: the over-bank formulas, never the switch); in each polyline fixture (irr_levee,
irr_mixed, irr_single, irr_storage) the water levels of 4 .. 28 nodes straddle a vertex of their section.
tests/test_iterate_recipes.py asserts all three."""
import copy
import functools

import numpy as np

from entry_recipes import TABLE, case_for
from kernel_harness import entry_id, f32_of, rel_err  # noqa: F401
from oracle import preissmann_oracle as O

B = 3                                  # reaches of one launch
SEEDS = (11, 23, 37)
ITER_TOL = 1e-30                       # of the iterate runs: no level is accepted early
LEVEL_TOL = 1e-6                       # of the level that converges ahead of the level-2 iterate, and of the residual-trace runs
# The offsets by kind of channel: (a_h, a_q, k_h, k_q, end_h, end_q).
# end_h, end_q: the sine vanishes at both ends and the cosine is 1 there, which for the suite's inflow hydrograph happens to be its
# value at level 1 (1.146 Qb against a start of 1.15 Qb): the boundary rows would start from a residual of ~0 and a wrong derivative
# in them would not show (the oracle: a boundary derivative off by 1e-4 moved x1 by 1e-8 only).  The two end nodes therefore take
# these multiples of (a_h, a_q) in place of the wave, (first node, last node), raised per kind until every boundary derivative shows
# (tests/test_iterate_recipes.py).
# "reservoir": a general reservoir row (area curve, rated outflow, losses) behind a trapezoid table answers a raised end depth with
# flows of twice the base flow and more; one multiple of the offset at that end keeps the reference's rounding 1e4 below the bar.
# "deep": the GERD reservoir (depths to 49 m over sections kilometres wide, cond_1(J) = 1e9).  5 % of such a depth is a volume that
# the first update turns into flows of 20 times the base flow, through zero at some nodes, and the reference's own rounding then
# moves x1 by 3e-12; with 2 % and a lowered end depth (the gate curve downstream is steep above its initial stage) it is 4e-13.
OFFSETS = {"prismatic": (0.10, 0.15, 7, 5, (1.0, 2.0), (-1.0, 2.0)),
           "fixture": (0.05, 0.10, 3, 2, (1.0, 2.0), (-1.0, 2.0)),
           "reservoir": (0.05, 0.10, 3, 2, (1.0, 1.0), (-1.0, 1.0)),
           "deep": (0.02, 0.10, 3, 2, (1.0, -1.0), (-1.0, 1.0))}
# the iterates held to the oracle: (level, m)
ITERATES = ((1, 1), (1, 2), (2, 1))


def level_tol(e, N):
    """the tolerance a level converges at: fp32 cannot resolve ||R|| below ~6e-8 |Q| sqrt(2N) (tests/test_gpu_instantiations.py)"""
    if f32_of(e):
        return 1e-3 if N <= 600 else 2e-2
    return LEVEL_TOL


def is_prismatic(p):
    g = p.geo
    return "irr_npts" not in g and all(np.ptp(g[k]) <= 1e-12 * np.max(np.abs(g[k])) for k in ("b_main", "m_main", "n_main")) and not np.any(g["is_compound"] > 0.5)


def offsets_of(p):
    st = p.ds.storage
    if st is not None and any(st.get(k) is not None for k in ("curve", "rc", "losses")) and "irr_npts" not in p.geo:
        return "reservoir"
    if is_prismatic(p):
        return "prismatic"
    return "deep" if np.max(p.h0) > 20.0 else "fixture"


def perturbed(p, seed, f32=False):
    """a copy of the problem, two levels long, whose initial state is off the fixed point at every node (fp32 entries: rounded to
    float32, the start the device holds)"""
    q = copy.deepcopy(p)
    a_h, a_q, k_h, k_q, end_h, end_q = OFFSETS[offsets_of(p)]
    rng = np.random.default_rng(seed)
    x = np.arange(p.N) / (p.N - 1)
    wave_h, wave_q = np.sin(2 * np.pi * k_h * x), np.cos(2 * np.pi * k_q * x)
    wave_h[[0, -1]], wave_q[[0, -1]] = end_h, end_q
    q.h0 = p.h0 * (1 + a_h * wave_h + 0.2 * a_h * rng.standard_normal(p.N))
    q.Q0 = p.Q0 * (1 + a_q * wave_q + 0.2 * a_q * rng.standard_normal(p.N))
    if f32:
        q.h0 = q.h0.astype(np.float32).astype(np.float64)
        q.Q0 = q.Q0.astype(np.float32).astype(np.float64)
    q.nt = 3
    q.max_iter = 100
    q.tol = ITER_TOL
    return q


def iterate_case(e):
    """(problems[B], section mode of the batch, n_main override) for a dispatch-table entry"""
    p, mode, override = case_for(e)
    assert p.nt >= 3
    return [perturbed(p, s, f32_of(e)) for s in SEEDS], mode, override


def at_level_tol(p, tol):
    q = copy.copy(p)
    q.tol = tol
    return q


def reference_iterate(p, level, m, tol=None):
    """the oracle's run that ends in status 1 at `level` after m updates; level 2 follows a level 1 converged at `tol`"""
    q = p if level == 1 else at_level_tol(p, tol)
    return O.newton_run(q, max_iter_at={level: m})


@functools.lru_cache(maxsize=None)
def _references(index):
    e = TABLE[index]
    probs, _, _ = iterate_case(e)
    return tuple({(lvl, m): reference_iterate(p, lvl, m, level_tol(e, p.N)) for lvl, m in ITERATES} for p in probs)


def references(e):
    """per reach: {(level, m): oracle run}; computed once per entry, shared and left unchanged"""
    return _references(e["index"])


def unknowns(ref):
    """(h, Q) of the oracle's x_next"""
    x = ref["x_next"]
    return x[0::2], x[1::2]
