"""Near-critical and supercritical reaches, pinned to the reference itself (oracle/gen_random_sweep.py --near-critical 24 ->
tests/golden/near_critical.npz): 24 steep, smooth rectangular / trapezoidal / compound reaches of 65 ... 513 nodes whose
flow runs at Froude numbers 0.9 ... 1.5 (one boundary condition per end, as the reference always imposes), half of them
the worst-conditioned of 96 draws.  The fixture keeps, next to the reference's depth / flow histories and Newton counts, the
1-norm condition number of the reference's own Jacobian (first iteration of every level): 4e4 ... 8e16.

What the data says (and these tests assert):
  * up to cond 1e11 everything that restates the reference's algorithm - the numpy oracle (the same SuperLU call), the C
    oracle (its own pivoted banded LU), the kernel (no pivoting) - reproduces it to 1e-8 with identical Newton counts;
  * beyond 1e12 - exactly where the reference's own `diagnos` switch would raise "Jacobian is ill-conditioned (rcond too
    small)", preissmann.py:139-144 - NOTHING does: the numpy oracle, which calls the very same solver and differs from
    the reference only in the rounding of the assembly, parts from it by up to 3e-3, the pivoted C oracle likewise.  The
    1e-8 bar cannot be held there by any implementation, pivoting or not;
  * the kernel knows: its conditioning monitor (FS_ILL_CONDITIONED, include/flowsim_abi.h) flags every case it misses by
    more than 1e-7, and none of the cases below cond 1e8.  It is a one-sided detector - it watches the growth of the
    upstream-travelling characteristic along the reach, which is how supercritical flow makes these systems
    ill-conditioned - not a condition estimate: one case beyond the reference's limit (cond 5e12) that it does not
    flag lands at 5e-8.
Rule for the kernel and for the case-script path: 1e-8 with identical Newton counts, or the status / warning is raised;
beyond the reference's own conditioning limit (cond > 1e12, where the reference's `diagnos` run refuses and where no
restatement holds 1e-8, see above) an unflagged case must still be within 1e-6."""
import os
import warnings

import numpy as np
import pytest

from conftest import GOLDEN
from fixture_batch import batch_from_problems, is_rect_uniform
from flowsim_amd import _abi as A
from kernel_harness import rel_err
from oracle import c_oracle as CO
from oracle import preissmann_oracle as O
from oracle.gen_random_sweep import build_from_recipe
from random_cases import random_problem

PATH = os.path.join(GOLDEN, "near_critical.npz")
CASES = list(O.sweep_cases(PATH))
TOL = 1e-8
ILL = 4                      # FS_ILL_CONDITIONED
COND_LIMIT = 1e12            # the reference's own threshold (rcond < 1e-12, preissmann.py:142)


def label(c):
    i, _, m = c
    return f"{i:02d}-{m['family']}-N{m['N']}-cond{m['cond1_max']:.0e}"


def deviation(depth, flow, fx, m):
    if depth.shape != fx["depth"].shape:
        return np.inf
    return max(rel_err(depth, fx["depth"], 1e-3 * m["h_n"]), rel_err(flow, fx["flow"], 1e-3 * m["Qb"]))


def test_the_fixture_is_what_it_says():
    conds = np.array([m["cond1_max"] for _, _, m in CASES])
    assert len(CASES) == 24 and np.sum(conds > COND_LIMIT) >= 10 and np.sum(conds < 1e8) >= 6
    assert {m["family"] for _, _, m in CASES} == {"rect", "trap", "compound"}
    assert {m["us_kind"] for _, _, m in CASES} == {"flow_hydrograph", "stage_hydrograph", "fixed_depth"}
    assert all(m["ic"] == "steady-state" and m["froude_max"] >= 0.9 for _, _, m in CASES)
    assert sum(m["froude_max"] > 1.0 for _, _, m in CASES) >= 16


@pytest.mark.parametrize("case", CASES, ids=[label(c) for c in CASES])
def test_oracles_reproduce_the_reference_up_to_its_own_conditioning_limit(case):
    _, fx, m = case
    p = O.problem_from_fixture(fx, m)
    for run in (O.newton_run, CO.run):
        r = run(p)
        assert r["status"] == 0
        dev = deviation(r["depth"], r["flow"], fx, m)
        if m["cond1_max"] <= 1e11:
            assert dev <= TOL and np.array_equal(r["iters"], fx["iters"]), (run.__module__, dev)
        else:
            assert dev <= 1e-2, (run.__module__, dev)          # same regime, same answer to plotting accuracy - not to 1e-8


def test_the_same_solver_call_cannot_hold_1e8_beyond_the_limit():
    """the point of the fixture: the numpy oracle calls scipy's spsolve exactly as the reference does"""
    worst = 0.0
    for _, fx, m in CASES:
        if m["cond1_max"] > COND_LIMIT:
            r = O.newton_run(O.problem_from_fixture(fx, m))
            worst = max(worst, deviation(r["depth"], r["flow"], fx, m))
    assert worst > 1e-5, worst


_seen = {}


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[label(c) for c in CASES])
def test_kernel_reproduces_the_reference_or_says_that_it_cannot(case):
    i, fx, m = case
    p = O.problem_from_fixture(fx, m)
    modes = ["table"] + (["rect_uniform"] if is_rect_uniform(p) else [])
    for mode in modes:
        with batch_from_problems([p], mode=mode, history=True) as b:
            b.step(p.nt - 1)
            st = int(b.status()[0])
            assert st in (0, ILL), (mode, st)
            h, Q = b.history_arrays(0, p.nt)
            its = b.iterations(0, p.nt)[:, 0]
        dev = deviation(h[:, 0], Q[:, 0], fx, m)
        _seen[(i, mode)] = (st, dev, m["cond1_max"])
        if st == 0:
            assert dev <= (TOL if m["cond1_max"] < COND_LIMIT else 1e-6), (mode, dev, m["cond1_max"])
            if dev <= TOL:
                assert np.array_equal(its, fx["iters"]), (mode, its, fx["iters"])
        else:
            assert dev <= 1e-2, (mode, dev)                    # flagged: still the same flood wave
        if m["cond1_max"] < 1e8:
            assert st == 0, (mode, "flagged a well-conditioned reach", m["cond1_max"])


@pytest.mark.gpu
def test_the_monitor_separates_the_fixture():
    if len(_seen) < len(CASES):
        pytest.skip("runs after the cases")
    flagged = [v for v in _seen.values() if v[0] == ILL]
    assert len(flagged) >= 10 and all(c >= 1e8 for _, _, c in flagged), flagged
    assert all(st == ILL for st, dev, _ in _seen.values() if dev > 1e-7)
    assert all(st == ILL or dev <= TOL for st, dev, c in _seen.values() if c < COND_LIMIT)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[label(c) for c in CASES])
def test_case_script_path_warns_or_raises_like_the_reference(case):
    """PreissmannSolver(...).run() of the mirror: results to 1e-8, or a RuntimeWarning (and `ill_conditioned`); with
    diagnos=True the reference's ValueError text (preissmann.py:144)"""
    _, fx, m = case
    solver, _, _ = build_from_recipe(m["recipe"])
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        solver.run(tolerance=m["tolerance"], verbose=0, max_iter=m["max_iter"])
    dev = deviation(solver.depth, solver.flow, fx, m)
    if solver.ill_conditioned:
        assert any(issubclass(x.category, RuntimeWarning) and "ill-conditioned" in str(x.message) for x in w)
        solver2, _, _ = build_from_recipe(m["recipe"])
        with pytest.raises(ValueError, match="Jacobian is ill-conditioned"):
            solver2.run(tolerance=m["tolerance"], verbose=0, max_iter=m["max_iter"], diagnos=True)
    else:
        assert dev <= (TOL if m["cond1_max"] < COND_LIMIT else 1e-6)
        if dev <= TOL:
            assert np.array_equal(solver.iterations, fx["iters"])


@pytest.mark.parametrize("case", CASES[::4], ids=[label(c) for c in CASES[::4]])
def test_mirror_sets_the_channel_up_as_the_reference_does(case):
    _, fx, m = case
    solver, hyd, extra = build_from_recipe(m["recipe"])
    assert type(solver).__module__.startswith("flowsim_amd")
    assert solver.number_of_nodes == m["N"] and solver.number_of_time_levels == m["nt"]
    for k in ("z_bed", "b_main", "m_main", "n_main", "is_compound", "h_bf"):
        np.testing.assert_allclose(solver.channel.node_geometry[k], fx["geo_" + k], rtol=1e-13, atol=1e-15, err_msg=k)
    np.testing.assert_allclose(solver.channel.initial_conditions, fx["initial_conditions"], rtol=1e-10, atol=1e-12)


@pytest.mark.gpu
def test_a_batch_without_history_watches_its_conditioning_by_default():
    """PreissmannBatch(monitor=True) is the default since round 4 (the reference's `diagnos` check is per run, preissmann.py:133-144): a
    batch that keeps neither history nor trace still runs the kernels that carry the conditioning monitor.  The four outliers of round 2's
    supercritical scan (profiles/round2/supercritical_scan.txt: seeds 5932, 6685, 6373, 5684 - Froude 1.08 ... 1.48, 1.5e-4 ... 8e-3 away from
    the pivoted oracle) come back flagged from such a batch.  (monitor=False - what bench.py asks for - selects the kernels compiled without
    diagnostics where the batch's shape has one.)"""
    for seed in (5932, 6685, 6373, 5684):
        p, info = random_problem(seed)
        mode = "rect_uniform" if (not info["trapezoid"] and info["ds"] != "blend") else "table"
        with batch_from_problems([p], mode=mode, history=False, monitor=True) as b:       # (the helper's default follows `history`; PreissmannBatch's is True)
            b.step(p.nt - 1)
            assert int(b.status()[0]) == ILL, (seed, b.status())
            assert A.kernel_table()[b.kernel_index()]["diag"] == 1
    from flowsim_amd import PreissmannBatch
    import inspect
    assert inspect.signature(PreissmannBatch.__init__).parameters["monitor"].default is True
