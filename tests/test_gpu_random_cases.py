"""Seeded random sweep: prismatic reaches drawn far outside the benchmark's parameter boxes - node counts 2 ... 700
(every lane / wave layout, ragged tails), theta 0.55 ... 1, time steps 30 s ... 1 h, spatial steps 25 m ... 2 km (Courant
numbers 0.3 ... 300), slopes 5e-5 ... 5e-3, widths 3 ... 600 m, Manning 0.012 ... 0.08, rectangles and trapezoids, every
pair of closed-form boundary kinds, flood waves of 10 % ... 300 % of the base flow - against the C oracle (pivoted banded
LU, the reference's algorithm).  fp64: 1e-8 relative on the whole history, identical Newton counts; the draw is part of
the test (seeded), a draw the ORACLE cannot solve is skipped and counted.

Supercritical draws are part of the sweep: there the Newton systems can be ill-conditioned (cond 1e13 ... 1e16: one boundary
condition per end is not what such a flow takes) and any two solvers part by 1e-6 ... 1e-2 - the reference and its own
restatements included (tests/test_near_critical.py pins that against the reference itself).  The rule for every draw is
therefore: 1e-8 with identical Newton counts, OR the kernel says so - status FS_ILL_CONDITIONED, raised by the conditioning
monitor of its elimination (include/flowsim_abi.h).  A last test keeps the monitor honest: it may flag only a small share
of the draws, and none of the clearly subcritical ones."""
import os

import numpy as np
import pytest

from fixture_batch import batch_from_problems
from flowsim_amd import _abi as A
from kernel_harness import rel_err
from oracle import c_oracle as CO
from random_cases import random_problem, random_table_problem, tidal_problem

pytestmark = pytest.mark.gpu
TOL = 1e-8
N_CASES = int(os.environ.get("FS_SWEEP_CASES", 384))          # a soak run: FS_SWEEP_CASES=8000 FS_SWEEP_TABLE=3000 pytest ...

_solved = []
_solved_table = []
_flagged = []          # (sweep, seed, Froude number or None, error) of every draw the conditioning monitor flagged
_unflagged_froude = []
ILL = 4                # FS_ILL_CONDITIONED
FLAGGED_TOL = 1e-2     # a flagged draw may miss 1e-8, not the flood wave (tests/test_near_critical.py: the same bound against the reference)
N_TABLE = int(os.environ.get("FS_SWEEP_TABLE", 128))


@pytest.mark.parametrize("seed", range(N_TABLE))
def test_random_compound_channel_against_the_oracle(seed):
    p, info = random_table_problem(seed)
    ref = CO.run(p)
    if ref["status"] != 0 or not np.all(np.isfinite(ref["depth"])) or np.min(ref["depth"]) <= 1e-3 * info["hn"]:
        _solved_table.append(False)
        pytest.skip(f"the oracle does not get through this draw (status {ref['status']}): {info}")
    _solved_table.append(True)
    with batch_from_problems([p], mode="table", history=True) as b:
        b.step(p.nt - 1)
        st = int(b.status()[0])
        assert st in (0, ILL), (st, info)
        h, Q = b.history_arrays(0, p.nt)
        its = b.iterations(0, p.nt)[:, 0]
    d, f = ref["depth"], ref["flow"]
    eh, eq = rel_err(h[:, 0], d, 1e-3 * info["hn"]), rel_err(Q[:, 0], f, 1e-3 * info["Qb"])
    if st == ILL:
        # flagged is not a free pass: the kernel says 1e-8 is not promised, the flood wave must still be the same one (the bound
        # tests/test_near_critical.py holds flagged reaches to against the reference itself)
        _flagged.append(("table", seed, None, max(eh, eq)))
        assert eh <= FLAGGED_TOL and eq <= FLAGGED_TOL, ("flagged draw off by more than 1e-2", eh, eq, info)
    else:
        assert eh <= TOL and eq <= TOL, (eh, eq, info)
        assert np.array_equal(its, ref["iters"]), (its, ref["iters"], info)
    over = np.any(d > p.geo["h_bf"][None, :]) and np.any(d < p.geo["h_bf"][None, :])
    info["both_sides_of_bankfull"] = bool(over)


@pytest.mark.parametrize("seed", range(N_CASES))
def test_random_reach_against_the_oracle(seed):
    p, info = random_problem(seed)
    ref = CO.run(p)
    if ref["status"] != 0 or not np.all(np.isfinite(ref["depth"])) or np.min(ref["depth"]) <= 1e-3 * info["hn"]:
        _solved.append(False)
        pytest.skip(f"the oracle does not get through this draw (status {ref['status']}): {info}")
    _solved.append(True)
    mode = "rect_uniform" if (not info["trapezoid"] and info["ds"] != "blend") else ("trap_uniform" if info["trapezoid"] and seed % 2 else "table")
    with batch_from_problems([p], mode=mode, history=True) as b:
        b.step(p.nt - 1)
        st = int(b.status()[0])
        assert st in (0, ILL), (st, info)
        h, Q = b.history_arrays(0, p.nt)
        its = b.iterations(0, p.nt)[:, 0]
    d, f = ref["depth"], ref["flow"]
    eh, eq = rel_err(h[:, 0], d, 1e-3 * info["hn"]), rel_err(Q[:, 0], f, 1e-3 * info["Qb"])
    if st == ILL:
        # the kernel itself says that this reach is beyond what its unpivoted elimination (or any solver, at 1e-8) stands for
        _flagged.append(("prismatic", seed, info["froude"], max(eh, eq)))
        assert eh <= FLAGGED_TOL and eq <= FLAGGED_TOL, ("flagged draw off by more than 1e-2", eh, eq, info)
        return
    _unflagged_froude.append(info["froude"])
    assert eh <= TOL and eq <= TOL, (eh, eq, info)
    assert np.array_equal(its, ref["iters"]), (its, ref["iters"], info)


N_LONG = int(os.environ.get("FS_SWEEP_LONG", 20))
_long_kernels = []


@pytest.mark.parametrize("seed", range(N_LONG))
def test_random_long_reach_against_the_oracle(seed, monkeypatch):
    """The same draws on reaches LONGER than one lane grid (4 097 ... 32 768 nodes: Courant numbers, slopes, boundary pairs and flood
    waves as above), on both kernels that take them: the team of workgroups (uniform sections; fs_kernel.hpp, TEAM) and the
    multi-pass kernel (FS_NO_TEAM=1, and the table mode; fs_long.hpp).  Node counts on and off the lane-grid multiples - a last
    member with one row, a full team, a ragged tail."""
    rng = np.random.default_rng(660000 + seed)
    special = (4097, 8192, 8193, 12288, 16384, 16385, 32768, 32767)
    N = special[seed] if seed < len(special) else int(rng.integers(4098, 24000))
    p, info = random_problem(5000 + seed, nodes=N)
    ref = CO.run(p)
    if ref["status"] != 0 or not np.all(np.isfinite(ref["depth"])) or np.min(ref["depth"]) <= 1e-3 * info["hn"]:
        pytest.skip(f"the oracle does not get through this draw (status {ref['status']}): {info}")
    d, f = ref["depth"], ref["flow"]
    uniform = "trap_uniform" if info["trapezoid"] else "rect_uniform"
    runs = [(uniform, False), (uniform, True)] if info["ds"] != "blend" else []
    if N <= 16384:
        runs.append(("table", False))
    for mode, no_team in runs:
        if no_team:
            monkeypatch.setenv("FS_NO_TEAM", "1")
        else:
            monkeypatch.delenv("FS_NO_TEAM", raising=False)
        with batch_from_problems([p], mode=mode, history=True) as b:
            b.step(p.nt - 1)
            st = int(b.status()[0])
            e = A.kernel_table()[b.kernel_index()]
            assert st in (0, ILL), (st, mode, no_team, info)
            assert (e["team"], e["long_reach"]) == ((1, 0) if (mode != "table" and not no_team) else (0, 1)), (e, mode, no_team)
            _long_kernels.append((e["team"], e["long_reach"]))
            h, Q = b.history_arrays(0, p.nt)
            its = b.iterations(0, p.nt)[:, 0]
        eh, eq = rel_err(h[:, 0], d, 1e-3 * info["hn"]), rel_err(Q[:, 0], f, 1e-3 * info["Qb"])
        if st == ILL:
            assert eh <= FLAGGED_TOL and eq <= FLAGGED_TOL, ("flagged draw off by more than 1e-2", eh, eq, mode, no_team, info)
            continue
        assert eh <= TOL and eq <= TOL, (eh, eq, mode, no_team, info)
        assert np.array_equal(its, ref["iters"]), (its, ref["iters"], mode, no_team, info)


def test_the_monitor_flags_few_draws_and_no_subcritical_prismatic_one():
    if len(_solved) < N_CASES or len(_solved_table) < N_TABLE:
        pytest.skip("runs after the sweeps")
    prism = [f for f in _flagged if f[0] == "prismatic"]
    assert all(fr >= 0.85 for _, _, fr, _ in prism), prism            # a flag on a prismatic reach means supercritical (or nearly) flow
    assert len(prism) <= 0.02 * N_CASES + 2 and len(_flagged) - len(prism) <= 0.03 * N_TABLE + 2, _flagged
    assert sum(fr >= 0.9 for fr in _unflagged_froude) >= 1 or N_CASES < 300        # supercritical draws that pass at 1e-8 unflagged exist too
    # what the flagged draws deviate by (each was held to FLAGGED_TOL above): printed with -s / in the captured output of a failure
    for sweep, seed, fr, err in sorted(_flagged, key=lambda f: -f[3]):
        print(f"flagged: {sweep} seed {seed} Froude {fr if fr is None else round(fr, 3)} deviation from the pivoted oracle {err:.3e}")
    assert all(err <= FLAGGED_TOL for *_, err in _flagged)


_reversed = []


@pytest.mark.parametrize("seed", range(24))
def test_flow_reversal_against_the_oracle(seed):
    p, info = tidal_problem(seed)
    ref = CO.run(p)
    if ref["status"] != 0:
        pytest.skip(f"the oracle does not get through this draw: {info}")
    _reversed.append(bool(np.min(ref["flow"]) < -0.05 * info["Qb"]))
    for mode in (("trap_uniform",) if info["trapezoid"] else ("rect_uniform", "table")):
        with batch_from_problems([p], mode=mode, history=True) as b:
            b.step(p.nt - 1)
            assert np.all(b.status() == 0), (b.status(), info)
            h, Q = b.history_arrays(0, p.nt)
            its = b.iterations(0, p.nt)[:, 0]
        assert rel_err(h[:, 0], ref["depth"], 1e-3 * info["hn"]) <= TOL and rel_err(Q[:, 0], ref["flow"], 1e-3 * info["Qb"]) <= TOL, info
        assert np.array_equal(its, ref["iters"]), info


def test_the_tide_does_reverse_the_flow():
    if len(_reversed) < 12:
        pytest.skip("runs after the tidal cases")
    assert sum(_reversed) >= len(_reversed) // 2, _reversed


def test_most_draws_are_solvable():
    """the sweep means something only if the reference's algorithm itself gets through most of it"""
    if len(_solved) < N_CASES or len(_solved_table) < N_TABLE:
        pytest.skip("runs after the sweeps")
    assert sum(_solved) >= 0.8 * N_CASES, f"{sum(_solved)} of {N_CASES}"
    assert sum(_solved_table) >= 0.7 * N_TABLE, f"{sum(_solved_table)} of {N_TABLE}"
