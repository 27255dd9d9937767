"""Every step kernel's Newton ITERATES against the oracle's, not only its fixed point.

Newton's method corrects its own Jacobian: a derivative that is off by 1e-3 leaves the converged rows where they were (5e-9 .. 1e-10
on the CPU oracle) and the iteration counts unchanged, and that is all the rest of the suite compares.  With max_iter = m a level
ends in FS_MAX_ITER after exactly m updates and fs_batch_get_guess holds the m-th iterate (include/flowsim_abi.h), which the numpy
oracle returns as x_next (newton_run(max_iter_at=...)).  x1 = x0 - J^-1 R(x0) sees what the fixed point hides: on the recipes of
tests/iterate_recipes.py each of T, dSe/dA, dSe/dQ and the boundary rows' df/dh, df/dQ, scaled by 1 + 1e-4, moves x1 by at least
6.8e-7 (68 times the fp64 bar), while rounding noise of 4 * 2^-52 on the reference's residual and Jacobian moves it by at most
4.8e-13 (tests/test_iterate_recipes.py asserts 50 times and 1e-12 for every entry, on the oracle alone).

For every entry of the dispatch table, three reaches of one channel that start off the fixed point at every node:
  a. level 1 capped at m = 1, 2 updates: status, count, guess() against the oracle on every node, state() untouched;
  b. level 1 converged, level 2 capped at one update: the level whose old state differs from its start vector;
  c. (fp64 entries that keep diagnostics) the residual norm of every iteration of two levels, at tests/test_gpu_dropin.py's bar;
  d. fs_batch_iterate (one launch per iteration) on a TABLE, a polyline and a ragged per-reach batch against the same vectors.
Bars: fp64 1e-8 (floors 1e-3 m, 1 m3/s), fp32 5e-4 of the fp64 oracle run from the float32-rounded start - the suite's own.

Measured on an MI355X (worst of depth / flow over the three iterates and three reaches of every entry of the family; nothing is
tightened to these):
  fp64  rect      one-grid 9.5e-14, no-diag 8.9e-14, team 2.6e-13, multi-pass 1.0e-13
        trap      one-grid 3.4e-14, no-diag 7.6e-15, team 5.2e-13, multi-pass 1.7e-13
        table     one-grid 3.8e-12, no-diag 3.8e-12, tail 3.8e-12 (the GERD fixture's flows; depth 1.5e-14), multi-pass 4.9e-14,
                  per-reach (fs_batch_iterate) 6.0e-14
        polyline  one-grid 6.8e-11, no-diag 4.0e-11, multi-pass 6.8e-11
        residual norms: at most 1.7 % of tests/test_gpu_dropin.py's allowance (rtol 1e-6, atol 1e-9 first + 1e-12)
  fp32  rect      one-grid 1.3e-4, multi-pass 5.0e-7        trap  one-grid 1.3e-4, no-diag 4.3e-7, multi-pass 3.8e-5
        table     one-grid 1.4e-4, multi-pass 5.3e-6
against 4.8e-13, the most that rounding noise on the reference's own residual and Jacobian moves its x1 (above).
"""
import functools

import numpy as np
import pytest

from entry_recipes import TABLE, fixture_problem
import failure_recipes as FR
from fixture_batch import hetero_batch_from_problems
from flowsim_amd import _abi as A
import iterate_recipes as IR
from kernel_harness import TOL, TOL_F32, batch_for_entry, capacity, entry_id, entry_of, rel_err
from oracle import preissmann_oracle as O

pytestmark = pytest.mark.gpu
FS_MAX_ITER = 1
IDS = [entry_id(e) for e in TABLE]


def family(e):
    sec = ("rect", "trap", "table", "polyline")[e["section_mode"]]
    form = "team" if e.get("team") else "multi-pass" if e.get("long_reach") else "tail" if e.get("tail", -1) >= 0 else "one-grid"
    return f"{'fp64' if e['dtype'] == 0 else 'fp32'} {sec} {form}{'' if e['diag'] else ' no-diag'}"


def _batch(probs, e, mode, override, **kw):
    assert probs[0].N <= capacity(e), "recipe does not fit the entry"
    if override is not None:
        override = np.broadcast_to(override, (len(probs),))
    return batch_for_entry(probs, e, mode, override, **kw)


def _compare(e, what, guess, refs, key):
    """guess() of the batch against the oracle's x_next of every reach: prints the figures, returns the worst (depth, flow)"""
    worst = [0.0, 0.0]
    for r, ref in enumerate(refs):
        h, Q = IR.unknowns(ref[key])
        eh, eq = rel_err(guess[0][r], h, 1e-3), rel_err(guess[1][r], Q, 1.0)
        worst = [max(worst[0], eh), max(worst[1], eq)]
    print(f"ITERATE {entry_id(e)} | {family(e)} | {what} | depth {worst[0]:.3e} flow {worst[1]:.3e}")
    return worst


@pytest.mark.parametrize("e", TABLE, ids=IDS)
def test_level_1_iterates_against_the_oracle(e, monkeypatch):
    probs, mode, override = IR.iterate_case(e)
    refs = IR.references(e)
    p0 = probs[0]
    tol = TOL_F32 if IR.f32_of(e) else TOL
    monkeypatch.setenv("FS_KERNEL_INDEX", str(e["index"]))
    got = {}
    for m in (1, 2):
        with _batch(probs, e, mode, override) as b:
            b.set_scheme(p0.theta, p0.dt, p0.dx, IR.ITER_TOL, m)
            initial = b.state()
            b.step(1)
            assert b.kernel_index() == e["index"]
            got[m] = dict(status=b.status().copy(), its=b.iterations(0, 2), guess=b.guess(), state=b.state(), initial=initial)
    worst = [_compare(e, f"level 1, m = {m}", got[m]["guess"], refs, (1, m)) for m in (1, 2)]
    for m in (1, 2):
        g = got[m]
        assert np.all(g["status"] == FS_MAX_ITER), g["status"]
        assert np.all(g["its"][1] == m), g["its"]
        assert all(np.array_equal(x, y) for x, y in zip(g["state"], g["initial"]))         # bit for bit the initial state
        for r, p in enumerate(probs):                                                      # ... which is the recipe's
            assert np.array_equal(g["initial"][0][r], p.h0) and np.array_equal(g["initial"][1][r], p.Q0)
    for eh, eq in worst:
        assert eh <= tol and eq <= tol, (eh, eq)


@pytest.mark.parametrize("e", TABLE, ids=IDS)
def test_level_2_iterate_against_the_oracle(e, monkeypatch):
    probs, mode, override = IR.iterate_case(e)
    refs = IR.references(e)
    p0 = probs[0]
    f32 = IR.f32_of(e)
    tol, level_tol = (TOL_F32 if f32 else TOL), IR.level_tol(e, p0.N)
    monkeypatch.setenv("FS_KERNEL_INDEX", str(e["index"]))
    with _batch(probs, e, mode, override) as b:
        b.set_scheme(p0.theta, p0.dt, p0.dx, level_tol, 100)
        b.step(1)
        assert b.kernel_index() == e["index"]
        first = b.status().copy()
        b.set_scheme(p0.theta, p0.dt, p0.dx, level_tol, 1)
        b.step(1)
        assert b.kernel_index() == e["index"]
        status, its, guess = b.status().copy(), b.iterations(0, 3), b.guess()
    want = np.array([ref[(2, 1)]["iters"][1] for ref in refs])
    print(f"ITERATE {entry_id(e)} | {family(e)} | level-1 counts {its[1]} oracle {want}")
    eh, eq = _compare(e, "level 2, m = 1", guess, refs, (2, 1))
    assert np.all(first == 0), first
    assert np.all(status == FS_MAX_ITER), status
    assert np.all(its[2] == 1), its
    if not f32:
        assert np.array_equal(its[1], want)
    assert eh <= tol and eq <= tol, (eh, eq)


@functools.lru_cache(maxsize=None)
def _traced(index):
    probs, _, _ = IR.iterate_case(TABLE[index])
    return tuple(O.newton_run(IR.at_level_tol(p, IR.LEVEL_TOL), trace=True) for p in probs)


TRACED = [e for e in TABLE if e["diag"] and not IR.f32_of(e)]


@pytest.mark.parametrize("e", TRACED, ids=[entry_id(e) for e in TRACED])
def test_residual_trace_from_the_perturbed_start(e, monkeypatch):
    """two levels with the residual trace on: the norm of every Newton iteration against the oracle's"""
    probs, mode, override = IR.iterate_case(e)
    p0 = probs[0]
    monkeypatch.setenv("FS_KERNEL_INDEX", str(e["index"]))
    with _batch(probs, e, mode, override, history=True, trace=True) as b:
        b.set_scheme(p0.theta, p0.dt, p0.dx, IR.LEVEL_TOL, 100)
        b.step(2)
        assert b.kernel_index() == e["index"]
        status, its, trace = b.status().copy(), b.iterations(0, 3), b.residual_trace(0, 3)
    assert np.all(status == 0), status
    worst = 0.0
    for r, ref in enumerate(_traced(e["index"])):
        assert ref["status"] == 0
        assert np.array_equal(its[:, r], ref["iters"]), (r, its[:, r], ref["iters"])
        for k in (1, 2):
            want = np.array([err for lvl, err in ref["norms"] if lvl == k])[:A.TRACE_CAP]
            got = trace[k, :len(want), r]
            assert np.all(trace[k, len(want):, r] == 0)
            worst = max(worst, float(np.max(np.abs(got - want) / (1e-6 * want + 1e-9 * want[0] + 1e-12))))
    print(f"ITERATE {entry_id(e)} | {family(e)} | residual trace, counts {its[1:, 0]} | worst deviation {worst:.3e} of the allowance")
    for r, ref in enumerate(_traced(e["index"])):
        for k in (1, 2):
            want = np.array([err for lvl, err in ref["norms"] if lvl == k])[:A.TRACE_CAP]
            np.testing.assert_allclose(trace[k, :len(want), r], want, rtol=1e-6, atol=1e-9 * want[0] + 1e-12)


# ---- fs_batch_iterate: one launch per Newton iteration, the same vectors ----
def _iterate_entry(kind):
    if kind == "table":
        return FR.find_entry(dtype=A.F64, section_mode=A.SEC_TABLE, boundary_class=-1, long_reach=0, cells_per_thread=2)
    return FR._plain("f64", A.SEC_IRREGULAR, 2, 1, 0, full=0)


@pytest.mark.parametrize("kind", ["table", "polyline"])
def test_one_iteration_per_launch_gives_the_same_iterates(kind):
    e = _iterate_entry(kind)
    probs, mode, override = IR.iterate_case(e)
    refs = IR.references(e)
    worst = []
    for m in (1, 2):
        with _batch(probs, e, mode, override) as b:
            for _ in range(m):
                n_open = b.iterate()
                assert n_open == IR.B and b.level == 0
            chosen = entry_of(b)
            assert chosen["section_mode"] == e["section_mode"] and chosen["dtype"] == A.F64
            assert np.all(b.status() == 0)
            worst.append(_compare(e, f"fs_batch_iterate x {m}", b.guess(), refs, (1, m)))
    for eh, eq in worst:
        assert eh <= TOL and eq <= TOL, (eh, eq)


def test_one_iteration_per_launch_on_a_ragged_batch():
    """three channels of their own, 26 / 41 / 21 nodes, one batch (fs_batch_set_reach_nodes): each reach's iterates are the oracle's"""
    probs = [IR.perturbed(fixture_problem(name, 8), seed) for name, seed in zip(("bc_trap_poly", "bc_compound_normal", "storage_curve_closed"), IR.SEEDS)]
    assert len({p.N for p in probs}) == 3
    for m in (1, 2):
        refs = [O.newton_run(p, max_iter_at={1: m}) for p in probs]
        with hetero_batch_from_problems(probs, mode="table") as b:
            for _ in range(m):
                assert b.iterate() == len(probs) and b.level == 0
            h, Q = b.guess()
        for r, (p, ref) in enumerate(zip(probs, refs)):
            assert ref["status"] == 1 and ref["iters"][1] == m
            want_h, want_Q = IR.unknowns(ref)
            eh, eq = rel_err(h[r, :p.N], want_h, 1e-3), rel_err(Q[r, :p.N], want_Q, 1.0)
            print(f"ITERATE ragged reach {r} (N = {p.N}) | fp64 table per-reach | fs_batch_iterate x {m} | depth {eh:.3e} flow {eq:.3e}")
            assert eh <= TOL and eq <= TOL, (r, m, eh, eq)
