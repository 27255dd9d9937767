"""What the step kernels return when a reach does NOT converge: FS_NAN, FS_MAX_ITER and FS_STORAGE_RANGE on every instantiation
they can be reached on, against the CPU oracle (status, failing level, the iteration count of that level, every row before it),
and what include/flowsim_abi.h promises about a failed reach: the status sticks, later launches leave the reach alone, the state
is that of the end of the previous call, a restart begins from FS_OK again, and the other reaches of the batch are not touched.

The failures are made by data alone (tests/failure_recipes.py; tests/test_failure_recipes.py checks on the CPU that each recipe
fails at the level and iteration it is meant to, by a margin): none of them is a device fault."""
import copy
import os

import numpy as np
import pytest

import case_builders as CB
from conftest import GOLDEN
from entry_recipes import TABLE
import failure_recipes as FR
from fixture_batch import boundary_spec, merge_specs
from flowsim_amd import _abi as A
from kernel_harness import TOL, TOL_F32, assert_same_bits, batch_for_entry, entry_id, rel_err, snapshot
from oracle import preissmann_oracle as O

pytestmark = pytest.mark.gpu
K = FR.K_STAR
CASES = [(e, x) for e in TABLE for x in ("nan", "maxiter")]


def _restore(b, good):
    """the unedited boundaries and a generous iteration cap"""
    b.set_scheme(good.theta, good.dt, good.dx, good.tol, 100)
    b.set_boundary(A.UPSTREAM, merge_specs([boundary_spec(good.us, good.nt)], 1))
    b.set_boundary(A.DOWNSTREAM, merge_specs([boundary_spec(good.ds, good.nt)], 1))


# ---------------------------------------------------------------------------------------------------------------------------
# 2. every instantiation, two exits
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e,exit_", CASES, ids=[f"{entry_id(e)}-{x}" for e, x in CASES])
def test_failure_exit_of_an_instantiation(e, exit_, monkeypatch):
    good, bad, mode, override = FR.case(e, exit_)
    f32, nt = FR.f32_of(e), good.nt
    n1 = nt - 2                        # levels of the first launch: the failing level is not its last, and one more step fits the batch
    assert K < n1
    ref = FR.oracle_run(bad)
    assert ref["status"] == FR.STATUS[exit_] and ref["fail_level"] == K
    monkeypatch.setenv("FS_KERNEL_INDEX", str(e["index"]))
    storage = good.ds.storage is not None

    with batch_for_entry([good], e, mode, override) as b:               # the same entry without the failure
        b.step(nt - 1)
        assert b.kernel_index() == e["index"] and np.all(b.status() == 0), b.status()
        clean = snapshot(b, nt)

    with batch_for_entry([bad], e, mode, override) as b:                # one launch over the failing level
        initial = b.state()
        stage0 = b.storage_stage() if storage else None
        b.step(n1)
        assert b.kernel_index() == e["index"]
        one = snapshot(b, nt, K - 1)
        if storage:                                            # the stage that belongs to that state, not the last accepted level's
            assert np.array_equal(b.storage_stage(), stage0)
        failed_guess = b.guess()
        b.step(1)                                              # a later launch leaves the reach alone
        assert_same_bits(one, snapshot(b, nt, K - 1))
        assert b.level == n1 + 1

    with batch_for_entry([bad], e, mode, override) as b:                # the same run, split ahead of the failing level
        b.step(K - 1)
        before = b.state()
        guess = b.guess()
        stage = b.storage_stage() if storage else None
        b.step(n1 - (K - 1))
        split = snapshot(b, nt, K - 1)
        if storage:
            assert np.array_equal(b.storage_stage(), stage) and stage[0] != 0
        b.step(1)
        assert_same_bits(split, snapshot(b, nt, K - 1))
        # restart ahead of the failing level, with the unedited target and a generous cap: FS_OK again, and the run completes
        _restore(b, good)
        b.restart(K - 1, *before, *guess, stage)
        assert np.all(b.status() == 0)
        b.step(nt - K)
        again = dict(status=b.status().copy(), iters=b.iterations(K, nt - K), hyd=b.hydrographs(K, nt - K), state=b.state())
        if b.history:
            again["hist"] = b.history_arrays(K, nt - K)

    # status and counts: the oracle's
    st, its = one["status"], one["iters"][:, 0]
    assert st[0] == ref["status"], (st, ref["status"])
    assert its[K] == ref["iters"][K], (its, ref["iters"])
    assert np.all(its[K + 1:] == 0)
    if not f32:
        assert np.array_equal(its[:K], ref["iters"][:K])
    else:
        assert np.all(its[1:K] > 0)
    # rows before the failing level: the oracle's, and bit for bit those of the run without the failure
    d, f, tol = ref["depth"], ref["flow"], TOL_F32 if f32 else TOL
    hyd = one["hyd"][:, :, 0]
    assert rel_err(hyd[:K, 0], d[:K, 0], 1e-3) <= tol and rel_err(hyd[:K, 2], d[:K, -1], 1e-3) <= tol
    assert rel_err(hyd[:K, 1], f[:K, 0], 1.0) <= tol and rel_err(hyd[:K, 3], f[:K, -1], 1.0) <= tol
    assert np.array_equal(one["hyd"][:K], clean["hyd"][:K]) and np.array_equal(one["iters"][:K], clean["iters"][:K])
    if "hist" in one:
        assert rel_err(one["hist"][0][:K, 0], d[:K], 1e-3) <= tol and rel_err(one["hist"][1][:K, 0], f[:K], 1.0) <= tol
        assert all(np.array_equal(x[:K], y[:K]) for x, y in zip(one["hist"], clean["hist"]))
    # one launch == split launches, except for the state: that of the end of the call before the failing one
    assert_same_bits(one, split, fields=("status", "iters", "hyd", "hist"))
    assert all(np.array_equal(x, y) for x, y in zip(one["state"], initial))
    assert all(np.array_equal(x, y) for x, y in zip(split["state"], before))
    if exit_ == "nan":                                         # the vector the failing level ended with: not a start vector
        assert np.any(np.isnan(failed_guess[0])) and np.any(np.isnan(failed_guess[1]))
    # the restart: complete, and from the failing level on the run without the failure (fp32: to its tolerance of the fp64 answer)
    assert np.all(again["status"] == 0)
    if not f32:
        assert np.array_equal(again["iters"], clean["iters"][K:]) and np.array_equal(again["hyd"], clean["hyd"][K:])
        assert all(np.array_equal(x, y) for x, y in zip(again["state"], clean["state"]))
        if "hist" in again:
            assert all(np.array_equal(x, y[K:]) for x, y in zip(again["hist"], clean["hist"]))
    else:
        assert rel_err(again["hyd"][:, 1], clean["hyd"][K:, 1], 1.0) <= TOL_F32 and rel_err(again["hyd"][:, 3], clean["hyd"][K:, 3], 1.0) <= TOL_F32


# ---------------------------------------------------------------------------------------------------------------------------
# 3. storage-range exits, one case per path
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FR.STORAGE_CASES)
def test_storage_range_exit(name, monkeypatch):
    c = FR.storage_case(name)
    bad, mode, e = c["bad"], c["mode"], c["entry"]
    ref = FR.oracle_run(bad)
    k = ref["fail_level"]
    assert ref["status"] == 3
    for key, v in c["env"].items():
        monkeypatch.setenv(key, v)
    nt = bad.nt
    if e is None:
        # the compiled flow / normal-depth pair kernels exist for this shape and must not take it: forced, the library refuses ...
        pair = FR._plain("f64", A.SEC_RECT_UNIFORM, 16, 4, 2 + A.BC_NORMAL_DEPTH, full=1)
        assert pair["boundary_class"] >= 2 and bad.N == 64 * pair["cells_per_thread"] * pair["waves_per_reach"]
        monkeypatch.setenv("FS_KERNEL_INDEX", str(pair["index"]))
        with batch_for_entry([bad], pair, mode) as b:
            with pytest.raises(A.FlowsimError, match="FS_KERNEL_INDEX"):
                b.step(1)
        monkeypatch.delenv("FS_KERNEL_INDEX")
        e = pair                         # (dtype and history of the batch below)
    else:
        monkeypatch.setenv("FS_KERNEL_INDEX", str(e["index"]))
    with batch_for_entry([bad], e, mode) as b:
        stage0 = b.storage_stage()
        b.step(nt - 2)
        chosen = TABLE[b.kernel_index()]
        got = snapshot(b, nt, k - 1)
        stages = b.storage_stages(0, nt)[:, 0]
        # the reservoir stage of a failed reach is that of the end of the previous call, like its state (one_wave, the general
        # reservoirs: levels were accepted in this launch before the failing one)
        assert np.array_equal(b.storage_stage(), stage0)
        b.step(1)
        assert_same_bits(got, snapshot(b, nt, k - 1))
    if c["entry"] is None:               # ... and left alone it picks a kernel of a general class
        assert chosen["boundary_class"] in (0, 1) and chosen["section_mode"] == A.SEC_RECT_UNIFORM, chosen
    else:
        assert chosen["index"] == e["index"]
    if name == "team":
        assert chosen.get("team") and bad.N > 4096
    if name == "long":
        assert chosen.get("long_reach")
    its = got["iters"][:, 0]
    assert got["status"][0] == 3
    assert np.array_equal(its[:k + 1], ref["iters"][:k + 1]) and np.all(its[k + 1:] == 0), (its, ref["iters"])
    d, f = ref["depth"], ref["flow"]
    hyd = got["hyd"][:, :, 0]
    assert rel_err(hyd[:k, 0], d[:k, 0], 1e-3) <= TOL and rel_err(hyd[:k, 2], d[:k, -1], 1e-3) <= TOL
    assert rel_err(hyd[:k, 1], f[:k, 0], 1.0) <= TOL and rel_err(hyd[:k, 3], f[:k, -1], 1.0) <= TOL
    if "hist" in got:
        assert rel_err(got["hist"][0][:k, 0], d[:k], 1e-3) <= TOL and rel_err(got["hist"][1][:k, 0], f[:k], 1.0) <= TOL
    want = np.asarray(ref["storage_stage"])[:k - 1]
    assert stages[0] == 0 and np.all(stages[k:] == 0)
    if k > 1:
        assert rel_err(stages[1:k], want, 1e-3) <= TOL


# ---------------------------------------------------------------------------------------------------------------------------
# 4. isolation: good, failing, good in one launch
# ---------------------------------------------------------------------------------------------------------------------------
def _family_entry(family):
    R, T, I = A.SEC_RECT_UNIFORM, A.SEC_TABLE, A.SEC_IRREGULAR
    if family == "one-wave":
        return FR._plain("f64", R, 2, 1, 0, full=0)
    if family == "multi-wave":
        return FR._plain("f64", R, 16, 4, 0, full=0)
    if family == "tail":
        return FR.find_entry(dtype=A.F64, section_mode=T, tail=0)
    if family == "team":
        return FR.find_entry(dtype=A.F64, section_mode=R, team=1, boundary_class=0)
    if family == "multi-pass":
        return FR.find_entry(dtype=A.F64, section_mode=R, long_reach=1)
    if family == "polyline":
        return FR._plain("f64", I, 2, 1, 0, full=0)
    if family == "fp32":
        return FR._plain("f32", R, 4, 1, 0, full=0)
    raise KeyError(family)


def _scaled(p, factor):
    """the same reach with another hydrograph (so that the two good reaches of a batch differ)"""
    side = FR.target_side(p)
    q = FR.edited(p, 0, float(getattr(p, side).target[0]))
    t = getattr(q, side).target
    t[1:] = t[0] + factor * (t[1:] - t[0])
    return q


# (max-iter needs an iteration cap per reach - the good reaches keep the default - which only the kernels of the general boundary
# classes read, include/flowsim_abi.h fs_batch_set_reach_tolerance; the tail form is compiled for one boundary pair.  The storage row is
# a boundary kind of the uniform section modes' general classes.)
ISOLATION = [(f, x) for f in ("one-wave", "multi-wave", "tail", "team", "multi-pass", "polyline", "fp32") for x in ("nan", "maxiter", "storage")
             if not (f == "tail" and x != "nan") and not (x == "storage" and f not in ("one-wave", "multi-wave", "team", "multi-pass"))]


@pytest.mark.parametrize("family,exit_", ISOLATION, ids=[f"{f}-{x}" for f, x in ISOLATION])
def test_a_failing_reach_leaves_its_neighbours_alone(family, exit_, monkeypatch):
    e = _family_entry(family)
    caps, own_ds = None, False
    if exit_ == "storage":
        c = FR.storage_case({"one-wave": "one_wave", "multi-wave": "multi_wave", "team": "team", "multi-pass": "long"}[family])
        good, bad, mode, override = c["good"], c["bad"], c["mode"], None
        e = c["entry"] if family != "team" else e              # (the team entry of class 0: the general pairs include the reservoir)
        for key, v in c["env"].items():
            monkeypatch.setenv(key, v)
        if good.N > 130:
            # the reservoir's first level does not converge on a long reach: the neighbours end in normal depth instead, the kinds
            # of the batch are per reach (fs_batch_set_bc_per_reach), and only the failing reach has the reservoir
            good = FR.prismatic_problem(c["entry"], ("flow", "normal"), False)
            own_ds = True
    else:
        good, bad, mode, override = FR.case(e, exit_)
        if exit_ == "maxiter":
            caps = [100, bad.max_iter, 100]
    other = _scaled(good, 1.1) if exit_ != "storage" or own_ds else good
    ref = FR.oracle_run(bad)
    k, nt = ref["fail_level"], good.nt
    monkeypatch.setenv("FS_KERNEL_INDEX", str(e["index"]))
    def batch(probs):
        if not own_ds:
            return batch_for_entry(probs, e, mode, override)
        plain = [copy.copy(p) for p in probs]
        for p in plain:
            p.ds = good.ds
        b = batch_for_entry(plain, e, mode, override)
        b.set_boundary_per_reach(A.DOWNSTREAM, [boundary_spec(p.ds, p.nt) for p in probs])
        return b

    with batch([good, other]) as b:
        if caps:
            b.set_reach_tolerance(None, [100, 100])
        b.step(nt - 1)
        assert b.kernel_index() == e["index"]
        alone = snapshot(b, nt)
    with batch([good, bad, other]) as b:
        if caps:
            b.set_reach_tolerance(None, caps)
        b.step(nt - 1)
        assert b.kernel_index() == e["index"]
        mixed = snapshot(b, nt)
    keep = [0, 2]
    assert mixed["status"][1] == ref["status"] == FR.STATUS[exit_]
    assert mixed["iters"][k, 1] == ref["iters"][k] and np.all(mixed["iters"][k + 1:, 1] == 0)
    assert np.array_equal(mixed["status"][keep], alone["status"])
    assert np.all(alone["status"] == 0) and np.all(alone["iters"][1:] > 0)
    assert np.array_equal(mixed["iters"][:, keep], alone["iters"])
    assert np.array_equal(mixed["hyd"][:, :, keep], alone["hyd"])
    assert all(np.array_equal(x[keep], y) for x, y in zip(mixed["state"], alone["state"]))
    if "hist" in mixed:
        assert all(np.array_equal(x[:, keep], y) for x, y in zip(mixed["hist"], alone["hist"]))


# ---------------------------------------------------------------------------------------------------------------------------
# 5. fs_batch_iterate closes a failed reach
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exit_", ["nan", "maxiter"])
def test_one_iteration_per_launch_closes_a_failed_reach(exit_, monkeypatch):
    """fs_batch_iterate on a TABLE batch with a failing reach among good ones: the open count reaches 0 at every level, the level
    advances, and every reach - the failed one included - ends as the fused loop (fs_batch_step through the same instantiation)
    leaves it, bit for bit"""
    e = FR.find_entry(dtype=A.F64, section_mode=A.SEC_TABLE, boundary_class=-1, long_reach=0, cells_per_thread=2)
    good, bad, mode, override = FR.maxiter_case(e) if exit_ == "maxiter" else FR.nan_case(FR._plain("f64", A.SEC_TABLE, 2, 1, 0, full=0))
    probs = [good, bad, _scaled(good, 1.1)]
    caps = [100, bad.max_iter, 100]
    nt = good.nt
    with batch_for_entry(probs, e, mode, override) as a, batch_for_entry(probs, e, mode, override) as b:
        for x in (a, b):
            x.set_reach_tolerance(None, caps)
        launches = 0
        while b.level < nt - 1:
            level = b.level
            n_open = b.iterate()
            launches += 1
            assert b.level == level + (1 if n_open == 0 else 0)
            assert launches <= 100 * nt, "the level never closed"
        monkeypatch.setenv("FS_KERNEL_INDEX", str(b.kernel_index()))
        a.step(nt - 1)
        assert a.kernel_index() == b.kernel_index()
        fused, opened = snapshot(a, nt, K - 1), snapshot(b, nt, K - 1)
        guesses = a.guess(), b.guess()
    assert fused["status"][1] == FR.STATUS[exit_] and fused["status"][0] == fused["status"][2] == 0
    assert_same_bits(fused, opened, fields=("status", "iters", "hyd"))
    keep = [0, 2]
    assert all(np.array_equal(x[keep], y[keep]) for x, y in zip(fused["state"], opened["state"]))
    assert all(np.array_equal(x[keep], y[keep]) for x, y in zip(*guesses))
    ref = FR.oracle_run(bad)
    assert opened["iters"][K, 1] == ref["iters"][K] and np.all(opened["iters"][K + 1:, 1] == 0)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the drop-in solver raises what the reference raises
# ---------------------------------------------------------------------------------------------------------------------------
EXAMPLE_Y_MAX = 23.4      # cases/example: the oracle's reservoir stage is <= 18.91 through level 3; level 4 evaluates 22.664, then 23.464 (outside by 2.7e-3)


def test_the_drop_in_solver_raises_the_reference_errors_for_nan_and_storage_range():
    """(the max-iter error: tests/test_gpu_dropin.py, test_non_convergence_raises_like_the_reference)"""
    # FS_NAN: the reference notices a NaN only with diagnos (preissmann.py:133-137); without it the norm test never passes
    # and the level runs into the iteration cap (:124-126)
    for diagnos, message in ((False, "Convergence within 7 iterations couldn't be achieved."), (True, "NaN in system assembly")):
        solver, tol = CB.akbari()
        hyd = solver.channel.upstream_boundary.hydrograph
        inflow, dt = hyd.used_function, solver.time_step
        hyd.set_function(lambda t: float("nan") if abs(t - 2 * dt) < 0.5 * dt else inflow(t))
        with pytest.raises(ValueError, match=message):
            solver.run(tolerance=tol, verbose=0, max_iter=7, diagnos=diagnos)
        assert solver.time_level == 2
    # FS_STORAGE_RANGE: brentq's ValueError (lumped_storage.py:24-35)
    fx, meta = O.load_fixture(os.path.join(GOLDEN, "example.npz"))
    p = O.problem_from_fixture(fx, meta)
    p.ds.storage["Y_max"] = EXAMPLE_Y_MAX
    ref = O.newton_run(p)
    assert ref["status"] == 3 and ref["fail_level"] == 4 and ref["iters"][4] == 2
    solver, tol = CB.example()
    solver.channel.downstream_boundary.lumped_storage.Y_max = EXAMPLE_Y_MAX
    with pytest.raises(ValueError, match=r"f\(a\) and f\(b\) must have different signs"):
        solver.run(tolerance=tol, verbose=0)
    assert solver.time_level == 4 and np.array_equal(solver.iterations[:5], ref["iters"][:5])
