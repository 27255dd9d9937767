"""The failure recipes of tests/failure_recipes.py, checked on the CPU oracle alone: every dispatch-table entry has a NaN and a
max-iter recipe that fail where they are meant to, with the margins that make the fp32 kernels' failing level and count the
oracle's without looking at a kernel; the storage-range recipes likewise; and the two oracles (numpy, C) report the same status,
level, iteration count and rows for all three exits.  tests/test_gpu_failure_exits.py runs the same recipes on the device."""
import warnings

import numpy as np
import pytest

import failure_recipes as FR
from oracle import c_oracle as CO
from oracle import preissmann_oracle as O

TABLE = FR.TABLE
IDS = [FR.entry_id(e) for e in TABLE]
PARITY = 1e-8          # the fp64 parity tolerance of the suite (storage margins are relative to it)


def _trace(p, n_steps):
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")          # (a diverging iterate divides by a vanishing area on the way: that is the point)
        return O.newton_run(p, n_steps=n_steps, trace=True)


def test_the_library_is_built_and_every_entry_is_covered():
    assert len(TABLE) > 100, "the dispatch table comes from the built library"
    for e in TABLE:
        for exit_ in ("nan", "maxiter"):
            good, bad, mode, _ = FR.case(e, exit_)            # raises for an entry without a recipe
            assert good.nt - 1 > FR.K_STAR >= 2, FR.entry_id(e)    # converged levels precede and would follow
    reasons = [FR.substituted(e) for e in TABLE]
    assert set(reasons) - {None} <= set(FR.SUBSTITUTED) and reasons.count(None) >= 70      # most entries run the suite's own case
    assert set(FR.STORAGE_CASES) == {"one_wave", "multi_wave", "pair_excluded", "team", "long", "curve_table", "curve_polyline"}


@pytest.mark.parametrize("e", TABLE, ids=IDS)
def test_nan_recipe(e):
    good, bad, mode, _ = FR.nan_case(e)
    k = FR.K_STAR
    ref = FR.oracle_run(bad)
    assert ref["status"] == FR.STATUS["nan"] and ref["fail_level"] == k
    assert ref["iters"][k] == 1 and np.all(ref["iters"][1:k] > 0) and np.all(ref["iters"][k + 1:] == 0)
    base = FR.oracle_run(FR._upto(good, k - 1))
    assert base["status"] == 0 and np.array_equal(base["iters"][:k], ref["iters"][:k])
    assert np.array_equal(base["depth"][:k], ref["depth"][:k])          # the edit is invisible before K_STAR


@pytest.mark.parametrize("e", TABLE, ids=IDS)
def test_max_iter_recipe(e):
    good, bad, mode, _ = FR.maxiter_case(e)
    k, tol = FR.K_STAR, good.tol
    assert bad.tol == tol
    base = _trace(good, k)
    assert base["status"] == 0
    assert bad.max_iter == int(max(base["iters"][1:k]))
    last = {}
    for lvl, err in base["norms"]:
        last[lvl] = err
    for lvl in range(1, k):
        print(f"{FR.entry_id(e)}: level {lvl} converged in {base['iters'][lvl]} iterations at ||R|| = {last[lvl] / tol:.1e} tol")
        assert last[lvl] < tol / FR.MARGIN, (lvl, last[lvl] / tol)
    ref = _trace(bad, k)
    at_k = [err for lvl, err in ref["norms"] if lvl == k]
    print(f"{FR.entry_id(e)}: level {k} after max_iter = {bad.max_iter} iterations ||R|| = {at_k[-1] / tol:.1e} tol")
    assert ref["status"] == FR.STATUS["maxiter"] and ref["fail_level"] == k and ref["iters"][k] == bad.max_iter == len(at_k)
    assert np.all(np.isfinite(at_k)) and at_k[-1] > FR.MARGIN * tol, at_k[-1] / tol
    fast = FR.oracle_run(bad)                       # the oracle the GPU test compares with (C where it applies)
    assert fast["status"] == 1 and fast["fail_level"] == k and np.array_equal(fast["iters"][:k + 1], ref["iters"][:k + 1])


@pytest.mark.parametrize("name", FR.STORAGE_CASES)
def test_storage_range_recipe(name):
    c = FR.storage_case(name)
    good, bad = c["good"], c["bad"]
    hi = bad.ds.storage["Y_max"]
    assert bad.ds.storage["Y_min"] == good.ds.storage["Y_min"] and hi < good.ds.storage["Y_max"]
    ref = _trace(bad, None)
    k = ref["fail_level"]
    assert ref["status"] == FR.STATUS["storage"]
    closed_form = not any(bad.ds.storage.get(x) is not None for x in ("curve", "rc", "losses"))
    assert (k >= 2 or (closed_form and good.N > 130 and k == 1)) and k < good.nt - 1
    count = int(ref["iters"][k])
    stages = ref["stage_trace"]
    assert stages[-1][:2] == (k, count) and len(stages) == int(ref["iters"][1:k + 1].sum())
    if closed_form:
        offending = stages[-1][2]
    else:                 # no bracket: the root the wide bracket finds at that iteration, from the same iterate
        wide = _trace(good, k)["stage_trace"]
        assert wide[len(stages) - 1][:2] == (k, count)
        offending = wide[len(stages) - 1][2]
    margin = FR.MARGIN * PARITY
    print(f"{name}: level {k}, iteration {count}: stage {offending:.6f} beyond Y_max = {hi} by {(offending - hi) / hi:.1e}; "
          f"stages before it inside by {min((hi - y) / hi for _, _, y in stages[:-1]):.1e}")
    assert (offending - hi) / hi > margin
    for lvl, it, y in stages[:-1]:
        assert (hi - y) / hi > margin and y > bad.ds.storage["Y_min"] * (1 + margin), (lvl, it, y)
    fast = FR.oracle_run(bad)
    assert fast["status"] == 3 and fast["fail_level"] == k and np.array_equal(fast["iters"][:k + 1], ref["iters"][:k + 1])


def _small_cases():
    e = FR._plain("f64", 0, 2, 1, 0, full=0)                   # 127 nodes, flow upstream, normal depth downstream
    yield "nan", FR.nan_case(e)[1]
    yield "maxiter", FR.maxiter_case(e)[1]
    yield "storage", FR.storage_case("one_wave")["bad"]
    yield "storage-level-1", FR.storage_case("multi_wave")["bad"]


@pytest.mark.parametrize("name,p", list(_small_cases()), ids=[n for n, _ in _small_cases()])
def test_the_two_oracles_agree_on_a_failure(name, p):
    """status, failing level, the iteration count of every level (the failing one included: the count include/flowsim_abi.h
    defines) and the rows before the failing level"""
    a, b = _trace(p, None), CO.run(p)
    k = a["fail_level"]
    assert a["status"] == b["status"] == FR.STATUS[name.split("-")[0]] and b["fail_level"] == k
    assert np.array_equal(a["iters"], b["iters"][:len(a["iters"])]) and np.all(b["iters"][k + 1:] == 0)
    assert np.max(np.abs(a["depth"][:k] - b["depth"][:k]) / np.abs(a["depth"][:k])) < 1e-9
    assert np.max(np.abs(a["flow"][:k] - b["flow"][:k]) / np.maximum(np.abs(a["flow"][:k]), 1.0)) < 1e-9
    if p.ds.storage is not None:
        assert np.allclose(a["storage_stage"], b["storage_stage"][:k - 1], rtol=1e-9, atol=0) and np.all(b["storage_stage"][k - 1:] == 0)
