"""Every instantiation of the step kernel (csrc/fs_entry_list.hpp, exported as the dispatch table of the C ABI) is
launched once and checked against the CPU oracle: fp64 to 1e-8 with identical Newton counts, fp32 to 5e-4 of the
fp64 answer.

The case for an entry follows from its attributes (tests/entry_recipes.py; tables and polylines have a second one from the
reference's own random sweep).  FS_KERNEL_INDEX makes fs_batch_step use exactly that entry or fail; the test also
fails for an entry it has no recipe for - adding an instantiation without coverage is an error."""
import os

import numpy as np
import pytest

from entry_recipes import TABLE, case_for, oracle_run, second_case_for
from fixture_batch import batch_from_problems
from flowsim_amd import _abi as A
from kernel_harness import TOL, TOL_F32, batch_for_entry, capacity, entry_id, f32_of, rel_err
from synth import rect_problem

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("e", TABLE, ids=[entry_id(e) for e in TABLE])
def test_instantiation_against_the_oracle(e, monkeypatch):
    p, mode, override = case_for(e)
    f32 = f32_of(e)
    if f32:
        p.tol = 1e-3 if p.N <= 600 else 2e-2      # fp32 cannot resolve ||R|| below ~6e-8 |Q| sqrt(2N) (bench.py uses the same)
    assert p.N <= capacity(e), "recipe does not fit the entry"
    ref = oracle_run(p)
    assert ref["status"] == 0
    monkeypatch.setenv("FS_KERNEL_INDEX", str(e["index"]))
    history = bool(e["diag"])
    with batch_for_entry([p], e, mode, override) as b:
        b.step(p.nt - 1)
        assert b.kernel_index() == e["index"]
        assert np.all(b.status() == 0), b.status()
        hyd = b.hydrographs(0, p.nt)[:, :, 0]
        h, Q = b.state()
        its = b.iterations(0, p.nt)[:, 0]
        hist = b.history_arrays(0, p.nt) if history else None
    d, f = ref["depth"], ref["flow"]
    tol = TOL_F32 if f32 else TOL
    assert rel_err(hyd[:, 0], d[:, 0], 1e-3) <= tol and rel_err(hyd[:, 2], d[:, -1], 1e-3) <= tol
    assert rel_err(hyd[:, 1], f[:, 0], 1.0) <= tol and rel_err(hyd[:, 3], f[:, -1], 1.0) <= tol
    assert rel_err(h[0], d[-1], 1e-3) <= tol and rel_err(Q[0], f[-1], 1.0) <= tol
    if hist is not None:
        assert rel_err(hist[0][:, 0], d, 1e-3) <= tol and rel_err(hist[1][:, 0], f, 1.0) <= tol
    if not f32:
        assert np.array_equal(its, ref["iters"])


SECOND = [e for e in TABLE if e["section_mode"] in (2, 3)]


@pytest.mark.parametrize("e", SECOND, ids=[entry_id(e) for e in SECOND])
def test_table_and_polyline_instantiations_on_a_second_case(e, monkeypatch):
    p, mode, ref_fx = second_case_for(e)
    f32 = f32_of(e)
    if f32:
        p.tol = max(p.tol, 1e-3)
    if ref_fx is None:
        ref = oracle_run(p)
        assert ref["status"] == 0
        d, f, ref_its = ref["depth"], ref["flow"], ref["iters"]
        hfloor, qfloor = 1e-3, 1.0
    else:
        fx, m = ref_fx
        d, f, ref_its = fx["depth"], fx["flow"], fx["iters"]
        hfloor, qfloor = 1e-3 * m["h_n"], 1e-3 * m["Qb"]
        if f32:                    # fp32 on the reference's random channels: the deviation measured against the case's scales (base depth, base
            hfloor, qfloor = m["h_n"], m["Qb"]          # flow), 2e-2 of them - a miscompiled kernel misses by orders of magnitude or faults
    monkeypatch.setenv("FS_KERNEL_INDEX", str(e["index"]))
    history = bool(e["diag"])
    with batch_for_entry([p], e, mode) as b:
        b.step(p.nt - 1)
        assert b.kernel_index() == e["index"]
        assert np.all(b.status() == 0), b.status()
        hyd = b.hydrographs(0, p.nt)[:, :, 0]
        its = b.iterations(0, p.nt)[:, 0]
        hist = b.history_arrays(0, p.nt) if history else None
    tol = (2e-2 if ref_fx is not None else TOL_F32) if f32 else TOL      # (fp32 on a reference sweep case: the same flood wave, see above)
    assert rel_err(hyd[:, 0], d[:, 0], hfloor) <= tol and rel_err(hyd[:, 2], d[:, -1], hfloor) <= tol
    assert rel_err(hyd[:, 1], f[:, 0], qfloor) <= tol and rel_err(hyd[:, 3], f[:, -1], qfloor) <= tol
    if hist is not None:
        assert rel_err(hist[0][:, 0], d, hfloor) <= tol and rel_err(hist[1][:, 0], f, qfloor) <= tol
    if not f32:
        assert np.array_equal(its, ref_its)


def test_the_second_recipes_differ_from_the_first():
    assert len(SECOND) >= 30
    for e in SECOND:
        p1, _, _ = case_for(e)
        p2, _, _ = second_case_for(e)
        assert (p1.N, p1.dt, p1.ds.kind, p1.us.kind) != (p2.N, p2.dt, p2.ds.kind, p2.us.kind) or not np.array_equal(p1.geo["n_main"], p2.geo["n_main"]), entry_id(e)


def test_the_table_is_what_this_file_expects():
    """every entry has a recipe, the recipes between them reach every boundary kind on both ends, and the forced index
    is refused when it does not fit"""
    assert len(TABLE) == A.lib().fs_kernel_table_size() > 0
    seen = set()
    for e in TABLE:
        p, mode, _ = case_for(e)
        seen.add(("us", p.us.kind)); seen.add(("ds", p.ds.kind, p.ds.rc_type, p.ds.storage is not None))
    for kind in ("flow_hydrograph", "stage_hydrograph", "fixed_depth", "normal_depth", "rating_curve"):
        assert ("us", kind) in seen, kind
    for key in (("ds", "flow_hydrograph", None, False), ("ds", "stage_hydrograph", None, False), ("ds", "fixed_depth", None, False),
                ("ds", "fixed_depth", None, True), ("ds", "normal_depth", None, False), ("ds", "rating_curve", "power", False),
                ("ds", "rating_curve", "polynomial", False), ("ds", "rating_curve", "blend", False)):
        assert key in seen, key
    os.environ["FS_KERNEL_INDEX"] = "0"            # entry 0 is an fp64 rectangular (2,1) kernel: 128 nodes at most
    try:
        with batch_from_problems([rect_problem(200, seed=1, n_steps=2)], mode="rect_uniform") as b:
            with pytest.raises(A.FlowsimError, match="FS_KERNEL_INDEX"):
                b.step(1)
    finally:
        del os.environ["FS_KERNEL_INDEX"]
