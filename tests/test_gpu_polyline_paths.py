"""Every polyline ("irregular") instantiation of the step kernel on every node-evaluation path of fs_poly.hpp.

The channels of tests/poly_edges.py put stages exactly on, 5e-7 and 2e-6 from vertex elevations (the edge walk of
poly_eval_whole), mix walk and table lanes in one wave, cross from one to three wetted runs (the sub-channel walk), reach 245
stations (multi-round breakpoint scans) and run over every vertex (the unbounded top interval).  Each polyline entry of the
dispatch table is forced with FS_KERNEL_INDEX and compared with the CPU oracle (fp64: 1e-8, identical Newton counts), with
stage tables and again with FS_POLY_WALK=1 (no tables); the three reference-generated irr_* fixtures run on every entry over
all their levels; a per-reach batch of ~70 reaches must give each reach the bits of its own one-reach run wherever it sits in
the batch; and a launch of a different, large-LDS table kernel between two runs of a case must not change the second run."""
import copy
import os

import numpy as np
import pytest

from conftest import GOLDEN
from flowsim_amd import _abi as A
from oracle import preissmann_oracle as O

from fixture_batch import batch_from_problems, hetero_batch_from_problems, per_reach_polyline_batch
from kernel_harness import TOL, capacity, kernel_table, rel_err
import poly_edges as PE

pytestmark = pytest.mark.gpu


ENTRIES = [e for e in kernel_table() if e["section_mode"] == A.SEC_IRREGULAR]


def test_the_polyline_entries_are_there():
    """an empty table (library missing or not importable) must fail here, not collect every test below as a skip"""
    assert ENTRIES and len(ENTRIES) == sum(e["section_mode"] == A.SEC_IRREGULAR for e in A.kernel_table())


def _id(e):
    return (f"{e['index']:03d}-{e['cells_per_thread']}x{e['waves_per_reach']}-bc{e['boundary_class']}"
            f"{'' if e['diag'] else '-nodiag'}{'-long' if e.get('long_reach') else ''}")


def fits(e, p):
    """the case fits the entry's capacity and its boundary class (class 5: flow in, normal depth out, nothing else)"""
    if p.N > capacity(e):
        return False
    if e["boundary_class"] >= 2:
        return p.us.kind == "flow_hydrograph" and p.ds.kind == "normal_depth"
    return True


# the poly_edges cases of this file (kind, N, seed); the long entry's own case is longer than the 8x4 capacity (2048 rows)
CASES = PE.CENSUS + [("near_vertex_mixed", 120, 31), ("multi_run", 100, 32), ("overtopped_shallow", 500, 33)]
LONG_CASE = ("on_vertex", 2100, 40)
_cache = {}


def case(spec):
    """(Problem, oracle run), once per module"""
    if spec not in _cache:
        _cache[spec] = PE.make(*spec, **({"nt": 4} if spec == LONG_CASE else {}))
    return _cache[spec]


def fixture(name):
    if name not in _cache:
        fx, meta = O.load_fixture(os.path.join(GOLDEN, name + ".npz"))
        p = O.problem_from_fixture(fx, meta)
        _cache[name] = (p, O.newton_run(p))
    return _cache[name]


def run_entry(e, p, monkeypatch, history, walk=False):
    """(hydrographs, final state, iterations, history or None, poly_tables) of problem p on entry e"""
    monkeypatch.setenv("FS_KERNEL_INDEX", str(e["index"]))
    if walk:
        monkeypatch.setenv("FS_POLY_WALK", "1")
    else:
        monkeypatch.delenv("FS_POLY_WALK", raising=False)
    try:
        with batch_from_problems([p], mode="irregular", history=history) as b:
            b.step(p.nt - 1)
            assert b.kernel_index() == e["index"]
            assert np.all(b.status() == 0), b.status()
            out = (b.hydrographs(0, p.nt)[:, :, 0], b.state(), b.iterations(0, p.nt)[:, 0],
                   b.history_arrays(0, p.nt) if history else None, b.poly_tables())
    finally:
        monkeypatch.delenv("FS_KERNEL_INDEX", raising=False)
        monkeypatch.delenv("FS_POLY_WALK", raising=False)
    return out


def check_against_oracle(e, p, ref, got, what):
    hyd, (h, Q), its, hist, _ = got
    d, f = ref["depth"], ref["flow"]
    assert rel_err(hyd[:, 0], d[:, 0], 1e-3) <= TOL and rel_err(hyd[:, 2], d[:, -1], 1e-3) <= TOL, what
    assert rel_err(hyd[:, 1], f[:, 0], 1.0) <= TOL and rel_err(hyd[:, 3], f[:, -1], 1.0) <= TOL, what
    assert rel_err(h[0, :p.N], d[-1], 1e-3) <= TOL and rel_err(Q[0, :p.N], f[-1], 1.0) <= TOL, what
    if hist is not None:
        assert rel_err(hist[0][:, 0, :p.N], d, 1e-3) <= TOL and rel_err(hist[1][:, 0, :p.N], f, 1.0) <= TOL, what
    assert np.array_equal(its, ref["iters"]), (what, its, ref["iters"])


def specs_for(e):
    if e.get("long_reach"):
        return [LONG_CASE]
    return [s for s in CASES if fits(e, case(s)[0])]


@pytest.mark.parametrize("walk", [False, True], ids=["tables", "walk"])
@pytest.mark.parametrize("e", ENTRIES, ids=[_id(e) for e in ENTRIES])
def test_edge_cases_against_the_oracle(e, walk, monkeypatch):
    specs = specs_for(e)
    assert len(specs) >= (1 if e.get("long_reach") else 5), "too few cases fit the entry"
    for spec in specs:
        p, ref = case(spec)
        got = run_entry(e, p, monkeypatch, history=bool(e["diag"]), walk=walk)
        assert got[4] == (0 if walk else 1), "stage tables on / off as asked"
        check_against_oracle(e, p, ref, got, spec)


@pytest.mark.parametrize("e", ENTRIES, ids=[_id(e) for e in ENTRIES])
def test_every_fixture_on_every_entry(e, monkeypatch):
    """irr_levee, irr_mixed and irr_single over all their levels (one fixture per entry before: the record of irr_levee going
    wrong from level 6 on the (2, 1) no-diagnostics entry was never re-tested)"""
    ran = 0
    for name in ("irr_levee", "irr_mixed", "irr_single"):
        p, ref = fixture(name)
        assert ref["status"] == 0
        if not fits(e, p):
            continue
        got = run_entry(e, p, monkeypatch, history=bool(e["diag"]))
        check_against_oracle(e, p, ref, got, name)
        ran += 1
    assert ran >= 2


BATCH_KINDS = [("on_vertex", 24, 1), ("on_vertex_fixed", 24, 2), ("near_vertex_mixed", 64, 3), ("multi_run", 20, 4),
               ("overtopped_shallow", 24, 5), ("stations48", 16, 6), ("near_vertex_mixed", 40, 9), ("multi_run", 33, 10)]


def common(p, nt=3):
    """a copy on the scheme every reach of one batch shares (theta, dt, dx, tolerance are the batch's), with nt levels (a
    tolerance no Newton norm of the BATCH_KINDS channels comes within 1.25x of: tests/poly_edges.py, fragile)"""
    q = copy.deepcopy(p)
    q.theta, q.dt, q.dx, q.tol, q.nt = 0.7, 300.0, 300.0, 1.5e-6, nt
    for bc in (q.us, q.ds):
        if bc.target is not None:
            bc.target = bc.target[:nt]
    return q


# per-reach channels and boundaries run on the kernels that read them: boundary classes 0 and -1 (fs_dispatch.hpp: fits, hetero)
BATCH_ENTRIES = [e for e in ENTRIES if not e.get("long_reach") and e["boundary_class"] <= 0]


@pytest.mark.parametrize("e", BATCH_ENTRIES, ids=[_id(e) for e in BATCH_ENTRIES])
def test_batch_placement_is_bitwise(e, monkeypatch):
    """~70 reaches, every one its own channel and node count, channels at indices 0, 1, 63, 64 and B-1 among others: each reach
    gives the bits of its own one-reach run on the same entry (memory: B N (KP + 32 P) 8 bytes of stage tables, ~60 MB here)"""
    base = [common(case(s)[0]) for s in BATCH_KINDS]
    base = [q for q in base if fits(e, q)]
    B = 70
    order = np.random.default_rng(e["index"]).permutation(np.resize(np.arange(len(base)), B))
    order[[0, 1, 63, 64, B - 1]] = [0, len(base) - 1, 1 % len(base), 2 % len(base), 3 % len(base)]
    probs = [base[i] for i in order]
    P = max(q.geo["irr_x"].shape[1] for q in probs)
    assert B * max(q.N for q in probs) * ((P + 16) // 16 * 16 + 32 * P) * 8 < 256 << 20
    history = bool(e["diag"])
    monkeypatch.setenv("FS_KERNEL_INDEX", str(e["index"]))
    try:
        with per_reach_polyline_batch(probs, history=history, monitor=history) as b:
            assert b.poly_tables() == 1
            b.step(probs[0].nt - 1)
            assert b.kernel_index() == e["index"]
            assert np.all(b.status() == 0), b.status()
            its = b.iterations(0, probs[0].nt)
            h, Q = b.state()
            hist = b.history_arrays(0, probs[0].nt) if history else None
        singles = {}
        for i, q in enumerate(base):
            with per_reach_polyline_batch([q], history=history, monitor=history) as c:
                c.step(q.nt - 1)
                assert np.all(c.status() == 0)
                singles[i] = (c.iterations(0, q.nt)[:, 0], c.state(), c.history_arrays(0, q.nt) if history else None)
    finally:
        monkeypatch.delenv("FS_KERNEL_INDEX", raising=False)
    for i, q in enumerate(base):               # each distinct channel against the oracle, once
        ref = O.newton_run(q, trace=True)
        assert ref["status"] == 0 and not PE.fragile(ref, q.tol), BATCH_KINDS[i]
        its1, (h1, Q1), _ = singles[i]
        assert rel_err(h1[0, :q.N], ref["depth"][-1], 1e-3) <= TOL and rel_err(Q1[0, :q.N], ref["flow"][-1], 1.0) <= TOL, i
        assert np.array_equal(its1, ref["iters"]), (i, its1, ref["iters"])
    for r, i in enumerate(order):
        n = base[i].N
        its1, (h1, Q1), hist1 = singles[i]
        assert np.array_equal(its[:, r], its1), (r, i)
        assert np.array_equal(h[r, :n], h1[0, :n]) and np.array_equal(Q[r, :n], Q1[0, :n]), (r, i)
        if history:
            assert np.array_equal(hist[0][:, r, :n], hist1[0][:, 0, :n]) and np.array_equal(hist[1][:, r, :n], hist1[1][:, 0, :n]), (r, i)


@pytest.mark.parametrize("e", ENTRIES, ids=[_id(e) for e in ENTRIES])
def test_launch_context_does_not_leak(e, monkeypatch):
    """a case, then a class -1 per-reach table batch (another kernel, large LDS, other data), then the same case: the same bits.  A read
    of LDS or registers before they are written shows up here as a difference."""
    spec = specs_for(e)[0] if e.get("long_reach") else ("near_vertex_mixed", 64, 3)
    p = case(spec)[0]
    first = run_entry(e, p, monkeypatch, history=bool(e["diag"]))
    mids = []
    for name in ("storage_curve_poly_losses", "storage_curve_power_trap", "storage_curve_closed"):
        fx, meta = O.load_fixture(os.path.join(GOLDEN, name + ".npz"))
        mids.append(O.problem_from_fixture(fx, meta))
    with hetero_batch_from_problems(mids, mode="table") as b:      # per-reach tables and reservoirs: a class -1 table kernel
        b.step(max(t.nt for t in mids) - 1)
        m = A.kernel_table()[b.kernel_index()]
        assert m["section_mode"] == A.SEC_TABLE and m["boundary_class"] == -1, m
        assert np.all(b.status() == 0)
    second = run_entry(e, p, monkeypatch, history=bool(e["diag"]))
    for a, b_ in zip(first[:3], second[:3]):
        assert all(np.array_equal(x, y) for x, y in zip(a, b_)) if isinstance(a, tuple) else np.array_equal(a, b_)
    if first[3] is not None:
        assert np.array_equal(first[3][0], second[3][0]) and np.array_equal(first[3][1], second[3][1])
