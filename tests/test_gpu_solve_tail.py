"""The solve's tail of the step kernels - the back-substituted update kept as p + m and p - m and applied after the acceptance block
with one fma per unknown, the continuity residual of the back-substitution with T / (2 dt) as one constant - and the boundary rows
around it, against the oracle, on the smallest shapes that take each path:

    full-16x4    the flagship entry, 4 096 nodes (the only size it takes): the boundary row in the last lane of wave 3
    ragged-1025  its ragged sibling: the boundary row in lane 0 of wave 1 (local row 0) ...
    ragged-3073  ... and in lane 0 of wave 3
    full-16x1    one wave per reach, 1 024 nodes: the root closed through lane reads
    trap-8x1     a trapezoid: the top width varies, 1/(2t) of every node is carried across the acceptance block to the update
    table-tail   a (2, 1) table entry of the tail-only form at 121 nodes: its lane masks ride in the update's factor
    f32-8x1      an fp32 rectangular entry: the pinned and fenced pending sums

Every shape is B = 3 reaches of one channel over 3 levels, started off uniform flow at every node (tests/iterate_recipes.py).
Bars: the suite's - 1e-8 of the oracle (floors 1e-3 m, 1 m3/s), fp32 5e-4 of the fp64 oracle run from the float32-rounded start.
The first iterate x1 (max_iter = 1) is held to the same bars: a wrong factor in the fused update moves it directly, where the fixed
point would hide it.  The normal-depth row is held to the oracle's iterates in its three cases (the usual one, a boundary bed level
of its own, an adverse slope) on the full and the ragged flagship entries and on the one-wave one.  The conditions on the recipes
themselves (the oracle alone solves each shape, the first update moves >= 99 % of the nodes) need no device and are not marked gpu.

Measured on an MI355X (worst of depth / flow over the three reaches; nothing is tightened to these): all levels fp64 <= 5.7e-14
(table-tail: flow 5.7e-12, the GERD fixture's flows), fp32 4.1e-7; x1 fp64 <= 6.0e-14 (table-tail 3.8e-12), fp32 3.1e-7; the row
cases <= 7.2e-14."""
import copy
import functools

import numpy as np
import pytest

from entry_recipes import fixture_problem, prismatic_problem
import failure_recipes as FR
from flowsim_amd import _abi as A
import iterate_recipes as IR
from kernel_harness import FIELDS, TOL, TOL_F32, assert_same_bits, batch_for_entry, rel_err, snapshot
from oracle import preissmann_oracle as O
from synth import rect_problem

LEVELS = 3
FS_NAN, FS_MAX_ITER = 2, 1


def _entry(name):
    nd = 2 + A.BC_NORMAL_DEPTH
    rect = dict(section_mode=A.SEC_RECT_UNIFORM, boundary_class=nd, long_reach=0, team=0)
    if name == "full-16x4":
        return FR.find_entry(dtype=A.F64, cells_per_thread=16, waves_per_reach=4, full=1, diag=0, **rect)
    if name in ("ragged-1025", "ragged-3073"):
        return FR.find_entry(dtype=A.F64, cells_per_thread=16, waves_per_reach=4, full=0, diag=0, **rect)
    if name == "full-16x1":
        return FR.find_entry(dtype=A.F64, cells_per_thread=16, waves_per_reach=1, full=1, diag=0, **rect)
    if name == "trap-8x1":
        return FR.find_entry(dtype=A.F64, section_mode=A.SEC_TRAP_UNIFORM, cells_per_thread=8, waves_per_reach=1, full=1, diag=0, long_reach=0, team=0)
    if name == "table-tail":
        return FR.find_entry(dtype=A.F64, section_mode=A.SEC_TABLE, cells_per_thread=2, waves_per_reach=1, tail=0, long_reach=0, team=0)
    if name == "f32-8x1":
        return FR.find_entry(dtype=A.F32, cells_per_thread=8, waves_per_reach=1, full=1, diag=1, **rect)
    raise KeyError(name)


SHAPES = ("full-16x4", "ragged-1025", "ragged-3073", "full-16x1", "trap-8x1", "table-tail", "f32-8x1")
NODES = {"full-16x4": 4096, "ragged-1025": 1025, "ragged-3073": 3073, "full-16x1": 1024, "trap-8x1": 512, "table-tail": 121, "f32-8x1": 512}


def _base(name):
    """(entry, unperturbed problem of LEVELS levels, section mode of the batch)"""
    e = _entry(name)
    if name == "trap-8x1":
        downstream = {A.BC_NORMAL_DEPTH: "normal", A.BC_RATING_POWER: "power", A.BC_RATING_BLEND: "blend"}[e["boundary_class"] - 2]
        p, mode = prismatic_problem(e, ("flow", downstream), True, n_steps=LEVELS), "trap_uniform"
    elif name == "table-tail":
        p, mode = fixture_problem("gerd", LEVELS), "table"
    else:
        p, mode = rect_problem(NODES[name], seed=NODES[name], n_steps=LEVELS), "rect_uniform"
    assert p.N == NODES[name] and p.nt == LEVELS + 1
    return e, p, mode


def _perturbed(e, p, tol):
    """B = 3 reaches of the channel, each off uniform flow at every node with its own seed (IR.perturbed), LEVELS levels long"""
    out = []
    for s in IR.SEEDS:
        q = IR.perturbed(p, s, IR.f32_of(e))
        q.nt, q.tol = LEVELS + 1, tol
        out.append(q)
    return out


@functools.lru_cache(maxsize=None)
def _case(name):
    """entry, problems at the level tolerance, mode, and the oracle's runs (computed once, shared, left unchanged):
    full = all levels; first = level 1 capped at one update (tolerance 1e-30: never accepted early)"""
    e, p, mode = _base(name)
    probs = _perturbed(e, p, IR.level_tol(e, p.N))
    full = tuple(FR.oracle_run(q) for q in probs)
    first = tuple(O.newton_run(IR.at_level_tol(q, IR.ITER_TOL), n_steps=1, max_iter_at={1: 1}) for q in probs)
    return dict(e=e, probs=probs, mode=mode, full=full, first=first)


def _snap(b, nt):
    return snapshot(b, nt, fields=FIELDS + ("guess",))


def _tol(e):
    return TOL_F32 if IR.f32_of(e) else TOL


# ---------------------------------------------------------------------------------------------------------------------------
# the recipes, on the oracle alone (no device)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES)
def test_the_oracle_solves_the_shape_and_the_first_update_moves(name):
    c = _case(name)
    for r, (p, full, first) in enumerate(zip(c["probs"], c["full"], c["first"])):
        assert full["status"] == 0 and np.all(full["iters"][1:] > 1), (r, full["status"], full["iters"])
        assert first["status"] == 1 and first["fail_level"] == 1 and first["iters"][1] == 1 and np.all(np.isfinite(first["x_next"]))
        h1 = IR.unknowns(first)[0]
        frac = float(np.mean(np.abs(h1 - p.h0) / p.h0 > 1e-4))
        print(f"TAIL {name} reach {r}: counts {full['iters'][1:]}, nodes moved by the first update {100 * frac:.2f} %, min depth {np.min(full['depth']):.3f}")
        assert frac >= 0.99 and np.min(full["depth"]) > 0 and np.min(h1) > 0


# ---------------------------------------------------------------------------------------------------------------------------
# on the device
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", SHAPES)
def test_every_level_against_the_oracle(name, monkeypatch):
    c = _case(name)
    e, probs, tol = c["e"], c["probs"], _tol(c["e"])
    monkeypatch.setenv("FS_KERNEL_INDEX", str(e["index"]))
    with batch_for_entry(probs, e, c["mode"]) as b:
        b.step(LEVELS)
        assert b.kernel_index() == e["index"]
        s = _snap(b, LEVELS + 1)
    assert np.all(s["status"] == 0), s["status"]
    worst = [0.0, 0.0]
    for r, ref in enumerate(c["full"]):
        d, f = ref["depth"], ref["flow"]
        hyd = s["hyd"][:, :, r]
        errs_h = [rel_err(hyd[:, 0], d[:, 0], 1e-3), rel_err(hyd[:, 2], d[:, -1], 1e-3), rel_err(s["state"][0][r], d[-1], 1e-3)]
        errs_q = [rel_err(hyd[:, 1], f[:, 0], 1.0), rel_err(hyd[:, 3], f[:, -1], 1.0), rel_err(s["state"][1][r], f[-1], 1.0)]
        if "hist" in s:
            errs_h.append(rel_err(s["hist"][0][:, r], d, 1e-3)); errs_q.append(rel_err(s["hist"][1][:, r], f, 1.0))
        worst = [max(worst[0], *errs_h), max(worst[1], *errs_q)]
        print(f"TAIL {name} reach {r}: counts {s['iters'][1:, r]} oracle {ref['iters'][1:]}")
    print(f"TAIL {name} | all levels | depth {worst[0]:.3e} flow {worst[1]:.3e}")
    assert worst[0] <= tol and worst[1] <= tol, worst
    for r, ref in enumerate(c["full"]):
        assert np.array_equal(s["iters"][:, r], ref["iters"]), (r, s["iters"][:, r], ref["iters"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", SHAPES)
def test_the_first_iterate_against_the_oracle(name, monkeypatch):
    c = _case(name)
    e, probs, tol = c["e"], c["probs"], _tol(c["e"])
    p0 = probs[0]
    monkeypatch.setenv("FS_KERNEL_INDEX", str(e["index"]))
    with batch_for_entry(probs, e, c["mode"]) as b:
        b.set_scheme(p0.theta, p0.dt, p0.dx, IR.ITER_TOL, 1)
        b.step(1)
        assert b.kernel_index() == e["index"]
        status, its, guess = b.status().copy(), b.iterations(0, 2), b.guess()
    worst = [0.0, 0.0]
    for r, ref in enumerate(c["first"]):
        h, Q = IR.unknowns(ref)
        worst = [max(worst[0], rel_err(guess[0][r], h, 1e-3)), max(worst[1], rel_err(guess[1][r], Q, 1.0))]
    print(f"TAIL {name} | x1 | depth {worst[0]:.3e} flow {worst[1]:.3e}")
    assert np.all(status == FS_MAX_ITER) and np.all(its[1] == 1), (status, its)
    assert worst[0] <= tol and worst[1] <= tol, worst


@pytest.mark.gpu
@pytest.mark.parametrize("name", SHAPES)
def test_one_launch_is_three_launches_and_a_restart_continues(name, monkeypatch):
    c = _case(name)
    e, probs, nt = c["e"], c["probs"], LEVELS + 1
    monkeypatch.setenv("FS_KERNEL_INDEX", str(e["index"]))
    with batch_for_entry(probs, e, c["mode"]) as b:
        b.step(LEVELS)
        one = _snap(b, nt)
    with batch_for_entry(probs, e, c["mode"]) as b:
        b.step(1)
        state1, guess1 = b.state(), b.guess()
        b.step(1); b.step(1)
        assert b.kernel_index() == e["index"]
        three = _snap(b, nt)
    assert_same_bits(one, three, what="one launch of three levels against three launches of one")
    assert np.all(one["status"] == 0)
    with batch_for_entry(probs, e, c["mode"]) as b:           # a fresh batch continues from level 1 of the split run
        b.restart(1, *state1, *guess1)
        b.step(LEVELS - 1)
        assert b.kernel_index() == e["index"]
        again = dict(status=b.status().copy(), iters=b.iterations(2, LEVELS - 1), hyd=b.hydrographs(2, LEVELS - 1), state=b.state(), guess=b.guess())
    want = dict(status=one["status"], iters=one["iters"][2:], hyd=one["hyd"][2:], state=one["state"], guess=one["guess"])
    assert_same_bits(want, again, what="restart from level 1")


@pytest.mark.gpu
@pytest.mark.parametrize("name", SHAPES)
def test_a_batch_of_three_is_each_reach_alone(name, monkeypatch):
    c = _case(name)
    e, probs, nt = c["e"], c["probs"], LEVELS + 1
    monkeypatch.setenv("FS_KERNEL_INDEX", str(e["index"]))
    with batch_for_entry(probs, e, c["mode"]) as b:
        b.step(LEVELS)
        together = _snap(b, nt)
    for r, p in enumerate(probs):
        with batch_for_entry([p], e, c["mode"]) as b:
            b.step(LEVELS)
            assert b.kernel_index() == e["index"]
            alone = _snap(b, nt)
        # reach r of the batch: status [B]; iters [levels, B]; hyd [levels, 4, B]; state, guess ([B, N], [B, N]); hist ([levels, B, N], ...)
        pick = {k: v[r:r + 1] if k == "status" else v[..., r:r + 1] if k in ("iters", "hyd") else
                tuple(a[:, r:r + 1] if k == "hist" else a[r:r + 1] for a in v) for k, v in together.items()}
        assert_same_bits(pick, alone, what=f"reach {r} alone")


# ---- the normal-depth row: the usual case, a boundary bed level of its own (the retained block), an adverse slope ----
ROW_CASES = ("usual", "own_bed_level", "adverse_slope")
ROW_SHAPES = ("full-16x4", "ragged-1025", "full-16x1")
# the iterates of level 1 held to the oracle.  An adverse slope asks the outflow to reverse within one update (Q = -sqrt|S0| K): the
# oracle's own second iterate has negative depths and is not finite, so that case is held at x1 - which sees the row's sign, its
# residual and its derivative directly
ROW_ITERATES = {"usual": (1, 2), "own_bed_level": (1, 2), "adverse_slope": (1,)}


@functools.lru_cache(maxsize=None)
def _row_case(name, case):
    """the shape's problems with the downstream boundary edited, and the oracle's first two iterates of level 1"""
    e, p, mode = _base(name)
    p = copy.deepcopy(p)
    if case == "own_bed_level":           # hw of the derivative is h + bed_level, of the residual z_min + h (boundary.py:80, :161-181): they differ
        p.ds.bed_level = 0.35
    elif case == "adverse_slope":         # S0 < 0: the row's sign(S0) sqrt|S0| (hydraulics.py:4-13)
        p.ds.bed_slope = -p.ds.bed_slope
    probs = _perturbed(e, p, IR.ITER_TOL)
    refs = tuple({m: O.newton_run(q, n_steps=1, max_iter_at={1: m}) for m in ROW_ITERATES[case]} for q in probs)
    return dict(e=e, probs=probs, mode=mode, refs=refs)


@pytest.mark.parametrize("case", ROW_CASES)
@pytest.mark.parametrize("name", ROW_SHAPES)
def test_the_row_cases_move_the_oracle(name, case):
    """(no device) the edited boundary is seen by the first iterate: it differs from the usual case's by far more than the bar"""
    if case == "usual":
        return
    for ref, usual in zip(_row_case(name, case)["refs"], _row_case(name, "usual")["refs"]):
        assert all(ref[m]["status"] == 1 and np.all(np.isfinite(ref[m]["x_next"])) for m in ROW_ITERATES[case])
        moved = max(rel_err(ref[1]["x_next"][0::2], usual[1]["x_next"][0::2], 1e-3), rel_err(ref[1]["x_next"][1::2], usual[1]["x_next"][1::2], 1.0))
        print(f"TAIL {name} {case}: x1 differs from the usual case's by {moved:.2e}")
        assert moved >= 100 * TOL


@pytest.mark.gpu
@pytest.mark.parametrize("case", ROW_CASES)
@pytest.mark.parametrize("name", ROW_SHAPES)
def test_the_normal_depth_row_against_the_oracle(name, case, monkeypatch):
    c = _row_case(name, case)
    e, probs = c["e"], c["probs"]
    p0 = probs[0]
    monkeypatch.setenv("FS_KERNEL_INDEX", str(e["index"]))
    for m in ROW_ITERATES[case]:
        with batch_for_entry(probs, e, c["mode"]) as b:
            b.set_scheme(p0.theta, p0.dt, p0.dx, IR.ITER_TOL, m)
            b.step(1)
            assert b.kernel_index() == e["index"]
            status, its, guess = b.status().copy(), b.iterations(0, 2), b.guess()
        worst = [0.0, 0.0]
        for r, ref in enumerate(c["refs"]):
            h, Q = IR.unknowns(ref[m])
            worst = [max(worst[0], rel_err(guess[0][r], h, 1e-3)), max(worst[1], rel_err(guess[1][r], Q, 1.0))]
        print(f"TAIL {name} {case} | x{m} | depth {worst[0]:.3e} flow {worst[1]:.3e}")
        assert np.all(status == FS_MAX_ITER) and np.all(its[1] == m), (status, its)
        assert worst[0] <= TOL and worst[1] <= TOL, worst


# ---- a NaN in the target hydrograph still ends the reach in FS_NAN, at the level tests/failure_recipes.py says ----
@pytest.mark.gpu
@pytest.mark.parametrize("name", SHAPES)
def test_a_nan_target_ends_in_fs_nan(name, monkeypatch):
    c = _case(name)
    e, K = c["e"], FR.K_STAR
    assert K < LEVELS
    bad = [FR.edited(p, K, np.nan) for p in c["probs"][:1]] + list(c["probs"][1:])       # reach 0 fails, its neighbours do not
    ref = FR.oracle_run(bad[0])
    assert ref["status"] == FS_NAN and ref["fail_level"] == K
    monkeypatch.setenv("FS_KERNEL_INDEX", str(e["index"]))
    with batch_for_entry(bad, e, c["mode"]) as b:
        b.step(LEVELS)
        assert b.kernel_index() == e["index"]
        s = _snap(b, LEVELS + 1)
    with batch_for_entry(c["probs"], e, c["mode"]) as b:
        b.step(LEVELS)
        clean = _snap(b, LEVELS + 1)
    assert list(s["status"]) == [FS_NAN, 0, 0], s["status"]
    assert s["iters"][K, 0] == ref["iters"][K] and np.all(s["iters"][K + 1:, 0] == 0), s["iters"][:, 0]
    assert np.array_equal(s["iters"][:K, 0], clean["iters"][:K, 0]) and np.array_equal(s["hyd"][:K, :, 0], clean["hyd"][:K, :, 0])
    assert np.array_equal(s["iters"][:, 1:], clean["iters"][:, 1:]) and np.array_equal(s["hyd"][:, :, 1:], clean["hyd"][:, :, 1:])
    assert all(np.array_equal(x[1:], y[1:]) for x, y in zip(s["state"], clean["state"]))
