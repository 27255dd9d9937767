"""The fold of the full-grid rectangular fp64 kernels: the downstream boundary row put into the last lane's last row by selects, and
the 4 M level constants read from LDS two cells ahead of the cell that uses them (fs_kernel.hpp, kFoldFlat / kFoldAhead).

The shapes are the smallest at which that code can go wrong: FULL lane grids - N = 64 W M, so that the last lane's last row is the
boundary row and every other lane's last row is a cell -

    4 096 nodes (16, 4)    2 048 (16, 2)    1 024 (16, 1)    512 (8, 1)

each as B = 3 of bench.py's C3 reaches (c3_reach_parameters) under a flow hydrograph, 4 levels, with three downstream boundaries:

    normal   normal depth: the kernels compiled for that boundary pair (class 5), full grid, no diagnostics
    power    a power rating curve through the uniform-flow point: not one of the closed-form rows, so the dispatcher takes the general
             kernels with the run-time switch over the kinds (class 0, boundary parameters in LDS), which exist in the ragged form only
    fixed    a fixed depth (the uniform-flow depth): a closed-form row, the rectangular kernels of class 1 (parameters in LDS), full grid

Which instantiation ran is asserted from the dispatch table.  Each case is run from uniform flow and once more from a depth rippled by 1 %
along the reach: from uniform flow the hydrograph's wave does not reach the last node within 4 levels and the downstream row sits at its
fixed point, where a wrong entry of it would move nothing; with the ripple the three downstream boundaries give depths 6e-4 ... 1.5e-2 m
apart (the oracle's), five orders above the bar.

Held to the C oracle at the project's parity bar - 1e-8 relative on h and Q (floors 1e-3 m, 1 m3/s), Newton counts equal level by
level.  Chunked stepping (2 + 2 levels against 4 in one launch) is held bit for bit: a constant read ahead of the level pass that
rewrites it would show there.  The ragged sibling (4 000 nodes) and the kernels with history and monitor (4 096) are held to the
oracle too, and diagnostics on against off bit for bit: equal Newton counts, equal hydrograph rows.

Measured on an MI355X (nothing is tightened to these): worst of depth / flow over every case 8.8e-14 against the oracle, counts equal;
diagnostics on against off bit-equal from both starts; the whole file 1.6 s."""
import functools

import numpy as np
import pytest

from flowsim_amd import _abi as A
from kernel_harness import TOL, assert_same_bits, entry_of, rel_err, snapshot
from oracle import c_oracle
from oracle import preissmann_oracle as O

pytestmark = pytest.mark.gpu
B, LEVELS = 3, 4
THETA, DT, DX, LEVEL_TOL = 0.6, 600.0, 250.0, 1e-6
SHAPES = {4096: (16, 4), 2048: (16, 2), 1024: (16, 1), 512: (8, 1)}
DOWNSTREAM = ("normal", "power", "fixed")
# (full, boundary class or None for 2 + BC_NORMAL_DEPTH, diag) of the entry each downstream boundary is dispatched to
ENTRY = {"normal": (1, None, 0), "power": (0, 0, 1), "fixed": (1, 1, 1)}
RATING_EXPONENT = 1.5
STARTS = ("uniform", "rippled")
RIPPLE = 0.01


def _parameters(N):
    from flowsim_amd.synthetic import c3_reach_parameters, inflow_table, normal_depth_rect
    b_, n_, S0, Qb = c3_reach_parameters(0, B)
    hn = normal_depth_rect(b_, n_, S0, Qb)
    return b_, n_, S0, Qb, hn, inflow_table(Qb, LEVELS + 1, DT)


def _start_depth(N, hn, start):
    """[B, N]: the uniform-flow depth of every reach, rippled along the reach (its own phase per reach) or not"""
    h = np.repeat(np.asarray(hn)[:, None], N, axis=1)
    if start == "rippled":
        h = h * (1.0 + RIPPLE * np.sin(0.37 * np.arange(N)[None, :] + np.arange(len(hn))[:, None]))
    return h


def _problem(N, ds, j, start):
    b_, n_, S0, Qb, hn, tgt = _parameters(N)
    L = (N - 1) * DX
    geo = {k: np.zeros(N) for k in O.GEO_KEYS}
    geo["b_main"][:] = b_[j]; geo["n_main"][:] = n_[j]; geo["n_left"][:] = n_[j]; geo["n_right"][:] = n_[j]
    geo["z_bed"] = S0[j] * L * (1 - np.arange(N) / (N - 1))
    if ds == "normal":
        down = O.BC("normal_depth", bed_level=0.0, bed_slope=S0[j])
    elif ds == "fixed":
        down = O.BC("fixed_depth", bed_level=0.0, initial_depth=hn[j])
    else:       # Q = a Y^1.5 through the uniform-flow point of the reach
        down = O.BC("rating_curve", bed_level=0.0, rc_type="power", rc=dict(a=Qb[j] / hn[j] ** RATING_EXPONENT, b=RATING_EXPONENT, shift=0.0))
    return O.Problem(geo=geo, h0=_start_depth(N, hn, start)[j], Q0=np.full(N, Qb[j]), us=O.BC("flow_hydrograph", bed_level=S0[j] * L, target=tgt[:, j]),
                     ds=down, theta=THETA, dt=DT, dx=DX, nt=LEVELS + 1, tol=LEVEL_TOL)


@functools.lru_cache(maxsize=None)
def _reference(N, ds, start="uniform"):
    """the C oracle on the B reaches: computed once, shared, read only"""
    refs = []
    for j in range(B):
        r = c_oracle.run(_problem(N, ds, j, start))
        assert r["status"] == 0 and np.all(r["iters"][1:] > 1), (N, ds, start, j, r["status"], r["iters"])
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        refs.append(r)
    return tuple(refs)


def _batch(N, ds, start="uniform", history=False, monitor=False):
    from flowsim_amd import BoundarySpec, PreissmannBatch
    b_, n_, S0, Qb, hn, tgt = _parameters(N)
    b = PreissmannBatch(B, N, LEVELS + 1, dtype="f64", section_mode="rect_uniform", history=history, monitor=monitor)
    b.set_scheme(THETA, DT, DX, LEVEL_TOL, 100)
    b.set_geometry_uniform(b_, n_, S0 * (N - 1) * DX, np.zeros(B))
    if ds == "normal":
        b.set_boundary(A.DOWNSTREAM, BoundarySpec(A.BC_NORMAL_DEPTH, dict(bed_slope=S0, bed_level=np.zeros(B))))
    elif ds == "fixed":
        b.set_boundary(A.DOWNSTREAM, BoundarySpec(A.BC_FIXED_DEPTH, dict(initial_depth=hn)))
    else:
        b.set_boundary(A.DOWNSTREAM, BoundarySpec(A.BC_RATING_POWER, dict(a=Qb / hn ** RATING_EXPONENT, b=np.full(B, RATING_EXPONENT),
                                                                          stage_shift=np.zeros(B), bed_level=np.zeros(B))))
    b.set_boundary(A.UPSTREAM, BoundarySpec(A.BC_FLOW_HYDROGRAPH, {}, tgt))
    if start == "uniform":
        b.set_state_uniform(hn, Qb)
    else:
        b.set_state(_start_depth(N, hn, start), np.repeat(Qb[:, None], N, axis=1))
    return b


def _assert_entry(b, shape, ds, full=None, diag=None):
    e = entry_of(b)
    full = ENTRY[ds][0] if full is None else full
    diag = ENTRY[ds][2] if diag is None else diag
    want_class = 2 + A.BC_NORMAL_DEPTH if ENTRY[ds][1] is None else ENTRY[ds][1]
    got = (e["dtype"], e["section_mode"], e["cells_per_thread"], e["waves_per_reach"], e["full"], e["boundary_class"], e["diag"], e["long_reach"], e["team"])
    assert got == (A.F64, A.SEC_RECT_UNIFORM, shape[0], shape[1], full, want_class, diag, 0, 0), e


def _against_the_oracle(b, refs, what):
    """boundary rows of every level, state of the last one, history where the batch keeps it, counts: every figure printed, then asserted"""
    nt = LEVELS + 1
    hyd, (h, Q), its = b.hydrographs(0, nt), b.state(), b.iterations(0, nt)
    hist = b.history_arrays(0, nt) if b.history else None
    for j, r in enumerate(refs):
        eh = [rel_err(hyd[:, 0, j], r["depth"][:, 0], 1e-3), rel_err(hyd[:, 2, j], r["depth"][:, -1], 1e-3), rel_err(h[j], r["depth"][-1], 1e-3)]
        eq = [rel_err(hyd[:, 1, j], r["flow"][:, 0], 1.0), rel_err(hyd[:, 3, j], r["flow"][:, -1], 1.0), rel_err(Q[j], r["flow"][-1], 1.0)]
        if hist is not None:
            eh.append(rel_err(hist[0][:, j], r["depth"], 1e-3)); eq.append(rel_err(hist[1][:, j], r["flow"], 1.0))
        print(f"FOLD-READS {what} reach {j}: depth {max(eh):.3e} flow {max(eq):.3e}  counts {its[1:, j]} oracle {r['iters'][1:]}")
        assert max(eh) <= TOL and max(eq) <= TOL, (what, j, eh, eq)
        assert np.array_equal(its[:, j], r["iters"]), (what, j, its[:, j], r["iters"])


@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("ds", DOWNSTREAM)
@pytest.mark.parametrize("N", sorted(SHAPES))
def test_full_grids_against_the_c_oracle(N, ds, start):
    with _batch(N, ds, start) as b:
        b.step(LEVELS)
        assert np.all(b.status() == 0), b.status()
        _assert_entry(b, SHAPES[N], ds)
        _against_the_oracle(b, _reference(N, ds, start), f"{N} {ds} {start}")


@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("ds", DOWNSTREAM)
@pytest.mark.parametrize("N", sorted(SHAPES))
def test_two_launches_of_two_levels_give_the_bits_of_one_of_four(N, ds, start):
    out = []
    for chunks in ((LEVELS,), (2, LEVELS - 2)):
        with _batch(N, ds, start) as b:
            for n in chunks:
                b.step(n)
            _assert_entry(b, SHAPES[N], ds)
            out.append(snapshot(b, LEVELS + 1, fields=("state", "guess", "hyd", "iters", "status")))
    assert np.all(out[0]["status"] == 0), out[0]["status"]
    assert_same_bits(*out, what=(N, ds, start))


@pytest.mark.parametrize("start", STARTS)
def test_the_ragged_sibling_against_the_c_oracle(start):
    N = 4000
    with _batch(N, "normal", start) as b:
        b.step(LEVELS)
        assert np.all(b.status() == 0), b.status()
        _assert_entry(b, (16, 4), "normal", full=0, diag=0)
        _against_the_oracle(b, _reference(N, "normal", start), f"4000 ragged {start}")


@pytest.mark.parametrize("start", STARTS)
def test_history_and_monitor_on_against_the_oracle_and_against_off(start):
    N = 4096
    with _batch(N, "normal", start, history=True, monitor=True) as b:
        b.step(LEVELS)
        assert np.all(b.status() == 0), b.status()
        _assert_entry(b, (16, 4), "normal", full=1, diag=1)
        _against_the_oracle(b, _reference(N, "normal", start), f"4096 diagnostics {start}")
        on = (b.hydrographs(0, LEVELS + 1), b.iterations(0, LEVELS + 1))
    with _batch(N, "normal", start) as b:
        b.step(LEVELS)
        _assert_entry(b, (16, 4), "normal", full=1, diag=0)
        off = (b.hydrographs(0, LEVELS + 1), b.iterations(0, LEVELS + 1))
    diff = float(np.max(np.abs(on[0] - off[0]) / np.maximum(np.abs(on[0]), 1e-3)))
    print(f"FOLD-READS diagnostics on against off ({start}): hydrograph rows differ by {diff:.3e}, bit-equal {np.array_equal(on[0], off[0])}")
    assert np.array_equal(on[1], off[1])
    assert np.array_equal(on[0], off[0])
