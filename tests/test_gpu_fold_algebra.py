"""The fold's regrouped arithmetic (fs_kernel.hpp step 2, fs_device.hpp node_terms_rect / _trap) against the C oracle.

What moved: the bed step's share of the water-surface slope rides in the level constant kc3 (cq dz) and the slope term S is two
fmas, the fast paths hand the fold half of dSe/dQ (the 2 lives in a constant) and R^(-2/3) is corrected directly: the residuals
round differently, so the Newton COUNTS are compared, not only the fields.  The level
constants have two instances (ahead of the time loop, at acceptance inside it): chunked stepping must give the bits of one launch.

Bounds: 1e-8 relative (the project's parity bar) with identical Newton counts in fp64; fp32 within 5e-4 of fp64."""
import numpy as np
import pytest

from fixture_batch import batch_from_problems
from flowsim_amd import _abi as A
from kernel_harness import entry_of, rel_err
from oracle import c_oracle
from oracle import preissmann_oracle as O
from synth import akbari_shape, normal_depth_trap, trap_problem

pytestmark = pytest.mark.gpu
TOL = 1e-8
TOL_F32 = 5e-4


def check_rows(b, refs, tol=TOL, counts=True):
    """what a batch without history keeps - the boundary rows of every level, the state of the last one, the counts - against
    the oracle's depth / flow [nt, N] of every reach; every figure is printed before it is asserted"""
    nt = refs[0]["depth"].shape[0]
    hyd = b.hydrographs(0, nt)
    h, Q = b.state()
    its = b.iterations(0, nt)
    for j, r in enumerate(refs):
        n = r["depth"].shape[1]
        e = dict(h_us=rel_err(hyd[:, 0, j], r["depth"][:, 0], 1e-3), Q_us=rel_err(hyd[:, 1, j], r["flow"][:, 0], 1.0),
                 h_ds=rel_err(hyd[:, 2, j], r["depth"][:, -1], 1e-3), Q_ds=rel_err(hyd[:, 3, j], r["flow"][:, -1], 1.0),
                 h_end=rel_err(h[j, :n], r["depth"][-1], 1e-3), Q_end=rel_err(Q[j, :n], r["flow"][-1], 1.0))
        print(f"reach {j}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()) + f"  Newton iterations {int(its[:, j].sum())} / {int(r['iters'].sum())}")
        assert max(e.values()) <= tol, (j, e)
        if counts:
            assert np.array_equal(its[:, j], r["iters"]), (j, its[:, j], r["iters"])


# ---- the flagship shape: 8 of bench.py's C3 reaches x 4 096 nodes x 10 levels ----
C3 = dict(B=8, N=4096, nt=11, theta=0.6, dt=600.0, dx=250.0, tol=1e-6)


def c3_problem(b, n, S0, Qb, hn, target):
    N, L = C3["N"], (C3["N"] - 1) * C3["dx"]
    geo = {k: np.zeros(N) for k in O.GEO_KEYS}
    geo["b_main"][:] = b; geo["n_main"][:] = n; geo["n_left"][:] = n; geo["n_right"][:] = n
    geo["z_bed"] = S0 * L * (1 - np.arange(N) / (N - 1))
    return O.Problem(geo=geo, h0=np.full(N, hn), Q0=np.full(N, Qb), us=O.BC("flow_hydrograph", bed_level=S0 * L, target=target),
                     ds=O.BC("normal_depth", bed_level=0.0, bed_slope=S0), theta=C3["theta"], dt=C3["dt"], dx=C3["dx"], nt=C3["nt"], tol=C3["tol"])


def c3_batch():
    """as bench.py builds its headline batch (build_batch, workload c3): no history, no trace, no monitor"""
    from flowsim_amd import BoundarySpec, PreissmannBatch
    from flowsim_amd.synthetic import c3_reach_parameters, inflow_table, normal_depth_rect
    B, N, nt = C3["B"], C3["N"], C3["nt"]
    b_, n_, S0, Qb = c3_reach_parameters(0, B)
    hn = normal_depth_rect(b_, n_, S0, Qb)
    b = PreissmannBatch(B, N, nt, dtype="f64", section_mode="rect_uniform", monitor=False)
    b.set_scheme(C3["theta"], C3["dt"], C3["dx"], C3["tol"], 100)
    b.set_geometry_uniform(b_, n_, S0 * (N - 1) * C3["dx"], np.zeros(B))
    b.set_boundary(A.DOWNSTREAM, BoundarySpec(A.BC_NORMAL_DEPTH, dict(bed_slope=S0, bed_level=np.zeros(B))))
    b.set_boundary(A.UPSTREAM, BoundarySpec(A.BC_FLOW_HYDROGRAPH, {}, inflow_table(Qb, nt, C3["dt"])))
    b.set_state_uniform(hn, Qb)
    return b


@pytest.fixture(scope="module")
def c3_reference():
    """the C oracle on the same eight reaches, computed once and read only"""
    from flowsim_amd.synthetic import c3_reach_parameters, inflow_table, normal_depth_rect
    b_, n_, S0, Qb = c3_reach_parameters(0, C3["B"])
    hn = normal_depth_rect(b_, n_, S0, Qb)
    tgt = inflow_table(Qb, C3["nt"], C3["dt"])
    refs = []
    for j in range(C3["B"]):
        r = c_oracle.run(c3_problem(b_[j], n_[j], S0[j], Qb[j], hn[j], tgt[:, j]))
        assert r["status"] == 0
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        refs.append(r)
    return refs


def assert_flagship(b):
    e = entry_of(b)
    assert (e["cells_per_thread"], e["waves_per_reach"], e["full"], e["diag"]) == (16, 4, 1, 0), e
    assert e["boundary_class"] == 2 + A.BC_NORMAL_DEPTH and e["dtype"] == A.F64, e


def test_flagship_against_the_c_oracle(c3_reference):
    with c3_batch() as b:
        b.step(C3["nt"] - 1)
        assert np.all(b.status() == 0)
        assert_flagship(b)
        check_rows(b, c3_reference)


def test_chunked_stepping_gives_the_bits_of_one_launch():
    """1 + 3 + 6 levels in three launches against 10 in one: the level constants of a launch's entry level come from the instance
    ahead of the time loop, those of every later level from the one in the acceptance block - the same bits, or the two drifted"""
    out = []
    for chunks in ((10,), (1, 3, 6)):
        with c3_batch() as b:
            for n in chunks:
                b.step(n)
            assert np.all(b.status() == 0)
            assert_flagship(b)
            out.append(b.state() + b.guess() + (b.hydrographs(0, C3["nt"]), b.iterations(0, C3["nt"])))
    names = ("depth", "flow", "next start depth", "next start flow", "hydrograph rows", "Newton counts")
    for name, one, three in zip(names, *out):
        assert np.array_equal(one, three), name


# ---- a bed step that differs from cell to cell: what cq dz inside kc3 can get wrong and a prismatic reach cannot show ----
@pytest.mark.parametrize("N", [121, 100])      # 121: the ensemble shape; 100: padding rows behind node N - 1 (lanes 50 .. 63)
def test_varying_bed_step_on_the_two_rows_per_lane_table_kernel(N):
    rng = np.random.default_rng(20261018 + N)
    dx, dt, nt, S0 = 500.0, 600.0, 9, 4e-4
    drop = S0 * dx * (0.25 + 1.5 * rng.random(N - 1))                 # random positive bed drops per cell, mean slope S0
    geo = {k: np.zeros(N) for k in O.GEO_KEYS}
    geo["z_bed"] = np.concatenate([np.cumsum(drop[::-1])[::-1], [0.0]])
    geo["b_main"][:] = 40.0; geo["m_main"][:] = 1.5
    geo["n_main"][:] = 0.03; geo["n_left"][:] = 0.03; geo["n_right"][:] = 0.03
    Qb = 120.0
    hn = normal_depth_trap(40.0, 1.5, 0.03, S0, Qb)
    tgt = np.array([akbari_shape(Qb, 2 * Qb, 5 * 3600.0, 15 * 3600.0, k * dt) for k in range(nt)])
    p = O.Problem(geo=geo, h0=np.full(N, hn), Q0=np.full(N, Qb), us=O.BC("flow_hydrograph", bed_level=float(geo["z_bed"][0]), target=tgt),
                  ds=O.BC("normal_depth", bed_level=0.0, bed_slope=S0), theta=0.6, dt=dt, dx=dx, nt=nt, tol=1e-6)
    ref = c_oracle.run(p)
    assert ref["status"] == 0 and ref["iters"][1:].min() >= 2           # (a real transient: the bed is not the uniform-flow one)
    with batch_from_problems([p], mode="table", history=True) as b:
        b.step(nt - 1)
        assert np.all(b.status() == 0)
        e = entry_of(b)
        assert (e["cells_per_thread"], e["waves_per_reach"]) == (2, 1), e
        h, Q = b.history_arrays()
        eh, eq = rel_err(h[:, 0], ref["depth"], 1e-3), rel_err(Q[:, 0], ref["flow"], 1.0)
        its = b.iterations()[:, 0]
        print(f"N = {N}: depth {eh:.2e} flow {eq:.2e} over {nt} levels, Newton iterations {int(its.sum())} / {int(ref['iters'].sum())}")
        assert eh <= TOL and eq <= TOL
        assert np.array_equal(its, ref["iters"])
        check_rows(b, [ref])


# ---- a one-wave kernel that shares the fold: bench.py's C5 reaches, 512 nodes, in both precisions ----
def test_one_wave_trapezoid_kernel_in_both_precisions():
    from flowsim_amd import BoundarySpec, PreissmannBatch
    from flowsim_amd.synthetic import c5_reach_parameters, inflow_table, normal_depth_trap
    B, N, nt, dt, dx = 4, 512, 9, 1800.0, 500.0
    b_, m_, n_, S0, Qb = c5_reach_parameters(0, B)
    hn = normal_depth_trap(b_, m_, n_, S0, Qb)
    tgt = inflow_table(Qb, nt, dt)
    refs = []
    for j in range(B):
        p = trap_problem(b_[j], m_[j], n_[j], S0[j], Qb[j], N, nt - 1, dt=dt, dx=dx)
        p.us.target = tgt[:, j]; p.h0 = np.full(N, hn[j])
        p.ds.rc = dict(a=Qb[j] / hn[j] ** 1.6, b=1.6); p.ds.initial_depth = hn[j]
        refs.append(c_oracle.run(p))
        assert refs[-1]["status"] == 0
    got = {}
    for dtype in ("f64", "f32"):
        with PreissmannBatch(B, N, nt, dtype=dtype, section_mode="trap_uniform", monitor=False) as b:
            b.set_scheme(0.6, dt, dx, 1e-6 if dtype == "f64" else 1e-3, 100)
            b.set_geometry_uniform(b_, n_, S0 * (N - 1) * dx, np.zeros(B), side_slope=m_)
            b.set_boundary(A.DOWNSTREAM, BoundarySpec(A.BC_RATING_POWER, dict(a=Qb / hn ** 1.6, b=np.full(B, 1.6),
                                                                            stage_shift=np.zeros(B), bed_level=np.zeros(B))))
            b.set_boundary(A.UPSTREAM, BoundarySpec(A.BC_FLOW_HYDROGRAPH, {}, tgt))
            b.set_state_uniform(hn, Qb)
            b.step(nt - 1)
            assert np.all(b.status() == 0)
            e = entry_of(b)
            assert (e["cells_per_thread"], e["waves_per_reach"], e["full"], e["diag"]) == (8, 1, 1, 0), e
            assert e["boundary_class"] == 2 + A.BC_RATING_POWER and e["dtype"] == (A.F64 if dtype == "f64" else A.F32)
            if dtype == "f64":
                check_rows(b, refs)
            got[dtype] = (b.hydrographs(0, nt), b.state())
    (hyd64, (h64, Q64)), (hyd32, (h32, Q32)) = got["f64"], got["f32"]
    e = dict(h_rows=max(rel_err(hyd32[:, i], hyd64[:, i], 1e-3) for i in (0, 2)), Q_rows=max(rel_err(hyd32[:, i], hyd64[:, i], 1.0) for i in (1, 3)),
             h_end=rel_err(h32, h64, 1e-3), Q_end=rel_err(Q32, Q64, 1.0))
    print("fp32 against fp64: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert max(e.values()) <= TOL_F32, e
