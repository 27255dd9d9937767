"""Boundary forcing built on the device: fs_batch_set_bc_sampled (Hydrograph.sample of a table each member scales, lifts and delays)
and fs_batch_route_pool (GerdHydrograph.build for every member at once), against numpy, against the reference's own routing
(tests/golden/pool_routing.npz, tools/gen_pool_routing_golden.py) and against its default case (tests/golden/gerd_full.npz).

Bars of the pool: brentq stops within (2e-12 + 4 eps 645) / 2 = 1.3e-12 m of the root, two valid evaluation paths can end 2.6e-12 m
apart; times the steepest outlet slope in the bracket (5.7e3 m3/s per m) over the smallest release (1 562.5) that is 1e-11 relative.
Both bars carry a factor of ten over that: stage 3e-11 m, release 1e-10 relative."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from flowsim_amd import _abi as A
from flowsim_amd.batch import BoundarySpec, PreissmannBatch
from flowsim_amd.forcing import PoolSpec
from flowsim_amd.hydromodel.hydrograph import Hydrograph
from kernel_harness import rel_err

pytestmark = pytest.mark.gpu

DT, LEVELS = 3600.0, 385
FLOW = BoundarySpec(A.BC_FLOW_HYDROGRAPH)
WEIRS = [(196.4017, 624.9, 640.0), (447.3594, 640.0), (654.6723, 642.0)]      # cases/gerd_roseires/gerd_discharge.py


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "pool_routing.npz"))


@pytest.fixture(scope="module")
def pool(fx):
    return PoolSpec(fx["curve_stage"], fx["curve_volume"], WEIRS, base_flow=1562.5, vol_scale=1e-6, z_lo=624.9, z_hi=645.0)


def channel(B, L, dtype="f64", dt=DT):
    """a batch of short rectangular reaches with the scheme set: all the forcing kernels need"""
    b = PreissmannBatch(B, 30, L, dtype=dtype, section_mode="rect_uniform")
    b.set_scheme(0.6, dt, 1000.0, 1e-6, 100)
    return b


def two_tables(fx, K):
    """(times [K], values [2, K]): the shipped inflow table and a second one, or one point of each"""
    tab = fx["inflow_table"]
    assert len(tab) == 17
    t, v = tab[:K, 0], tab[:K, 1]
    return t, np.stack([v, 0.5 * v[::-1] + 100.0])


@pytest.mark.parametrize("B", [1, 65, 130])
@pytest.mark.parametrize("L", [2, LEVELS])
@pytest.mark.parametrize("K", [1, 17])
def test_sampler_is_np_interp_bit_for_bit(fx, B, L, K):
    t, v = two_tables(fx, K)
    rng = np.random.default_rng(B * 1000 + L + K)
    table_of = rng.integers(0, 2, B).astype(np.int32)
    scale, offset, shift = rng.uniform(0.25, 3.0, B), rng.uniform(-50.0, 50.0, B), rng.choice([0.0, 5400.0, -5400.0, 1234.5], B)
    plain = np.arange(B) % 3 == 0                      # these members are Hydrograph.sample itself
    scale[plain], offset[plain], shift[plain] = 1.0, 0.0, 0.0
    times = np.arange(L) * DT
    want = np.stack([offset[r] + scale[r] * np.interp(times - shift[r], t, v[table_of[r]]) for r in range(B)], axis=1)
    for r in np.flatnonzero(plain):
        assert np.array_equal(want[:, r], Hydrograph(table=np.column_stack([t, v[table_of[r]]])).sample(L, DT))
    with channel(B, L) as b:
        b.set_boundary_sampled(A.UPSTREAM, FLOW, t, v, table_of=table_of, scale=scale, offset=offset, shift=shift)
        got = b.bc_target(A.UPSTREAM)
        assert got.shape == (L, B) and np.array_equal(got, want)
        # no per-member vectors at all: every member is table 0 sampled as it is
        b.set_boundary_sampled(A.UPSTREAM, FLOW, t, v[0])
        assert np.array_equal(b.bc_target(A.UPSTREAM), np.tile(Hydrograph(table=np.column_stack([t, v[0]])).sample(L, DT)[:, None], (1, B)))
    with channel(B, L, dtype="f32") as b:
        b.set_boundary_sampled(A.UPSTREAM, FLOW, t, v, table_of=table_of, scale=scale, offset=offset, shift=shift)
        assert np.array_equal(b.bc_target(A.UPSTREAM), want.astype(np.float32).astype(np.float64))


def test_sampler_takes_each_reachs_own_time_step(fx):
    B, L = 65, 40
    t, v = two_tables(fx, 17)
    dts = np.linspace(900.0, 7200.0, B)
    with channel(B, L) as b:
        b.set_reach_scheme(dt=dts)
        b.set_boundary_sampled(A.UPSTREAM, BoundarySpec(A.BC_STAGE_HYDROGRAPH, dict(bed_level=0.0)), t, v[0])
        got = b.bc_target(A.UPSTREAM)
    for r in range(B):
        assert np.array_equal(got[:, r], Hydrograph(table=np.column_stack([t, v[0]])).sample(L, dts[r])), r


def routed(fx, pool, members, L=LEVELS, weir_scale=None, spec=None):
    """sample + route of the fixture's members `members` -> (release [L, B], stage [L, B], info)"""
    tab = fx["inflow_table"]
    with channel(len(members), L) as b:
        b.set_boundary_sampled(A.UPSTREAM, FLOW, tab[:, 0], tab[:, 1], scale=fx["scale"][members], shift=fx["shift"][members])
        info = b.route_pool(A.UPSTREAM, spec or pool, fx["initial_stage"][members], weir_scale=weir_scale)
        return b.bc_target(A.UPSTREAM), b.pool_stages(), info


def tiled(fx, B):
    n = len(fx["scale"]) - 1                           # the member without a bracket is the last one
    assert fx["no_bracket_level"][n] >= 0 and np.all(fx["no_bracket_level"][:n] < 0)
    return np.arange(B) % n


@pytest.mark.parametrize("B", [1, 65, 130])
def test_pool_is_the_references_routing(fx, pool, B):
    """measured on MI355X over the 23 bracketed members, B = 130: every stage bit equal, release within 4.43e-16 relative"""
    members = tiled(fx, B)
    release, stage, info = routed(fx, pool, members)
    assert np.all(info["flags"] == 0) and np.all(info["level"] == -1)
    dz = np.max(np.abs(stage - fx["stage"][:, members]))
    dq = np.max(np.abs(release - fx["release"][:, members]) / np.abs(fx["release"][:, members]))
    print(f"B={B}: worst stage error {dz:.3e} m, worst release error {dq:.3e}")
    assert dz <= 3e-11 and dq <= 1e-10
    n = len(fx["scale"]) - 1
    for r in range(n, B):                              # the tiles: identical bits in another lane and another workgroup
        assert np.array_equal(release[:, r], release[:, r - n]) and np.array_equal(stage[:, r], stage[:, r - n]), r
    # the default member against the reference's own default case, an independent run
    us = np.load(os.path.join(GOLDEN, "gerd_full.npz"))["us_target"]
    assert np.max(np.abs(release[:len(us), 0] - us) / np.abs(us)) <= 1e-10


def test_pool_over_two_levels(fx, pool):
    members = tiled(fx, 65)
    release, stage, _ = routed(fx, pool, members, L=2)
    assert release.shape == (2, 65)
    assert np.max(np.abs(stage - fx["stage"][:2, members])) <= 3e-11
    assert np.max(np.abs(release - fx["release"][:2, members]) / np.abs(fx["release"][:2, members])) <= 1e-10


def test_pool_of_an_fp32_batch_routes_in_fp64_and_rounds_once(fx, pool):
    """The inflow an fp32 batch holds is the sampled one rounded to fp32 (2^-24 relative); the recurrence does not amplify (DESIGN.md
    section 8), and the release is rounded to fp32 once more: 2 * 2^-24 = 1.2e-7, with a factor of ten 1.2e-6.  The stage stays fp64:
    it moves by the inflow's rounding times dt * vol_scale over the curve's slope (above 400 units per m around 637 m), below 1e-6 m."""
    members = tiled(fx, 65)
    tab = fx["inflow_table"]
    with channel(65, LEVELS, dtype="f32") as b:
        b.set_boundary_sampled(A.UPSTREAM, FLOW, tab[:, 0], tab[:, 1], scale=fx["scale"][members], shift=fx["shift"][members])
        info = b.route_pool(A.UPSTREAM, pool, fx["initial_stage"][members])
        release, stage = b.bc_target(A.UPSTREAM), b.pool_stages()
    assert np.all(info["flags"] == 0)
    assert np.array_equal(release, release.astype(np.float32).astype(np.float64))
    dq = np.max(np.abs(release - fx["release"][:, members]) / np.abs(fx["release"][:, members]))
    dz = np.max(np.abs(stage - fx["stage"][:, members]))
    print(f"fp32 batch: worst release error {dq:.3e}, worst stage error {dz:.3e} m")
    assert dq <= 1.2e-6 and dz <= 1e-6


def test_member_without_a_bracket(fx, pool):
    bad = len(fx["scale"]) - 1
    lvl = int(fx["no_bracket_level"][bad])
    members = tiled(fx, 65)
    clean = routed(fx, pool, members)
    members[7] = bad
    tab = fx["inflow_table"]
    with channel(65, LEVELS) as b:
        b.set_geometry_uniform(np.full(65, 300.0), np.full(65, 0.03), np.full(65, 29 * 1000.0 * 2e-4), np.zeros(65))
        b.set_boundary_sampled(A.UPSTREAM, FLOW, tab[:, 0], tab[:, 1], scale=fx["scale"][members], shift=fx["shift"][members])
        info = b.route_pool(A.UPSTREAM, pool, fx["initial_stage"][members])
        release, stage = b.bc_target(A.UPSTREAM), b.pool_stages()
        assert info["flags"][7] == A.POOL_NO_BRACKET and info["level"][7] == lvl
        assert np.all(np.delete(info["flags"], 7) == 0) and np.all(np.delete(info["level"], 7) == -1)
        assert np.max(np.abs(stage[:lvl, 7] - fx["stage"][:lvl, bad])) <= 3e-11
        assert np.max(np.abs(release[:lvl, 7] - fx["release"][:lvl, bad]) / np.abs(fx["release"][:lvl, bad])) <= 1e-10
        assert np.all(np.isnan(release[lvl:, 7])) and np.all(np.isnan(stage[lvl:, 7]))
        others = np.arange(65) != 7
        assert np.array_equal(release[:, others], clean[0][:, others]) and np.array_equal(stage[:, others], clean[1][:, others])
        # each member starts from its own level-0 release at normal depth; the NaN target reaches the flagged member at `lvl`
        q0 = release[0]
        h0 = (q0 * 0.03 / (300.0 * np.sqrt(2e-4))) ** 0.6
        b.set_boundary(A.DOWNSTREAM, BoundarySpec(A.BC_NORMAL_DEPTH, dict(bed_slope=2e-4, bed_level=0.0)))
        b.set_state_uniform(h0, q0)
        b.step(lvl + 1)
        st = b.status()
        assert st[7] == A.NAN and np.all(st[others] == A.OK), st


def test_a_gate_out_of_service_is_a_pool_without_it(fx, pool):
    members = tiled(fx, 65)
    scale = np.ones((3, 65))
    scale[0] = 0.0
    off = routed(fx, pool, members, weir_scale=scale)
    without = routed(fx, pool, members, spec=pool.without_weir(0))
    # (without the gated spillway some pools leave the bracket: those members are flagged, at the same level, in both runs)
    assert np.array_equal(off[2]["flags"], without[2]["flags"]) and np.array_equal(off[2]["level"], without[2]["level"])
    assert np.any(off[2]["flags"] == 0)
    assert np.array_equal(off[0], without[0], equal_nan=True) and np.array_equal(off[1], without[1], equal_nan=True)
    assert not np.array_equal(off[0], routed(fx, pool, members)[0], equal_nan=True)


def test_order_and_misuse_leave_the_batch_usable(fx, pool):
    tab = fx["inflow_table"]
    E = A.FlowsimError
    with PreissmannBatch(3, 30, 8, section_mode="rect_uniform") as b:
        with pytest.raises(E, match="scheme"):
            b.set_boundary_sampled(A.UPSTREAM, FLOW, tab[:, 0], tab[:, 1])
        b.set_scheme(0.6, DT, 1000.0, 1e-6, 100)
        with pytest.raises(E, match="target"):
            b.route_pool(A.UPSTREAM, pool, 637.0)                                  # no target yet
        with pytest.raises(E, match="target"):
            b.bc_target(A.UPSTREAM)
        b.set_boundary_sampled(A.DOWNSTREAM, BoundarySpec(A.BC_STAGE_HYDROGRAPH, dict(bed_level=0.0)), tab[:, 0], tab[:, 1])
        with pytest.raises(E, match="FS_BC_FLOW_HYDROGRAPH"):
            b.route_pool(A.DOWNSTREAM, pool, 637.0)                                # a stage hydrograph is no inflow
        with pytest.raises(E, match="no pool"):
            b.pool_stages()
        lib = A.lib()
        t = np.ascontiguousarray(tab[::-1, 0])
        v = np.ascontiguousarray(tab[:, 1])
        D = A._D
        assert lib.fs_batch_set_bc_sampled(b._h, 0, A.BC_FLOW_HYDROGRAPH, None, 0, t.ctypes.data_as(D), v.ctypes.data_as(D), 17, 1, None, None, None, None) != 0
        assert b"increasing" in lib.fs_last_error()
        idx = np.array([0, 1, 0], dtype=np.int32)
        t = np.ascontiguousarray(tab[:, 0])
        assert lib.fs_batch_set_bc_sampled(b._h, 0, A.BC_FLOW_HYDROGRAPH, None, 0, t.ctypes.data_as(D), v.ctypes.data_as(D), 17, 1, idx.ctypes.data_as(A._I), None, None, None) != 0
        assert b"table_of" in lib.fs_last_error()
        assert lib.fs_batch_set_bc_sampled(b._h, 0, A.BC_FIXED_DEPTH, None, 0, t.ctypes.data_as(D), v.ctypes.data_as(D), 17, 1, None, None, None, None) != 0
        # and the batch works
        b.set_boundary_sampled(A.UPSTREAM, FLOW, tab[:, 0], tab[:, 1])
        info = b.route_pool(A.UPSTREAM, pool, 637.0)
        assert np.all(info["flags"] == 0)
        assert np.max(np.abs(b.bc_target(A.UPSTREAM)[:, 0] - fx["release"][:8, 0]) / fx["release"][:8, 0]) <= 1e-10


# ---- end to end: a routed target drives the step kernels of the GERD -> Roseires reach to what the host-built one does ----
TOL = 1e-8                                              # the suite's parity bar (tests/test_gpu_dropin.py)


def assert_same_run(got, want, label):
    for col, floor in enumerate((1e-3, 1.0, 1e-3, 1.0)):          # h[0], Q[0], h[N-1], Q[N-1]
        err = rel_err(got["hydrographs"][:, col], want["hydrographs"][:, col], floor)
        print(label, "column", col, "relative error", err)
        assert err <= TOL, (label, col, err)
    assert np.array_equal(got["iterations"], want["iterations"]), label
    assert np.array_equal(got["status"], want["status"]) and np.all(want["status"] == A.OK), label


@pytest.fixture(scope="module")
def gerd_case():
    """(solver of the case over its 385 levels, the raw inflow table, the case's PoolSpec)"""
    from cases.gerd_roseires import settings as S
    from cases.gerd_roseires.gerd_discharge import GerdHydrograph
    from cases.gerd_roseires.inputs import import_hydrograph
    from cases.gerd_roseires.model import build
    solver, _ = build(inflow_hyd_func=None)
    assert solver.number_of_time_levels == LEVELS
    return solver, import_hydrograph(S.inflow_hyd_path), GerdHydrograph.pool_spec()


def host_release(solver, table, scale, shift, level):
    """the mirror's GerdHydrograph.build, on the host, for one member"""
    from cases.gerd_roseires.gerd_discharge import GerdHydrograph
    inflow = Hydrograph(function=lambda t: scale * float(np.interp(t - shift, table[:, 0], table[:, 1])))
    out = GerdHydrograph()
    out.build(inflow_hydrograph=inflow, time_step=solver.time_step, duration=(LEVELS - 1) * solver.time_step, initial_stage=level)
    return out


def test_gerd_ensemble_with_the_device_built_target_is_the_host_built_one(gerd_case):
    """8 members (the n study's values) over all 385 levels: sample + route from the inflow table on the device, against the same
    ensemble with the host-built release uploaded through set_boundary"""
    from cases.gerd_roseires import settings as S
    from flowsim_amd.ensemble import run_manning_ensemble, run_scenario_ensemble
    solver, table, spec = gerd_case
    ns = np.linspace(0.020, 0.060, 8)
    release = host_release(solver, table, 1.0, 0.0, S.initial_gerd_level)
    ch = solver.channel
    kept = ch.upstream_boundary.hydrograph, ch.initial_flow_rate
    try:
        ch.upstream_boundary.hydrograph, ch.initial_flow_rate = release, release.get_at(0)
        want = run_manning_ensemble(solver, ns, tolerance=S.tolerance, initial="gvf")
    finally:
        ch.upstream_boundary.hydrograph, ch.initial_flow_rate = kept
    got = run_scenario_ensemble(solver, spec, table, pool_level=S.initial_gerd_level, n_main=ns, tolerance=S.tolerance)
    assert np.all(got["pool"]["flags"] == 0) and np.array_equal(got["initial_flow"], np.full(8, release.get_at(0)))
    assert_same_run(got, want, "ensemble")


def test_scenario_sweep_is_its_members_run_one_at_a_time(gerd_case):
    """6 members that differ in inflow scale, timing and initial GERD level (and n) through run_scenario_ensemble, each against a
    single-member run of the mirror's GerdHydrograph.build + run_manning_ensemble"""
    from cases.gerd_roseires import settings as S
    from flowsim_amd.ensemble import run_manning_ensemble, run_scenario_ensemble
    solver, table, spec = gerd_case
    scale = np.array([0.5, 1.0, 1.5, 2.0, 2.5, 1.25])
    shift = np.array([0.0, 5400.0, -5400.0, 0.0, 5400.0, 0.0])
    level = np.array([640.0, 637.0, 634.125, 641.0, 632.0, 642.0])
    ns = np.array([0.030, 0.025, 0.035, 0.030, 0.040, 0.028])
    got = run_scenario_ensemble(solver, spec, table, inflow_scale=scale, inflow_shift=shift, pool_level=level, n_main=ns, tolerance=S.tolerance)
    assert np.all(got["pool"]["flags"] == 0)
    ch = solver.channel
    kept = ch.upstream_boundary.hydrograph, ch.initial_flow_rate
    try:
        for m in range(len(scale)):
            release = host_release(solver, table, scale[m], shift[m], level[m])
            ch.upstream_boundary.hydrograph, ch.initial_flow_rate = release, release.get_at(0)
            want = run_manning_ensemble(solver, ns[m:m + 1], tolerance=S.tolerance, initial="gvf")
            one = dict(hydrographs=got["hydrographs"][:, :, m:m + 1], iterations=got["iterations"][:, m:m + 1], status=got["status"][m:m + 1])
            assert abs(got["initial_flow"][m] - release.get_at(0)) <= 1e-10 * release.get_at(0)
            assert_same_run(one, want, f"member {m}")
    finally:
        ch.upstream_boundary.hydrograph, ch.initial_flow_rate = kept
