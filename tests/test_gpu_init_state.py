"""Initial conditions on the device (fs_batch_init_state / PreissmannBatch.init_state) against the reference's own answers.

tests/golden/random_sweep.npz holds Channel.initial_conditions of 80 channels (23 'GVF_equation', 19 'steady-state', 38 'linear'),
tests/golden/gerd_ensemble.npz the per-member backwater profiles of the Manning-n study, tests/golden/init_state_polyline.npz the
backwater profiles of the sweep's 12 polyline channels (tools/gen_init_state_golden.py).  Depth is held to the tolerance the host
mirror is held to on the same fixtures (tests/test_random_sweep.py: rtol 1e-10, atol 1e-12), flow is exact; 'linear' to 1e-13.
The measured maxima are in DESIGN.md section 8."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from fixture_batch import batch_from_problems, is_rect_uniform, per_reach_polyline_batch
from flowsim_amd import PreissmannBatch
from flowsim_amd import _abi as A
from kernel_harness import rel_err
from oracle import preissmann_oracle as O
from oracle.gen_random_sweep import build_from_recipe

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-10, 1e-12
CASES = list(O.sweep_cases(os.path.join(GOLDEN, "random_sweep.npz")))
BY_IC = {ic: [c for c in CASES if c[2]["ic"] == ic] for ic in ("GVF_equation", "steady-state", "linear")}
POISON = 7.25          # a state the batch holds before init_state: whatever survives shows


def worst(got, want):
    """largest |got - want| / (ATOL + RTOL |want|): <= 1 passes"""
    return float(np.max(np.abs(got - want) / (ATOL + RTOL * np.abs(want))))


def pad(a, N):
    a = np.asarray(a, dtype=np.float64)
    return np.concatenate([a, np.repeat(a[-1:], N - len(a), axis=0)], axis=0)


def table_batch(probs, **kw):
    """one TABLE batch, every reach its own table, node count and dx; no boundaries, a poisoned state"""
    B, N = len(probs), max(p.N for p in probs)
    b = PreissmannBatch(B, N, 4, section_mode="table", **kw)
    b.set_scheme(0.6, 60.0, probs[0].dx)
    b.set_geometry_table({k: np.stack([pad(p.geo[k], N) for p in probs]) for k in A.GEO_ROWS})
    b.set_reach_nodes([p.N for p in probs])
    b.set_reach_scheme(dx=[p.dx for p in probs])
    b.set_state(np.full((B, N), POISON), np.full((B, N), POISON))
    return b


def rect_batch(width, manning, z_us, z_ds, nodes, dx, dtype="f64", mode="rect_uniform", side_slope=None):
    B, N = len(nodes), int(max(nodes))
    b = PreissmannBatch(B, N, 4, dtype=dtype, section_mode=mode)
    b.set_scheme(0.6, 60.0, float(np.atleast_1d(dx)[0]))
    b.set_geometry_uniform(width, manning, z_us, z_ds, **({} if side_slope is None else dict(side_slope=side_slope)))
    if len(set(nodes)) > 1:
        b.set_reach_nodes(nodes)
    if np.ndim(dx):
        b.set_reach_scheme(dx=dx)
    b.set_state(np.full((B, N), POISON), np.full((B, N), POISON))
    return b


def check_against(h, Q, members, what):
    """rows of a batch against the reference's initial_conditions of each member; nodes beyond a reach's own repeat its last"""
    top = 0.0
    for r, (i, ic) in enumerate(members):
        n = len(ic)
        w = worst(h[r, :n], ic[:, 0])
        top = max(top, w)
        assert w <= 1.0, (what, i, w, float(np.max(np.abs(h[r, :n] - ic[:, 0]))))
        assert np.array_equal(Q[r, :n], ic[:, 1]), (what, i)
        assert np.all(h[r, n:] == h[r, n - 1]) and np.all(Q[r, n:] == Q[r, n - 1]), (what, i)
    print(f"{what}: worst depth error {top:.3g} of the tolerance over {len(members)} reaches")


# ---- 1. backwater --------------------------------------------------------------------------------------------------------------
def test_backwater_matches_the_reference_in_one_heterogeneous_launch():
    cases = BY_IC["GVF_equation"]
    assert len(cases) == 23 and {m["N"] for _, _, m in cases} >= {3, 257}
    probs = [O.problem_from_fixture(fx, m) for _, fx, m in cases]
    members = [(i, fx["initial_conditions"]) for i, fx, _ in cases]
    flow = [ic[0, 1] for _, ic in members]
    h_ds = [ic[-1, 0] for _, ic in members]
    with table_batch(probs) as b:
        info = b.init_state("GVF_equation", flow, depth_ds=h_ds)
        assert not info["flags"].any() and np.all(info["node"] == -1)
        assert b.level == 0
        h, Q = b.state()
    check_against(h, Q, members, "backwater, per-reach tables")
    rect = [k for k, p in enumerate(probs) if is_rect_uniform(p)]
    assert len(rect) >= 3
    with rect_batch([probs[k].geo["b_main"][0] for k in rect], [probs[k].geo["n_main"][0] for k in rect],
                    [probs[k].geo["z_bed"][0] for k in rect], [probs[k].geo["z_bed"][-1] for k in rect],
                    [probs[k].N for k in rect], np.array([probs[k].dx for k in rect])) as b:
        info = b.init_state("GVF_equation", [flow[k] for k in rect], depth_ds=[h_ds[k] for k in rect])
        assert not info["flags"].any()
        h, Q = b.state()
    check_against(h, Q, [members[k] for k in rect], "backwater, rectangular fast path")


# ---- 2. normal depth -----------------------------------------------------------------------------------------------------------
def mirror_bed_slopes(m):
    solver, _, _ = build_from_recipe(m["recipe"])
    return np.array([xs.bed_slope for xs in solver.channel.xs_at_node], dtype=np.float64)


def test_normal_depth_matches_the_reference(monkeypatch):
    cases = BY_IC["steady-state"]
    assert len(cases) == 19
    trap = [c for c in cases if c[2]["family"] != "polyline"]
    poly = [c for c in cases if c[2]["family"] == "polyline"]
    assert len(poly) == 3 and min(m["N"] for _, _, m in cases) == 2
    probs = [O.problem_from_fixture(fx, m) for _, fx, m in trap]
    N = max(p.N for p in probs)
    slopes = np.stack([pad(mirror_bed_slopes(m), N) for _, _, m in trap])
    members = [(i, fx["initial_conditions"]) for i, fx, _ in trap]
    with table_batch(probs) as b:
        assert (b.B * b.N) % 256 != 0
        info = b.init_state("steady-state", [ic[0, 1] for _, ic in members], bed_slope=slopes)
        assert not info["flags"].any()
        h, Q = b.state()
    check_against(h, Q, members, "normal depth, per-reach tables")
    for walk in (False, True):
        if walk:
            monkeypatch.setenv("FS_POLY_WALK", "1")
        for i, fx, m in poly:
            p = O.problem_from_fixture(fx, m)
            with batch_from_problems([p], mode="irregular", history=False) as b:
                assert b.poly_tables() == (0 if walk else 1)
                b.set_state(np.full((1, p.N), POISON), np.full((1, p.N), POISON))
                info = b.init_state("steady-state", m["Qb"], bed_slope=mirror_bed_slopes(m))
                assert not info["flags"].any()
                h, Q = b.state()
            check_against(h, Q, [(i, fx["initial_conditions"])], f"normal depth, polyline case {i}, {'edge walk' if walk else 'stage tables'}")


# ---- 3. linear -----------------------------------------------------------------------------------------------------------------
def test_linear_matches_the_reference():
    cases = BY_IC["linear"]
    assert len(cases) == 38
    # (the method reads no section: the polyline channels among them run on their table rows)
    probs = [O.problem_from_fixture(fx, m) for _, fx, m in cases]
    with table_batch(probs) as b:
        info = b.init_state("linear", [m["Qb"] for _, _, m in cases], depth_us=[m["us_initial_depth"] for _, _, m in cases],
                            depth_ds=[m["ds_initial_depth"] for _, _, m in cases])
        assert not info["flags"].any()
        h, Q = b.state()
    for r, (i, fx, m) in enumerate(cases):
        ic = fx["initial_conditions"]
        np.testing.assert_allclose(h[r, :m["N"]], ic[:, 0], rtol=1e-13, atol=0, err_msg=str(i))
        assert np.array_equal(Q[r, :m["N"]], ic[:, 1])


# ---- 4. the ensemble form ------------------------------------------------------------------------------------------------------
def test_ensemble_members_start_from_their_own_backwater_profile():
    path = os.path.join(GOLDEN, "gerd_ensemble.npz")
    fx, meta = O.load_fixture(path)
    probs = [O.problem_from_fixture(fx, meta, k) for k in range(meta["B"])]
    assert probs[0].N == 121 and np.any(probs[0].geo["is_compound"] > 0.5)
    override = [float(p.geo["n_main"][0]) for p in probs]
    ics = fx["initial_conditions"]
    with batch_from_problems(probs, mode="table", n_main_override=override, history=False) as b:
        b.set_state(np.full((b.B, b.N), POISON), np.full((b.B, b.N), POISON))
        info = b.init_state("GVF_equation", ics[0, 0, 1], depth_ds=ics[0, -1, 0])
        assert not info["flags"].any()
        h, Q = b.state()
    assert np.ptp(h[:, 0]) > 1e-3          # the profiles do depend on n
    check_against(h, Q, [(k, ics[k]) for k in range(meta["B"])], "backwater, shared table with Manning override")


# ---- 5. polylines --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walk", [False, True], ids=["stage_tables", "edge_walk"])
def test_polyline_backwater_matches_the_reference(walk, monkeypatch):
    gold = np.load(os.path.join(GOLDEN, "init_state_polyline.npz"))
    poly = [c for c in CASES if c[2]["family"] == "polyline"]
    assert len(poly) == 12
    if walk:
        monkeypatch.setenv("FS_POLY_WALK", "1")
    probs = [O.problem_from_fixture(fx, m) for _, fx, m in poly]
    members = [(i, gold[f"c{i:02d}_initial_conditions"]) for i, _, _ in poly]
    with per_reach_polyline_batch(probs, history=False) as b:
        assert b.poly_tables() == (0 if walk else 1)
        b.set_reach_scheme(dx=[p.dx for p in probs])
        b.set_state(np.full((b.B, b.N), POISON), np.full((b.B, b.N), POISON))
        info = b.init_state("GVF_equation", [ic[0, 1] for _, ic in members], depth_ds=[ic[-1, 0] for _, ic in members])
        assert not info["flags"].any()
        h, Q = b.state()
    check_against(h, Q, members, f"backwater, polylines, {'edge walk' if walk else 'stage tables'}")


# ---- 6. the same batch as set_state --------------------------------------------------------------------------------------------
def first_case(ic, family, min_nt=4):
    return next(c for c in CASES if c[2]["ic"] == ic and c[2]["family"] == family and c[2]["nt"] >= min_nt and c[2]["ds_kind"] != "storage_curve")


@pytest.mark.parametrize("which", ["trapezoid", "polyline"])
def test_the_batch_is_where_set_state_would_leave_it(which):
    i, fx, m = first_case("GVF_equation", "trap") if which == "trapezoid" else first_case("steady-state", "polyline")
    p = O.problem_from_fixture(fx, m)
    mode = "table" if which == "trapezoid" else "irregular"
    ic = fx["initial_conditions"]
    with batch_from_problems([p], mode=mode, history=True) as b, batch_from_problems([p], mode=mode, history=True) as twin:
        b.step(1)                                        # a batch that has been somewhere: level counter, status, records
        if which == "trapezoid":
            b.init_state("GVF_equation", ic[0, 1], depth_ds=ic[-1, 0])
        else:
            b.init_state("steady-state", ic[0, 1], bed_slope=mirror_bed_slopes(m))
        assert b.level == 0
        twin.set_state(*b.state())
        for x in (b, twin):
            x.step(3)
        assert np.all(b.status() == 0) and np.array_equal(b.status(), twin.status())
        assert np.array_equal(b.hydrographs(0, 4), twin.hydrographs(0, 4))
        hb, Qb = b.history_arrays(0, 4)
        ht, Qt = twin.history_arrays(0, 4)
        assert np.array_equal(hb, ht) and np.array_equal(Qb, Qt)
        assert b.hydrographs(0, 1)[0, 0, 0] == hb[0, 0, 0] and b.hydrographs(0, 1)[0, 2, 0] == hb[0, 0, p.N - 1]
        for fb, ft in zip(b.state() + b.guess(), twin.state() + twin.guess()):
            assert np.array_equal(fb, ft)
        its = b.iterations(0, 4)
        assert np.array_equal(its, twin.iterations(0, 4))
    assert rel_err(hb[:, 0], fx["depth"][:4], 1e-3 * m["h_n"]) <= 1e-8 and rel_err(Qb[:, 0], fx["flow"][:4], 1e-3 * m["Qb"]) <= 1e-8
    assert np.array_equal(its[:, 0], fx["iters"][:4])


# ---- 7. shapes -----------------------------------------------------------------------------------------------------------------
def mirror_rect_profile(width, n, z_us, z_ds, N, dx, Q, h_ds, method="GVF_equation", h_us=None):
    from flowsim_amd.hydromodel import Boundary, Channel
    us = Boundary(condition='flow_hydrograph', bed_level=z_us, chainage=0, initial_depth=h_us)
    ds = Boundary(condition='fixed_depth', bed_level=z_ds, chainage=(N - 1) * dx, initial_depth=h_ds)
    ch = Channel(us, ds, Q, roughness=n, width=width, interpolation_method=method)
    ch.initialize_conditions(N)
    return ch.initial_conditions


def test_replicas_of_one_reach_are_bit_identical():
    i, fx, m = first_case("GVF_equation", "compound", min_nt=3)
    p = O.problem_from_fixture(fx, m)
    ic = fx["initial_conditions"]
    ref = None
    for B in (1, 63, 65, 130):
        with PreissmannBatch(B, p.N, 4, section_mode="table") as b:
            b.set_scheme(0.6, 60.0, p.dx)
            b.set_geometry_table(p.geo)
            b.init_state("GVF_equation", ic[0, 1], depth_ds=ic[-1, 0])
            h, Q = b.state()
        ref = h[0] if ref is None else ref
        assert np.all(h == ref[None]) and np.all(Q == ic[0, 1])
    assert worst(ref, ic[:, 0]) <= 1.0


def test_node_counts_around_the_tile_and_a_ragged_batch():
    geo = dict(width=30.0, n=0.03, z_us=2.0, dx=150.0, Q=60.0, h_ds=2.5)
    singles = {}
    for N in (2, 3, 63, 64, 65, 128, 129, 257):
        z_us = 2e-4 * (N - 1) * geo["dx"]
        with rect_batch([geo["width"]], [geo["n"]], [z_us], [0.0], [N], geo["dx"]) as b:
            info = b.init_state("GVF_equation", geo["Q"], depth_ds=geo["h_ds"])
            assert not info["flags"].any()
            h, Q = b.state()
        singles[N] = h[0]
        want = mirror_rect_profile(geo["width"], geo["n"], z_us, 0.0, N, geo["dx"], geo["Q"], geo["h_ds"])
        assert worst(h[0], want[:, 0]) <= 1.0 and np.all(Q == geo["Q"]), N
    nodes = [2, 257, 64, 65, 3, 129, 63, 128]
    with rect_batch([geo["width"]] * 8, [geo["n"]] * 8, [2e-4 * (n - 1) * geo["dx"] for n in nodes], [0.0] * 8, nodes, geo["dx"]) as b:
        b.init_state("GVF_equation", geo["Q"], depth_ds=geo["h_ds"])
        h, Q = b.state()
    for r, n in enumerate(nodes):
        assert np.array_equal(h[r, :n], singles[n]), n
        assert np.all(h[r, n:] == geo["h_ds"])
    # the per-node kernels on a batch whose B N is no multiple of their block
    with rect_batch([geo["width"]] * 7, [geo["n"]] * 7, [1.0] * 7, [0.0] * 7, [37] * 7, geo["dx"]) as b:
        assert (7 * 37) % 256 != 0
        b.init_state("linear", geo["Q"], depth_us=1.5, depth_ds=np.linspace(2.0, 3.0, 7))
        h, Q = b.state()
        for r, hd in enumerate(np.linspace(2.0, 3.0, 7)):
            want = mirror_rect_profile(geo["width"], geo["n"], 1.0, 0.0, 37, geo["dx"], geo["Q"], hd, "linear", 1.5)
            np.testing.assert_allclose(h[r], want[:, 0], rtol=1e-13)
        b.init_state("steady-state", geo["Q"])               # bed_slope None: (z_us - z_ds) / ((n - 1) dx), channel.py:286
        h, Q = b.state()
        want = mirror_rect_profile(geo["width"], geo["n"], 1.0, 0.0, 37, geo["dx"], geo["Q"], 2.0, "steady-state")
        assert worst(h, np.broadcast_to(want[:, 0], h.shape)) <= 1.0 and np.all(Q == geo["Q"])


# ---- 8. flags ------------------------------------------------------------------------------------------------------------------
def test_a_supercritical_reach_is_flagged_and_leaves_its_neighbours_alone():
    import re
    N, dx, Q, h_ds = 17, 50.0, 50.0, 3.0
    steep = dict(width=10.0, n=0.03, z_us=0.02 * (N - 1) * dx)
    mild = dict(width=10.0, n=0.03, z_us=2e-4 * (N - 1) * dx)
    with pytest.raises(RuntimeError, match="GVF Error: Flow became supercritical") as e:
        mirror_rect_profile(steep["width"], steep["n"], steep["z_us"], 0.0, N, dx, Q, h_ds)
    node = int(re.search(r"at node (\d+)", str(e.value)).group(1))
    assert 0 < node < N - 1
    three = [mild, steep, mild]
    with rect_batch([g["width"] for g in three], [g["n"] for g in three], [g["z_us"] for g in three], [0.0] * 3, [N] * 3, dx) as b, \
            rect_batch([mild["width"]] * 2, [mild["n"]] * 2, [mild["z_us"]] * 2, [0.0] * 2, [N] * 2, dx) as clean:
        info = b.init_state("GVF_equation", Q, depth_ds=[h_ds, h_ds, h_ds + 0.5], strict=False)
        assert info["flags"].tolist() == [0, A.IC_SUPERCRITICAL, 0] and info["node"].tolist() == [-1, node, -1]
        h, _ = b.state()
        clean.init_state("GVF_equation", Q, depth_ds=[h_ds, h_ds + 0.5])
        hc, _ = clean.state()
        assert np.array_equal(h[[0, 2]], hc) and np.all(np.isfinite(hc))
        # the reach keeps what it marched and NaN where it did not get to
        reached = np.isfinite(h[1])
        assert reached[-1] and not reached[0] and np.all(np.diff(reached.astype(int)) >= 0)
        assert int(np.max(np.flatnonzero(~reached))) in (node, node - 1)      # stopped in the corrector at `node`, or in the predictor one above
        with pytest.raises(RuntimeError, match=rf"GVF Error: Flow became supercritical .* at node {node}\b"):
            b.init_state("GVF_equation", Q, depth_ds=[h_ds, h_ds, h_ds + 0.5])


def test_normal_depth_fallbacks_and_refusals():
    N, dx = 9, 100.0
    with rect_batch([20.0] * 3, [0.03] * 3, [0.0, 0.4, 0.4], [0.4, 0.0, 0.0], [N] * 3, dx) as b:
        # reach 0 rises downstream (S < 0): normal_flow is 0, brentq refuses the bracket, (z_min + 100) - z_min comes back
        info = b.init_state("steady-state", [40.0, 40.0, -1.0])
        h, Q = b.state()
        w = np.arange(N) * (1.0 / (N - 1))
        z_up, z_down = 0.4 * w, 0.4 * (1.0 - w)              # the beds of reach 0 and of reaches 1, 2
        assert np.array_equal(h[0], (z_up + 100.0) - z_up) and np.all(h[2] == 0.0) and np.all(Q[2] == -1.0)
        assert info["flags"].tolist() == [A.IC_NO_ROOT, 0, A.IC_NO_ROOT]
        want = mirror_rect_profile(20.0, 0.03, 0.4, 0.0, N, dx, 40.0, 1.0, "steady-state")
        assert worst(h[1], want[:, 0]) <= 1.0
        slope = np.full(N, 5e-4)
        slope[3] = np.nan
        with pytest.raises(A.FlowsimError, match="Bed slope must be defined"):
            b.init_state("steady-state", 40.0, bed_slope=slope)
        slope[3] = 0.0
        b.init_state("steady-state", 40.0, bed_slope=slope)
        h, _ = b.state()
        assert h[0, 3] == (z_up[3] + 100.0) - z_up[3] and np.all(h[1:, 3] == (z_down[3] + 100.0) - z_down[3]) and np.all(h[:, 4] < 10.0)
    with PreissmannBatch(2, 9, 4, section_mode="table") as b:
        with pytest.raises(A.FlowsimError, match="scheme.*geometry"):
            b.init_state("linear", 1.0, depth_us=1.0, depth_ds=1.0)
        b.set_scheme(0.6, 60.0, 100.0)
        with pytest.raises(A.FlowsimError, match="geometry"):
            b.init_state("linear", 1.0, depth_us=1.0, depth_ds=1.0)


# ---- 9. fp32 -------------------------------------------------------------------------------------------------------------------
def test_fp32_holds_the_library_claim():
    """include/flowsim_abi.h: an fp32 batch holds 5e-4 of the fp64 answer"""
    from flowsim_amd.synthetic import c5_reach_parameters, normal_depth_trap
    B, N, dx = 64, 33, 200.0
    width, m_side, n, S0, Q = c5_reach_parameters(0, B)
    z_us = S0 * (N - 1) * dx
    h_ds = 1.25 * normal_depth_trap(width, m_side, n, S0, Q)         # a backwater curve behind a raised downstream level
    out = {}
    for dtype in ("f64", "f32"):
        with rect_batch(width, n, z_us, np.zeros(B), [N] * B, dx, dtype=dtype, mode="trap_uniform", side_slope=m_side) as b:
            for method, kw in (("GVF_equation", dict(depth_ds=h_ds)), ("steady-state", {}), ("linear", dict(depth_us=1.0, depth_ds=h_ds))):
                info = b.init_state(method, Q, **kw)
                assert not info["flags"].any()
                out[dtype, method] = b.state()[0]
    for method in ("GVF_equation", "steady-state", "linear"):
        err = float(np.max(np.abs(out["f32", method] - out["f64", method]) / np.abs(out["f64", method])))
        print(f"fp32 against fp64, {method}: {err:.3g}")
        assert err <= 5e-4, (method, err)


# ---- 10. end to end ------------------------------------------------------------------------------------------------------------
def test_calibration_curve_with_device_initial_conditions():
    from cases.gerd_roseires.n_calibrate import rmse_curve
    fx = np.load(os.path.join(GOLDEN, "rmse_curve.npz"))
    got = np.array(rmse_curve(fx["n_values"], device_ic=True))
    np.testing.assert_allclose(got, fx["rmse"], rtol=1e-8, atol=0)
