"""fs_batch_assimilate on the device (PreissmannBatch.assimilate): the analysis step of the ensemble Kalman filter, held bit for bit
to the sequential restatement of tests/assim_checks.py - the gathered gauge values are read back from the device (the row
fs_batch_gauges(b, -1, 1) fills), everything after them is restated: coefficients, chunked moments, update.  States come from
set_state with random positive depths and flows, so no test needs a long run; the twin experiment at the end is the one that steps."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
import assim_checks as K
from failure_recipes import K_STAR
from fixture_batch import batch_from_problems
from flowsim_amd import _abi as A
from flowsim_amd import assimilation as DA
from flowsim_amd.batch import BoundarySpec, PreissmannBatch
from oracle import preissmann_oracle as O
from synth import rect_problem

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
NP_DTYPE = {"f64": np.float64, "f32": np.float32}
SIGNAL_VARIANCE = (0.01, 4.0, 0.01, 0.0025)              # depth, flow, stage, velocity


def rect_members(B, N, dtype="f64", steps=5, history=False, bad=(), manning=None, width=None, seed=901, dt=600.0):
    """RECT_UNIFORM batch of B members of ONE channel (N nodes) that differ in width and Manning n, an inflow hydrograph upstream and
    normal depth downstream (manning, width [B]: the members' own instead); bad: the members whose target is NaN at K_STAR.  Returns
    (batch, problem); no state yet."""
    p = rect_problem(N, seed=seed, n_steps=steps, dt=dt)
    rng = np.random.default_rng(77)
    width = p.geo["b_main"][0] * rng.uniform(0.9, 1.1, B) if width is None else np.asarray(width, dtype=np.float64)
    manning = p.geo["n_main"][0] * rng.uniform(0.9, 1.1, B) if manning is None else np.asarray(manning, dtype=np.float64)
    b = PreissmannBatch(B, N, p.nt, dtype=dtype, section_mode="rect_uniform", history=history)
    b.set_scheme(p.theta, p.dt, p.dx, 1e-3 if dtype == "f32" else p.tol, p.max_iter)
    b.set_geometry_uniform(width, manning, [p.geo["z_bed"][0]] * B, [p.geo["z_bed"][-1]] * B)
    target = np.repeat(p.us.target[:, None], B, axis=1)
    target[K_STAR, list(bad)] = NAN
    b.set_boundary(A.UPSTREAM, BoundarySpec(A.BC_FLOW_HYDROGRAPH, {}, target))
    b.set_boundary(A.DOWNSTREAM, BoundarySpec(A.BC_NORMAL_DEPTH, dict(bed_slope=np.full(B, p.ds.bed_slope), bed_level=np.zeros(B))))
    return b, p


def fixture_members(name, mode, dtype, B):
    fx, meta = O.load_fixture(os.path.join(GOLDEN, name + ".npz"))
    p = O.problem_from_fixture(fx, meta)
    return batch_from_problems([p] * B, mode=mode, dtype=dtype, history=False, n_main_override=p.geo["n_main"][0] * np.linspace(0.9, 1.1, B)), p


def random_state(B, N, seed, h0=2.5, Q0=60.0):
    """an ensemble with structure: a member-wide offset that every node shares, and noise on top; depths and flows positive"""
    rng = np.random.default_rng(seed)
    h = h0 + 0.3 * rng.standard_normal((B, 1)) + 0.05 * rng.standard_normal((B, N))
    Q = Q0 + 5.0 * rng.standard_normal((B, 1)) + 0.5 * rng.standard_normal((B, N))
    return np.maximum(h, 0.2), np.maximum(Q, 1.0)


def four_gauges(N):
    """node 0; the last node; between the last two; an interior node at a quarter of the way (on the node itself where it is the last)"""
    mid = N // 2
    return np.array([0, N - 1, N - 2, mid], dtype=np.int32), np.array([0.0, 0.0, 0.5, 0.25 if mid + 1 < N else 0.0])


def observations_of(b, m, seed):
    """m observations that mix the four gauges and the four signals (all sixteen pairs at m = 16), each a little off the ensemble
    mean of the current state; returns (observations, y [m, B]: the gathered values, as the call itself will gather them)"""
    b.gauges(current=True)
    rows = [b.gauge_rows(g, b.level, 1)[0] for g in range(4)]
    rng = np.random.default_rng(seed)
    obs, y = [], []
    for k in range(m):
        g, s = k % 4, (k // 4 + k) % 4
        y.append(rows[g][s])
        spread = np.sqrt(SIGNAL_VARIANCE[s])
        obs.append(DA.Observation(g, A.GAUGE_ROWS[s], float(np.nanmean(rows[g][s]) + spread * rng.normal()), SIGNAL_VARIANCE[s]))
    return obs, np.array(y)


def snapshot(b):
    (hk, Qk), (hg, Qg) = b.state(), b.guess()
    return hk, Qk, hg, Qg


def restated(b, obs, y, perturb=None, taper=None, floor=1e-3, dtype="f64"):
    """the restatement on the batch's current state; a member is active when it holds every observed gauge (a NaN row: mark bit 0)"""
    hk, Qk, hg, Qg = snapshot(b)
    active = ~np.any(np.isnan(y), axis=0)
    tap = None if taper is None else np.broadcast_to(np.asarray(taper, dtype=np.float64), (len(obs), hk.shape[1]))
    return K.analysis(y, active, hk, Qk, hg, Qg, [o.value for o in obs], [o.variance for o in obs], perturb, tap, floor, NP_DTYPE[dtype])


def assert_the_call_is(got, b, want, what):
    hk, Qk, hg, Qg = snapshot(b)
    assert got["n_active"] == want["n_active"], what
    prior = np.stack([got["prior"][k] for k in ("mean_h", "var_h", "mean_Q", "var_Q")])
    for name, g, w in (("prior", prior, want["prior"]), ("cross_cov", got["cross_cov"], want["cross_cov"]), ("hk", hk, want["hk"]), ("Qk", Qk, want["Qk"]),
                       ("hg", hg, want["hg"]), ("Qg", Qg, want["Qg"])):
        assert K.same(g, w), (what, name, float(np.nanmax(np.abs(np.asarray(g) - w))))
    assert np.array_equal(got["clamped"], want["clamped"]), what


# ---- 1. bit for bit against the restatement -------------------------------------------------------------------------------------------
# B below, at and across a chunk boundary and over three chunks with a ragged last one; N of one lane, a few, odd, and more than one
# block of 256 nodes (300, 4 096); m in every bucket's way: 1 alone, 3 padded to 4, 16 full
SHAPES = [("f64", 2, 2, 1), ("f64", 3, 5, 3), ("f64", 130, 121, 3), ("f64", 256, 5, 16), ("f64", 257, 121, 1), ("f64", 600, 300, 16), ("f64", 600, 2, 3),
          ("f64", 3, 4096, 3), ("f64", 2, 300, 16), ("f32", 2, 2, 3), ("f32", 130, 121, 16), ("f32", 257, 5, 3), ("f32", 600, 300, 1), ("f32", 256, 121, 3),
          ("f32", 3, 5, 16)]


@pytest.mark.parametrize("dtype,B,N,m", SHAPES)
def test_the_analysis_is_the_restatement_bit_for_bit(dtype, B, N, m):
    b, _ = rect_members(B, N, dtype)
    with b:
        b.set_state(*random_state(B, N, seed=B * 7 + N))
        b.set_gauges(node=four_gauges(N)[0], weight=four_gauges(N)[1])
        obs, y = observations_of(b, m, seed=m)
        perturb = DA.perturbations(3, [o.variance for o in obs], B)
        taper = np.random.default_rng(4).uniform(0.0, 1.0, (m, N))
        want = restated(b, obs, y, perturb, taper, dtype=dtype)
        got = b.assimilate(obs, perturb, taper)
        assert b.last_step_ms() >= 0.0
        assert_the_call_is(got, b, want, (dtype, B, N, m))
        assert got["n_active"] == B and np.max(np.abs(want["Z"])) > 0.0


@pytest.mark.parametrize("mode,name,dtype,m", [("table", "bc_compound_normal", "f64", 3), ("table", "bc_compound_normal", "f32", 16),
                                               ("irregular", "irr_mixed", "f64", 16)])
def test_tables_and_polylines_are_the_restatement_bit_for_bit(mode, name, dtype, m):
    """stage and velocity go through the section tables and the polylines here: the gather is fs_batch_gauges' own"""
    B = 130
    b, p = fixture_members(name, mode, dtype, B)
    with b:
        rng = np.random.default_rng(9)
        h = p.h0[None, :] * (1.0 + 0.1 * rng.standard_normal((B, 1)) + 0.01 * rng.standard_normal((B, p.N)))
        Q = p.Q0[None, :] * (1.0 + 0.1 * rng.standard_normal((B, 1)) + 0.01 * rng.standard_normal((B, p.N)))
        b.set_state(h, Q)
        node, weight = four_gauges(p.N)
        b.set_gauges(node=node, weight=weight)
        obs, y = observations_of(b, m, seed=m)
        assert not np.any(np.isnan(y))
        perturb = DA.perturbations(5, [o.variance for o in obs], B)
        want = restated(b, obs, y, perturb, None, dtype=dtype)
        got = b.assimilate(obs, perturb)
        assert_the_call_is(got, b, want, (mode, dtype, m))
        assert got["n_active"] == B


# ---- 2. inactive members --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_failed_member_is_inactive_and_keeps_every_bit(dtype):
    B, N = 5, 33
    b, _ = rect_members(B, N, dtype, history=True, bad=(1,))
    with b:
        h0, Q0 = random_state(B, N, seed=2, h0=2.0, Q0=40.0)
        b.set_state(np.repeat(h0[:, :1], N, axis=1), np.repeat(Q0[:, :1], N, axis=1))       # a uniform depth and flow per member: it steps
        b.step(3)
        assert b.status().tolist() == [A.OK, A.NAN, A.OK, A.OK, A.OK]
        b.set_gauges(node=four_gauges(N)[0], weight=four_gauges(N)[1])
        obs, y = observations_of(b, 3, seed=1)
        assert np.all(np.isnan(y[:, 1])) and not np.any(np.isnan(np.delete(y, 1, axis=1)))
        before = snapshot(b)
        perturb = DA.perturbations(6, [o.variance for o in obs], B, active=np.arange(B) != 1)
        want = restated(b, obs, y, perturb, dtype=dtype)
        got = b.assimilate(obs, perturb)
        after = snapshot(b)
        assert got["n_active"] == B - 1
        for x0, x1 in zip(before, after):
            assert K.same(x0[1], x1[1]) and not np.array_equal(x0[0], x1[0])
        assert_the_call_is(got, b, want, dtype)                                              # the others: the restatement without it
        alone = K.analysis(np.delete(y, 1, axis=1), np.ones(B - 1, dtype=bool), *[np.delete(x, 1, axis=0) for x in before], [o.value for o in obs],
                           [o.variance for o in obs], np.delete(perturb, 1, axis=1), None, 1e-3, NP_DTYPE[dtype])
        assert K.same(alone["hk"], np.delete(after[0], 1, axis=0)) and K.same(alone["Qg"], np.delete(after[3], 1, axis=0))


# ---- 3. taper -------------------------------------------------------------------------------------------------------------------------
def test_a_taper_of_zero_keeps_its_nodes_and_a_taper_of_ones_is_no_taper():
    B, N, m = 130, 33, 3
    results = {}
    for which in ("zeros_on_10_19", "ones", "none"):
        b, _ = rect_members(B, N)
        with b:
            b.set_state(*random_state(B, N, seed=8))
            b.set_gauges(node=four_gauges(N)[0], weight=four_gauges(N)[1])
            obs, y = observations_of(b, m, seed=2)
            taper = None if which == "none" else np.ones((m, N))
            if which == "zeros_on_10_19":
                taper[:, 10:20] = 0.0
            before = snapshot(b)
            got = b.assimilate(obs, None, taper)
            results[which] = (before, snapshot(b), got)
    before, after, _ = results["zeros_on_10_19"]
    for x0, x1 in zip(before, after):
        assert K.same(x0[:, 10:20], x1[:, 10:20])                                            # every member, bit for bit
        assert np.all(np.any(x0[:, :10] != x1[:, :10], axis=1)) and np.all(np.any(x0[:, 20:] != x1[:, 20:], axis=1))
    for x1, x2 in zip(results["ones"][1], results["none"][1]):
        assert K.same(x1, x2)
    assert K.same(results["ones"][2]["cross_cov"], results["none"][2]["cross_cov"]) and K.same(results["ones"][2]["cross_cov"], results["zeros_on_10_19"][2]["cross_cov"])


# ---- 4. depth floor -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_depths_end_on_the_floor_not_below_it(dtype):
    B, N, floor = 130, 33, 0.05
    b, _ = rect_members(B, N, dtype)
    with b:
        b.set_state(*random_state(B, N, seed=13, h0=1.0))
        b.set_gauges(node=four_gauges(N)[0], weight=four_gauges(N)[1])
        b.gauges(current=True)
        y = b.gauge_rows(3, 0, 1)[0][:1]
        obs = [DA.Observation(3, "depth", -2.0, 1e-8)]                                       # far below the ensemble, and trusted
        want = restated(b, obs, y, None, None, floor, dtype)
        got = b.assimilate(obs, depth_floor=floor)
        hk, Qk, hg, Qg = snapshot(b)
        low = want["hk"] == NP_DTYPE[dtype](floor)
        assert low.sum() > 0 and np.array_equal(got["clamped"], want["clamped"]) and np.array_equal(got["clamped"], low.sum(axis=1))
        assert np.all(hk[low] == NP_DTYPE[dtype](floor)) and np.all(hg[low] == NP_DTYPE[dtype](floor))
        assert hk.min() >= NP_DTYPE[dtype](floor) and hg.min() >= NP_DTYPE[dtype](floor)     # nobody ends below the floor
        assert_the_call_is(got, b, want, dtype)


# ---- 5. the scalar identity, through the whole path -----------------------------------------------------------------------------------
@pytest.mark.parametrize("B,weight", [(130, 0.0), (257, 0.25)])
def test_one_stage_observation_moves_the_mean_by_the_kalman_gain(B, weight):
    """posterior mean - observation = (prior mean - observation) r / (sigma^2 + r): the stage at a gauge is linear in the depths, so
    the identity is exact in real arithmetic.  The bar: the means are sums of B stages (B roundings of the stage's size each, here
    and in the call's own ybar), every member's new depth and stage round once more, sigma^2 carries (B + 2) roundings into a
    correction that is smaller than the stage: 4 (B + 16) 2^-52 max|stage| covers them with a factor two."""
    N, r = 33, 0.04
    b, _ = rect_members(B, N)
    with b:
        b.set_state(*random_state(B, N, seed=21))
        b.set_gauges(node=[N // 2], weight=[weight])
        b.gauges(current=True)
        prior = b.gauge_rows(0, 0, 1)[0][2]
        value = float(prior.mean() + 0.4)
        got = b.assimilate([DA.Observation(0, "stage", value, r)], depth_floor=0.0)
        assert got["n_active"] == B and not np.any(got["clamped"])
        b.gauges(current=True)
        post = b.gauge_rows(0, 0, 1)[0][2]
        sigma2 = prior.var(ddof=1)
        want = (prior.mean() - value) * r / (sigma2 + r)
        bar = 4 * (B + 16) * K.EPS * np.max(np.abs(prior))
        err = abs((post.mean() - value) - want)
        print(f"B {B} weight {weight}: prior distance {prior.mean() - value:.6g}, posterior {post.mean() - value:.6g}, identity {want:.6g}, off by {err:.3g}, bar {bar:.3g}")
        assert err <= bar, (err, bar)
        assert abs(post.mean() - value) < abs(prior.mean() - value)


# ---- 6. what is left alone ------------------------------------------------------------------------------------------------------------
def test_the_records_of_the_forecast_stay_and_the_batch_steps_on():
    B, N = 65, 33
    b, _ = rect_members(B, N, history=True)
    with b:
        h0, Q0 = random_state(B, N, seed=5, h0=2.0, Q0=40.0)
        b.set_state(np.repeat(h0[:, :1], N, axis=1), np.repeat(Q0[:, :1], N, axis=1))
        b.step(3)
        b.set_gauges(node=four_gauges(N)[0], weight=four_gauges(N)[1])
        record = lambda: (b.hydrographs(), *b.history_arrays(), b.iterations(), b.status(), b.level)
        before = record()
        obs, y = observations_of(b, 3, seed=3)
        state0 = snapshot(b)
        got = b.assimilate(obs, DA.perturbations(1, [o.variance for o in obs], B))
        assert got["n_active"] == B and not np.array_equal(state0[0], snapshot(b)[0])
        for x0, x1 in zip(before, record()):
            assert K.same(x0, x1) if isinstance(x0, np.ndarray) else x0 == x1
        b.step(2)
        assert b.level == 5 and np.all(b.status() == A.OK), b.status()
        assert K.same(before[1][:4], b.history_arrays()[0][:4])                              # the history before the analysis is not rewritten


# ---- 7. every refusal -----------------------------------------------------------------------------------------------------------------
def raw_call(b, n_obs, gauge, signal, value, variance, perturb=None, taper=None, floor=1e-3):
    """fs_batch_assimilate itself, so that what _pack would refuse reaches the library; returns (rc, text)"""
    arr = lambda a, t: np.ascontiguousarray(a, dtype=t)
    g, s, v, var = arr(gauge, np.int32), arr(signal, np.int32), arr(value, np.float64), arr(variance, np.float64)
    p = None if perturb is None else arr(perturb, np.float64)
    t = None if taper is None else arr(taper, np.float64)
    ptr = lambda a, T: None if a is None else a.ctypes.data_as(T)
    n_active = C.c_int32(-1)
    rc = b._lib.fs_batch_assimilate(b._h, n_obs, ptr(g, A._I), ptr(s, A._I), ptr(v, A._D), ptr(var, A._D), ptr(p, A._D), ptr(t, A._D), float(floor),
                                    None, None, None, C.byref(n_active))
    return rc, A.last_error()


def refused(b, text, *args, **kw):
    before = snapshot(b) if kw.pop("has_state", True) else None
    rc, err = raw_call(b, *args, **kw)
    assert rc != 0 and "fs_batch_assimilate" in err and text in err, (text, rc, err)
    if before is not None:
        for x0, x1 in zip(before, snapshot(b)):
            assert K.same(x0, x1), text


def test_misuse_is_refused_with_a_text_that_names_the_entry_point_and_the_state_stays():
    B, N = 4, 5
    node, weight = four_gauges(N)
    one = (1, [0], [0], [2.0], [0.01])
    with rect_members(B, N)[0] as b:
        b.set_gauges(node=node, weight=weight)
        refused(b, "no state", *one, has_state=False)
    with PreissmannBatch(B, N, 4) as b:
        b.set_state(*random_state(B, N, 1))
        refused(b, "geometry", *one)
    with rect_members(B, N)[0] as b:
        b.set_state(*random_state(B, N, 1))
        refused(b, "no gauges", *one)
        b.set_gauges(node=np.tile(node, (B, 1)), weight=np.tile(weight, (B, 1)))
        refused(b, "per reach", *one)
        b.set_gauges(node=node, weight=weight)
        refused(b, "n_obs must be 1 .. 16, not 0", 0, [], [], [], [])
        refused(b, "n_obs must be 1 .. 16, not 17", 17, [0] * 17, [0] * 17, [1.0] * 17, [1.0] * 17)
        refused(b, "gauge 4 is not one of 0 .. 3", 1, [4], [0], [2.0], [0.01])
        refused(b, "gauge -1 is not one of 0 .. 3", 1, [-1], [0], [2.0], [0.01])
        refused(b, "signal 4 is not one of", 1, [0], [4], [2.0], [0.01])
        refused(b, "signal -1 is not one of", 1, [0], [-1], [2.0], [0.01])
        for bad in (0.0, -1.0, NAN, INF):
            refused(b, "variances must be finite and > 0", 1, [0], [0], [2.0], [bad])
        for bad in (NAN, INF, -INF):
            refused(b, "values must be finite", 1, [0], [0], [bad], [0.01])
            refused(b, "perturbations must be finite", *one, perturb=[0.0, bad, 0.0, 0.0])
            refused(b, "depth_floor must be finite and >= 0", *one, floor=bad)
        refused(b, "depth_floor must be finite and >= 0", *one, floor=-1e-6)
        for bad in (NAN, -1e-9, 1.0 + 2.0 ** -52, INF):
            refused(b, "tapers must be finite and in [0, 1]", *one, taper=[1.0, 1.0, bad, 1.0, 1.0])
        h, Q = random_state(B, N, 1)
        h[2, 0] = NAN
        b.set_state(h, Q)
        refused(b, "member 2 holds a NaN in observation 0", *one)
        h[:, 0] = [1.0, 3.0, 5.0, 3.0]                                                       # anomalies -2, 0, 2, 0: C = 8 / 3 + 1e-30 twice
        h[:, 1] = [1.0, 3.0, 5.0, 3.0]
        b.set_state(h, Q)
        refused(b, "not positive definite (pivot 1", 2, [0, 0], [0, 0], [2.0, 2.0], [1e-30, 1e-30])
        rc, err = raw_call(b, 2, [0, 0], [0, 1], [2.0, 50.0], [0.01, 4.0])
        assert rc == 0, err                                                                  # and after all that the batch still takes an analysis
    b, p = fixture_members("bc_compound_normal", "table", "f64", B)                      # (fs_batch_iterate steps table and polyline batches)
    with b:
        b.set_state(np.repeat(1.05 * p.h0[None, :], B, axis=0), np.repeat(p.Q0[None, :], B, axis=0))
        b.set_gauges(node=four_gauges(p.N)[0], weight=four_gauges(p.N)[1])
        assert b.iterate() > 0
        refused(b, "fs_batch_iterate", *one)
    with rect_members(B, N)[0] as b:
        b.set_reach_nodes([N, N, N - 1, N])
        b.set_state(*random_state(B, N, 1))
        b.set_gauges(node=node, weight=weight)
        refused(b, "per-reach node counts", *one)
    b, _ = rect_members(3, 33, history=True, bad=(0, 2))
    with b:
        b.set_state(np.full((3, 33), 2.0), np.full((3, 33), 40.0))
        b.step(3)
        assert b.status().tolist() == [A.NAN, A.OK, A.NAN]
        b.set_gauges(node=four_gauges(33)[0], weight=four_gauges(33)[1])
        refused(b, "1 active member(s)", *one)


# ---- 8. a small twin experiment -------------------------------------------------------------------------------------------------------
def test_a_twin_experiment_pulls_the_ensemble_to_the_truth_at_a_gauge_it_does_not_see():
    """64 members x 61 nodes whose Manning n is spread over 0.8 .. 1.6 of the truth's (the truth lies inside the spread, not at its
    centre, so every forecast drifts off again and every analysis has an error to remove), each started at its own normal depth, 40
    levels of half an hour (at 10 minutes the members drift back so little in 5 levels that the error left at the hidden gauge by
    two gauges 8 km apart, a few millimetres, is the size of the error to remove: the restatement then fails the condition on the
    CPU oracle's forecasts, at levels 10 and 15); every 5 levels the truth's
    stage at two gauges is assimilated with perturbations of a fixed seed, and at a third gauge between them, which no analysis
    sees, the ensemble-mean stage must be strictly closer to the truth after the call than before - first by the restatement on
    the device's forecast, then on the device."""
    B, N, steps, every, r, dt = 64, 61, 40, 5, 1e-4, 1800.0
    p = rect_problem(N, seed=901, n_steps=steps, dt=dt)
    n_true = p.geo["n_main"][0]
    manning = n_true * np.random.default_rng(31).uniform(0.8, 1.6, B)
    node, weight = np.array([12, 44, 29], dtype=np.int32), np.array([0.0, 0.5, 0.25])
    width = p.geo["b_main"][0]
    truth, _ = rect_members(1, N, steps=steps, manning=[n_true], width=[width], dt=dt)
    ens, _ = rect_members(B, N, steps=steps, manning=manning, width=[width] * B, dt=dt)
    ratios = []
    with truth, ens:
        truth.set_state(p.h0[None, :], p.Q0[None, :])
        ens.set_state(p.h0[None, :] * (manning[:, None] / n_true) ** 0.6, np.repeat(p.Q0[None, :], B, axis=0))      # (wide channel: h ~ n^(3/5))
        truth.set_gauges(node=node, weight=weight)
        ens.set_gauges(node=node, weight=weight)
        for level in range(every, steps + 1, every):
            truth.step(every); ens.step(every)
            assert truth.status()[0] == A.OK and np.all(ens.status() == A.OK), (level, ens.status())
            truth.gauges(current=True); ens.gauges(current=True)
            seen = [float(truth.gauge_rows(g, level, 1)[0][2, 0]) for g in (0, 1)]
            hidden = float(truth.gauge_rows(2, level, 1)[0][2, 0])
            obs = [DA.Observation(g, "stage", seen[g], r) for g in (0, 1)]
            perturb = DA.perturbations(1000 + level, [r, r], B, active=np.ones(B, dtype=bool))
            y = np.array([ens.gauge_rows(g, level, 1)[0][2] for g in (0, 1)])
            prior = float(np.mean(ens.gauge_rows(2, level, 1)[0][2]))
            want = restated(ens, obs, y, perturb, None, 1e-3)
            z = float(p.geo["z_bed"][29] + 0.25 * (p.geo["z_bed"][30] - p.geo["z_bed"][29]))
            by_numpy = float(np.mean(want["hk"][:, 29] + 0.25 * (want["hk"][:, 30] - want["hk"][:, 29]))) + z
            assert abs(by_numpy - hidden) < abs(prior - hidden), (level, prior - hidden, by_numpy - hidden)
            got = ens.assimilate(obs, perturb)
            assert got["n_active"] == B and not np.any(got["clamped"])
            ens.gauges(current=True)
            post = float(np.mean(ens.gauge_rows(2, level, 1)[0][2]))
            print(f"level {level}: mean stage - truth at the hidden gauge {prior - hidden:+.5f} -> {post - hidden:+.5f}  (restatement {by_numpy - hidden:+.5f})")
            assert abs(post - hidden) < abs(prior - hidden), (level, prior - hidden, post - hidden)
            ratios.append(abs(post - hidden) / abs(prior - hidden))
    print("improvement ratios |posterior| / |prior|:", " ".join(f"{v:.3f}" for v in ratios))
