"""Flood envelopes along the reach and their bands across the members (fs_batch_envelope, fs_batch_profile_bands;
flow-sim_amd/csrc/fs_envelope.hpp) on the device.

  1. against the reference's own histories and derived fields (tests/golden): extremes within the bound fs_batch_derive is held to,
     level indices and crossings exact wherever the fixture itself decides them with a margin;
  2. against fs_batch_derive on the same batch, bit for bit: fp64 and fp32, a ragged batch with an odd B N, a range that begins
     after level 0, a restarted batch;
  3. a reach driven to FS_MAX_ITER enters with the rows before its failing level and leaves its neighbours' bits alone;
  4. profile bands on the reference's 8-member GERD ensemble and on corner shapes, against numpy on the downloaded envelope;
  5. run_manning_ensemble(envelope=...) is a direct PreissmannBatch run, and without the keyword what it was."""
import copy
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN
from envelope_checks import STEPS, assert_envelope_is_numpy_on, check_profile, crossings_of, fields_of, ragged_batch
import failure_recipes as FR
from fixture_batch import batch_from_problems
from flowsim_amd import PreissmannBatch
from flowsim_amd import _abi as A
from kernel_harness import TOL, batch_for_entry, rel_err
from oracle import preissmann_oracle as O

pytestmark = pytest.mark.gpu

QUANTITIES = A.ENV_QUANTITIES
# the reference's array behind each quantity, the field of fs_batch_derive that holds it (None: the history itself), the floor of rel_err
FIXTURE_FIELD = dict(depth=("depth", None, 1e-3), stage=("derived_level", "level", 1e-6), flow=("flow", None, 1.0),
                     velocity=("derived_velocity", "velocity", 1e-6), froude_number=("derived_froude_number", "froude_number", 1e-6),
                     top_width=("derived_top_width", "top_width", 1e-6))


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the reference's own histories
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["akbari", "bc_compound_normal", "irr_levee", "irr_mixed"])
def test_envelopes_of_the_reference_histories(name):
    fx, meta = O.load_fixture(os.path.join(GOLDEN, name + ".npz"))
    p = O.problem_from_fixture(fx, meta)
    stage = fx["derived_level"]
    lo, hi = stage.min(axis=0), stage.max(axis=0)
    mid = 0.5 * (lo + hi)
    assert np.min(np.abs(stage - mid)) > 2e-3                      # no sample of the fixture sits on the threshold
    with batch_from_problems([p]) as b:
        b.step(p.nt - 1)
        assert b.status()[0] == 0
        env = b.envelope(QUANTITIES, threshold=mid)
        above = b.envelope(("stage",), threshold=hi + 1.0)
        below = b.envelope(("stage",), threshold=lo - 1.0)
        unassessed = b.envelope(("stage",), threshold=np.where(np.arange(p.N) % 2 == 0, np.nan, mid))
    assert env["levels"].tolist() == [p.nt]
    rectangular = name == "akbari"
    for q in QUANTITIES:
        ref, _, floor = FIXTURE_FIELD[q]
        x = fx[ref]
        srt = np.sort(x, axis=0)
        for stat, want, lvl, extreme, second in (("max", x.max(axis=0), np.argmax(x, axis=0), srt[-1], srt[-2]),
                                                 ("min", x.min(axis=0), np.argmin(x, axis=0), srt[0], srt[1])):
            got, got_level = env[q][stat][0], env[q][stat + "_level"][0]
            err = rel_err(got, want, floor)
            separated = np.abs(extreme - second) > 1e-7 * np.maximum(1.0, np.abs(extreme))
            left_out = int(np.sum(~separated))
            print(name, q, stat, "rel err", err, "nodes left out of the level comparison", left_out)
            assert err <= TOL, (q, stat)
            if q == "top_width" and rectangular:
                continue                                           # a constant series: every level is the extreme's
            # maxima: no node of these fixtures fails the separation; minima: at most one (flow: exactly one, but for the compound case)
            if stat == "max":
                assert left_out == 0, (q, stat)
            else:
                assert left_out == (1 if q == "flow" and name != "bc_compound_normal" else 0), (q, stat, left_out)
            assert np.array_equal(got_level[separated], lvl[separated]), (q, stat)
    for got, thr in ((env, mid), (above, hi + 1.0), (below, lo - 1.0)):
        first, last, count = crossings_of(stage, thr)
        c = got["crossing"]
        assert np.array_equal(c["first"][0], first) and np.array_equal(c["last"][0], last) and np.array_equal(c["count"][0], count)
    assert np.all(above["crossing"]["count"] == 0) and np.all(above["crossing"]["first"] == -1) and np.all(above["crossing"]["last"] == -1)
    assert np.all(below["crossing"]["count"] == p.nt) and np.all(below["crossing"]["first"] == 0) and np.all(below["crossing"]["last"] == p.nt - 1)
    even = np.arange(p.N) % 2 == 0                                 # NaN entries: not assessed
    c = unassessed["crossing"]
    assert np.all(c["count"][0, even] == 0) and np.all(c["first"][0, even] == -1) and np.all(c["last"][0, even] == -1)
    assert all(np.array_equal(c[k][0, ~even], env["crossing"][k][0, ~even]) for k in A.ENV_CROSS_ROWS)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the same batch's fs_batch_derive, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
RAGGED = (20, 63, 33)            # B N = 189: odd, so no thread's elements start on a 16-byte boundary at every level


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_envelope_is_numpy_over_the_derived_fields_of_a_ragged_batch(dtype):
    B, N = len(RAGGED), max(RAGGED)
    own = np.arange(N)[None, :] < np.array(RAGGED)[:, None]        # [B, N]: the nodes each reach has
    with ragged_batch(RAGGED, dtype) as b:
        b.step(STEPS)
        assert np.all(b.status() == 0) and (B * N) % 2 == 1
        for first, n in ((0, STEPS + 1), (2, 3), (STEPS, 1)):
            x = fields_of(b, first, n)
            thr = np.where(own, 0.5 * (x["stage"].min(axis=0) + x["stage"].max(axis=0)), 0.0)          # [B, N], on samples where n = 1
            env = b.envelope(QUANTITIES, threshold=thr, first=first, n=n)
            assert env["levels"].tolist() == [n] * B
            for q in QUANTITIES:
                assert_envelope_is_numpy_on(env, x[q], q, own, (dtype, first, n))
                # nodes beyond a reach's own count: values 0, levels -1
                assert np.all(env[q]["max"][~own] == 0) and np.all(env[q]["min"][~own] == 0)
                assert np.all(env[q]["max_level"][~own] == -1) and np.all(env[q]["min_level"][~own] == -1)
            t = thr.astype(np.float32).astype(np.float64) if dtype == "f32" else thr          # rounded once to the batch's type
            first_, last_, count_ = crossings_of(x["stage"], t)
            c = env["crossing"]
            assert np.array_equal(c["first"][own], first_[own]) and np.array_equal(c["last"][own], last_[own])
            assert np.array_equal(c["count"][own], count_[own])
            assert np.all(c["count"][~own] == 0) and np.all(c["first"][~own] == -1) and np.all(c["last"][~own] == -1)
            # the quantities that need no section run in an instantiation of their own (the stage alone never reads the flow)
            for names in (("depth", "stage", "flow"), ("stage",), ("flow",)):
                plain = b.envelope(names, threshold=thr, first=first, n=n)
                assert all(np.array_equal(plain[q][s], env[q][s]) for q in names for s in A.ENV_STATS), names
                assert all(np.array_equal(plain["crossing"][k], c[k]) for k in A.ENV_CROSS_ROWS), names
            # one quantity alone and the threshold on a quantity that is not selected: the same rows
            flow_thr = 0.5 * (x["flow"].min() + x["flow"].max())
            one = b.envelope("velocity", threshold=flow_thr, threshold_quantity="flow", first=first, n=n)
            assert sorted(one) == ["crossing", "levels", "velocity"]
            assert all(np.array_equal(one["velocity"][s], env["velocity"][s]) for s in A.ENV_STATS)
            ft = np.float64(np.float32(flow_thr)) if dtype == "f32" else flow_thr
            assert np.array_equal(one["crossing"]["count"][own], crossings_of(x["flow"], ft)[2][own])
        ms = b.last_step_ms()
        assert 0.0 < ms < 1000.0                                   # the envelope kernel's HIP-event time
        ptrs = b.envelope_device(("depth", "flow"), threshold=1.0)
        assert len(ptrs) == 2 * 4 + 3 and all(ptrs.values()) and len(set(ptrs.values())) == len(ptrs)
        assert b._lib.fs_batch_envelope_device_ptr(b._h, 11) is None and b._lib.fs_batch_envelope_device_ptr(b._h, -1) is None
        assert b.envelope_device(("depth",))[("depth", "max")] and b._lib.fs_batch_envelope_device_ptr(b._h, 4) is None


def test_envelope_after_a_restart():
    fx, meta = O.load_fixture(os.path.join(GOLDEN, "akbari.npz"))
    p = O.problem_from_fixture(fx, meta)
    K, more = 5, 4
    with batch_from_problems([p]) as b, batch_from_problems([p]) as c:
        b.step(K)
        (h, Q), (hg, Qg) = b.state(), b.guess()
        c.restart(K, h, Q, hg, Qg)
        b.step(more)
        c.step(more)
        with pytest.raises(A.FlowsimError, match=f"restarted at level {K}; the history before it was not restored"):
            c.envelope(QUANTITIES, first=0, n=K + more + 1)
        with pytest.raises(A.FlowsimError, match=f"restarted at level {K}"):
            c.envelope(("stage",), first=K - 1, n=2)
        got, want = c.envelope(QUANTITIES, first=K, n=more + 1), b.envelope(QUANTITIES, first=K, n=more + 1)
        x = fields_of(c, K, more + 1)
        for q in QUANTITIES:
            assert_envelope_is_numpy_on(got, x[q], q, None, "restarted")
            assert all(np.array_equal(got[q][s], want[q][s]) for s in A.ENV_STATS), q
        assert got["levels"].tolist() == [more + 1] and got["crossing"] is None


def test_argument_errors_leave_the_batch_usable():
    fx, meta = O.load_fixture(os.path.join(GOLDEN, "akbari.npz"))
    p = O.problem_from_fixture(fx, meta)
    p.nt = 4
    with batch_from_problems([p], history=False) as b:
        b.step(3)
        with pytest.raises(A.FlowsimError, match="fs_batch_envelope: batch was created without FS_FLAG_HISTORY"):
            b.envelope()
    with batch_from_problems([p]) as b:
        b.step(2)
        with pytest.raises(ValueError, match="holds no envelope"):
            b.profile_bands("stage")
        lib, h = b._lib, b._h
        mom = np.empty((p.N, 4))
        D = lambda a: a.ctypes.data_as(A._D)
        assert lib.fs_batch_profile_bands(h, 2, 0, None, 0, D(mom), None, None, None) == -1 and "holds no envelope" in A.last_error()
        with pytest.raises(A.FlowsimError, match=r"levels \[0, 4\) are not inside 0 .. 2"):
            b.envelope(n=4)
        with pytest.raises(A.FlowsimError, match="levels"):
            b.envelope(first=-1, n=1)
        assert lib.fs_batch_envelope_device(h, 0, 3, 0, None, 0, 2) == -1 and "quantities" in A.last_error()
        assert lib.fs_batch_envelope_device(h, 0, 3, 128, None, 0, 2) == -1 and "quantities" in A.last_error()
        thr = np.zeros(p.N)
        assert lib.fs_batch_envelope_device(h, 0, 3, 2, D(thr), 0, 3) == -1 and "threshold_quantity" in A.last_error()
        out = np.empty((1, 4, 1, p.N))
        assert lib.fs_batch_envelope(h, 0, 3, 2, None, 0, 2, D(out), D(out), None) == -1 and "need a threshold" in A.last_error()
        env = b.envelope(("stage",))
        x = fields_of(b, 0, 3)
        assert_envelope_is_numpy_on(env, x["stage"], "stage")
        with pytest.raises(ValueError, match="does not hold 'depth'"):
            b.profile_bands("depth")
        assert lib.fs_batch_profile_bands(h, 1, 0, None, 0, D(mom), None, None, None) == -1 and "no such row" in A.last_error()
        assert lib.fs_batch_profile_bands(h, 2, 4, None, 0, D(mom), None, None, None) == -1 and "no such row" in A.last_error()
        assert lib.fs_batch_profile_bands(h, A.ENV_CROSSING, 2, None, 0, D(mom), None, None, None) == -1 and "no such row" in A.last_error()
        assert lib.fs_batch_profile_bands(h, 2, 0, None, 0, D(mom), None, D(thr), None) == -1 and "exceed needs" in A.last_error()
        assert lib.fs_batch_profile_bands(h, 2, 0, None, 0, None, None, None, None) == -1 and "no output" in A.last_error()
        assert lib.fs_batch_profile_bands(h, 2, 0, None, 17, D(mom), None, None, None) == -1 and "n_q" in A.last_error()
        got = b.profile_bands("stage")
        assert got["exceed"] is None and np.array_equal(got["max"], env["stage"]["max"][0]) and np.all(got["n_members"] == 1)
        b.step(1)                                                  # the batch goes on
        assert b.status()[0] == 0 and b.envelope(("stage",))["levels"].tolist() == [4]


# ---------------------------------------------------------------------------------------------------------------------------
# 3. a failed reach
# ---------------------------------------------------------------------------------------------------------------------------
def scaled(p, factor):
    """the same reach with another hydrograph (so that the two good reaches of a batch differ)"""
    side = FR.target_side(p)
    q = FR.edited(p, 0, float(getattr(p, side).target[0]))
    t = getattr(q, side).target
    t[1:] = t[0] + factor * (t[1:] - t[0])
    return q


def test_a_reach_that_ran_out_of_iterations_enters_with_the_rows_before_its_failing_level(monkeypatch):
    e = FR._plain("f64", A.SEC_RECT_UNIFORM, 2, 1, 0, full=0)
    good, bad, mode, override = FR.maxiter_case(e)
    other = scaled(good, 1.1)
    nt, K = good.nt, FR.K_STAR
    monkeypatch.setenv("FS_KERNEL_INDEX", str(e["index"]))
    with batch_for_entry([good, other], e, mode, override, history=True) as b:
        b.set_reach_tolerance(None, [100, 100])
        b.step(nt - 1)
        assert np.all(b.status() == 0)
        stage = fields_of(b, 0, nt)["stage"]
        thr = 0.5 * (stage[:, 0].min(axis=0) + stage[:, 0].max(axis=0))          # [N], shared by the reaches of both batches
        alone = b.envelope(QUANTITIES, threshold=thr)
    with batch_for_entry([good, bad, other], e, mode, override, history=True) as b:
        b.set_reach_tolerance(None, [100, bad.max_iter, 100])
        b.step(nt - 1)
        assert b.status().tolist() == [A.OK, A.MAX_ITER, A.OK]
        env = b.envelope(QUANTITIES, threshold=thr)
        assert env["levels"].tolist() == [nt, K, nt]
        x = fields_of(b, 0, K)                                     # the rows before the failing level
        for q in QUANTITIES:
            sub = {q: {s: env[q][s][1:2] for s in A.ENV_STATS}}
            assert_envelope_is_numpy_on(sub, x[q][:, 1:2], q, None, "failed reach")
            for s in A.ENV_STATS:                                  # the other reaches: the bits of the batch without the failing one
                assert np.array_equal(env[q][s][[0, 2]], alone[q][s]), (q, s)
        first, last, count = crossings_of(x["stage"][:, 1], thr)
        c = env["crossing"]
        assert np.array_equal(c["first"][1], first) and np.array_equal(c["last"][1], last) and np.array_equal(c["count"][1], count)
        assert all(np.array_equal(c[k][[0, 2]], alone["crossing"][k]) for k in A.ENV_CROSS_ROWS)
        # ranges that leave the failed reach one row, and none
        part = b.envelope(("depth",), first=K - 1, n=3)
        assert part["levels"].tolist() == [3, 1, 3]
        assert np.array_equal(part["depth"]["max"][1], x["depth"][K - 1, 1]) and np.all(part["depth"]["max_level"][1] == 0)
        none = b.envelope(("depth",), threshold=0.0, first=K, n=2)
        assert none["levels"].tolist() == [2, 0, 2]
        assert np.all(np.isnan(none["depth"]["max"][1])) and np.all(np.isnan(none["depth"]["min"][1]))
        assert np.all(none["depth"]["max_level"][1] == -1) and np.all(none["depth"]["min_level"][1] == -1)
        assert np.all(none["crossing"]["count"][1] == 0) and np.all(none["crossing"]["first"][1] == -1)
        # across the members the failed one is left out
        b.envelope(("depth",), threshold=0.0, threshold_quantity="depth")
        pb = b.profile_bands("depth", "max", ())
        assert np.all(pb["n_members"] == 2) and np.all(pb["exceed"] == 1.0)
        assert np.array_equal(pb["max"], np.maximum(alone["depth"]["max"][0], alone["depth"]["max"][1]))


# ---------------------------------------------------------------------------------------------------------------------------
# 4. profile bands
# ---------------------------------------------------------------------------------------------------------------------------
def test_profile_bands_of_the_reference_ensemble():
    fx, meta = O.load_fixture(os.path.join(GOLDEN, "gerd_ensemble.npz"))
    B, nt, N = meta["B"], meta["nt"], meta["N"]
    probs = [O.problem_from_fixture(fx, meta, m) for m in range(B)]
    peak_depth = fx["depth"].max(axis=1)                           # [B, N]
    peak_stage = peak_depth + fx["geo_z_bed"][None, :]
    thr = np.median(peak_stage, axis=0)                            # at every node about half the members reach it
    with batch_from_problems(probs, mode="table", n_main_override=[float(p.geo["n_main"][0]) for p in probs]) as b:
        b.step(nt - 1)
        assert np.all(b.status() == 0)
        env = b.envelope(("depth", "stage"), threshold=thr)
        assert rel_err(env["depth"]["max"], peak_depth, 1e-3) <= TOL
        assert rel_err(env["stage"]["max"], peak_stage, 1e-3) <= TOL
        enters = np.ones((B, N), dtype=bool)
        counts = env["crossing"]["count"]
        got = check_profile(b, env["stage"]["max"], enters, "stage", "max", counts)
        assert 0.0 < np.min(got["exceed"]) and np.max(got["exceed"]) < 1.0 and np.all(got["n_members"] == B)
        check_profile(b, env["depth"]["max"], enters, "depth", "max", counts)
        check_profile(b, env["depth"]["min"], enters, "depth", "min", counts)
        check_profile(b, env["stage"]["max_level"], enters, "stage", "max_level", counts)          # rows of many ties
        check_profile(b, counts, enters, "crossing", "count", counts)
        check_profile(b, env["crossing"]["first"], enters, "crossing", "first", counts)


NT = 6


def akbari_members(B, dtype="f64"):
    """B copies of the rectangular akbari reach that differ in width and Manning n (+-10 %, fixed seed); the last repeats the first"""
    fx, meta = O.load_fixture(os.path.join(GOLDEN, "akbari.npz"))
    base = O.problem_from_fixture(fx, meta)
    base.nt = NT
    if dtype == "f32":
        base.tol = 1e-3
    rng = np.random.default_rng(20261020)
    out = []
    for r in range(B):
        p = copy.deepcopy(base)
        if r > 0:
            p.geo["b_main"] = p.geo["b_main"] * (1.0 + 0.1 * rng.uniform(-1, 1))
            p.geo["n_main"] = p.geo["n_main"] * (1.0 + 0.1 * rng.uniform(-1, 1))
        out.append(p)
    if B > 1:
        out[-1] = copy.deepcopy(out[0])
    return out


@pytest.mark.parametrize("B,dtype", [(1, "f64"), (2, "f64"), (257, "f64"), (300, "f64"), (257, "f32")])
def test_profile_bands_corner_shapes(B, dtype):
    probs = akbari_members(B, dtype)
    N = probs[0].N
    with batch_from_problems(probs, mode="rect_uniform", dtype=dtype) as b:
        b.step(NT - 1)
        assert np.all(b.status() == 0)
        env = b.envelope(("stage", "flow"), threshold=np.float64(np.median(fields_of(b, 0, NT)["stage"].max(axis=0))))
        enters = np.ones((B, N), dtype=bool)
        counts = env["crossing"]["count"]
        if B > 1:                                                  # the tied members
            assert np.array_equal(env["stage"]["max"][0], env["stage"]["max"][-1])
        check_profile(b, env["stage"]["max"], enters, "stage", "max", counts)
        check_profile(b, env["flow"]["min"], enters, "flow", "min", counts)
        check_profile(b, env["flow"]["max_level"], enters, "flow", "max_level", counts)
        sixteen = b.profile_bands("stage", "max", np.linspace(0.0, 1.0, 16))
        assert sixteen["quantiles"].shape == (N, 16) and np.all(np.diff(sixteen["quantiles"], axis=1) >= 0)
        assert np.array_equal(sixteen["quantiles"][:, 0], env["stage"]["max"].min(axis=0))
        assert np.array_equal(sixteen["quantiles"][:, 15], env["stage"]["max"].max(axis=0))
        assert 0.0 < b.last_step_ms() < 1000.0


def test_profile_bands_leave_out_a_failed_member():
    good = akbari_members(5)[:4]
    bad = FR.edited(good[1], FR.K_STAR, np.nan)                    # NaN in the target hydrograph at level 2
    with batch_from_problems([good[0], bad, good[1], good[2], good[3]], mode="rect_uniform") as b:
        b.step(NT - 1)
        assert b.status().tolist() == [A.OK, A.NAN, A.OK, A.OK, A.OK]
        env = b.envelope(("stage",), threshold=0.0)
        assert env["levels"].tolist() == [NT, FR.K_STAR, NT, NT, NT]
        enters = np.ones((5, good[0].N), dtype=bool)
        enters[1] = False
        got = check_profile(b, env["stage"]["max"], enters, "stage", "max", env["crossing"]["count"])
        assert np.all(got["n_members"] == 4)


def test_profile_bands_of_a_ragged_batch_count_the_members_that_have_the_node():
    B, N = len(RAGGED), max(RAGGED)
    enters = np.arange(N)[None, :] < np.array(RAGGED)[:, None]
    with ragged_batch(RAGGED, "f64") as b:
        b.step(STEPS)
        assert np.all(b.status() == 0)
        env = b.envelope(("depth", "velocity"), threshold=0.0, threshold_quantity="depth")
        got = check_profile(b, env["velocity"]["max"], enters, "velocity", "max", env["crossing"]["count"])
        assert got["n_members"].tolist() == [3] * 20 + [2] * 13 + [1] * 30
        assert np.all(got["exceed"] == 1.0)
    # nodes no member has: every reach is shorter than the rows of the batch
    short, N = (20, 17, 12), 24
    enters = np.arange(N)[None, :] < np.array(short)[:, None]
    with ragged_batch(short, "f64", seed=950, N=N) as b:
        b.step(STEPS)
        assert np.all(b.status() == 0)
        env = b.envelope(("depth",))
        got = check_profile(b, env["depth"]["max"], enters, "depth", "max")
        assert got["n_members"].tolist() == [3] * 12 + [2] * 5 + [1] * 3 + [0] * 4 and got["exceed"] is None
        assert np.all(np.isnan(got["mean"][20:])) and np.all(np.isnan(got["quantiles"][20:]))


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the ensemble runner
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gerd_lead():
    from cases.gerd_roseires.n_calibrate import member_setup
    fx, _ = O.load_fixture(os.path.join(GOLDEN, "gerd_ensemble.npz"))
    ns = fx["n_members"]
    solvers = [member_setup(float(n))[0] for n in ns]
    lead = solvers[0]
    lead.channel.member_ics = np.stack([s.channel.initial_conditions for s in solvers])
    return lead, ns


def direct_batch(lead, ns, tolerance, history):
    from flowsim_amd.hydromodel.preissmann import boundary_to_spec
    ch, nt = lead.channel, lead.number_of_time_levels
    b = PreissmannBatch(len(ns), lead.number_of_nodes, nt, section_mode="table", history=history)
    b.set_scheme(lead.theta, lead.time_step, lead.spatial_step, tolerance, 100)
    b.set_geometry_table(ch.node_geometry, n_main_override=np.ascontiguousarray(ns, dtype=np.float64))
    b.set_boundary(A.UPSTREAM, boundary_to_spec(ch.upstream_boundary, nt, lead.time_step))
    b.set_boundary(A.DOWNSTREAM, boundary_to_spec(ch.downstream_boundary, nt, lead.time_step))
    b.set_state(ch.member_ics[:, :, 0], ch.member_ics[:, :, 1])
    b.step(nt - 1)
    return b


def test_the_manning_ensemble_runner_returns_the_envelopes_of_a_direct_batch():
    from cases.gerd_roseires import settings as S
    from flowsim_amd.ensemble import run_manning_ensemble
    lead, ns = gerd_lead()
    fx, _ = O.load_fixture(os.path.join(GOLDEN, "gerd_ensemble.npz"))
    thr = np.median(fx["depth"].max(axis=1) + fx["geo_z_bed"][None, :], axis=0)
    spec = dict(quantities=("stage", "velocity"), threshold=thr, quantiles=(0.1, 0.5, 0.9))
    res = run_manning_ensemble(lead, ns, tolerance=S.tolerance, envelope=spec)
    assert sorted(res) == ["envelope", "hydrographs", "iterations", "profile_bands", "status"]
    with direct_batch(lead, ns, S.tolerance, True) as b:
        env = b.envelope(("stage", "velocity"), threshold=thr)
        bands = {q: b.profile_bands(q, "max", (0.1, 0.5, 0.9)) for q in ("stage", "velocity")}
        hyd = b.hydrographs()
    assert np.array_equal(res["hydrographs"], hyd) and np.all(res["status"] == 0)
    assert sorted(res["envelope"]) == ["crossing", "levels", "stage", "velocity"] and sorted(res["profile_bands"]) == ["stage", "velocity"]
    for q in ("stage", "velocity"):
        assert all(np.array_equal(res["envelope"][q][s], env[q][s]) for s in A.ENV_STATS), q
        assert all(np.array_equal(res["profile_bands"][q][k], bands[q][k]) for k in bands[q]), q
    assert all(np.array_equal(res["envelope"]["crossing"][k], env["crossing"][k]) for k in A.ENV_CROSS_ROWS)
    assert np.array_equal(res["envelope"]["levels"], env["levels"]) and res["envelope"]["levels"].tolist() == [len(hyd)] * len(ns)
    assert rel_err(res["envelope"]["stage"]["max"], fx["depth"].max(axis=1) + fx["geo_z_bed"][None, :], 1e-3) <= TOL
    with pytest.raises(ValueError, match="unknown keys"):
        run_manning_ensemble(lead, ns, tolerance=S.tolerance, envelope=dict(quantity="stage"))


def test_the_manning_ensemble_runner_without_the_keyword_is_what_it_was():
    from cases.gerd_roseires import settings as S
    from flowsim_amd.ensemble import run_manning_ensemble
    lead, ns = gerd_lead()
    res = run_manning_ensemble(lead, ns, tolerance=S.tolerance)
    assert list(res) == ["hydrographs", "iterations", "status"]
    with direct_batch(lead, ns, S.tolerance, False) as b:          # no history: the step kernels the runner has always selected
        assert np.array_equal(res["hydrographs"], b.hydrographs()) and np.array_equal(res["iterations"], b.iterations())
        assert np.array_equal(res["status"], b.status())
        with pytest.raises(A.FlowsimError, match="without FS_FLAG_HISTORY"):
            b.envelope()
