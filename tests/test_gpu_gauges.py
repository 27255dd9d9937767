"""Interior gauges on the device (flow-sim_amd/csrc/fs_gauge.hpp: fs_batch_set_gauges, fs_batch_gauges, fs_batch_gauge_bands,
fs_batch_gauge_lookup, fs_batch_gauge_score).

Rows.  The reference is the path the library had before: the downloaded history and fs_batch_derive's level and velocity
(envelope_checks.fields_of), picked at the gauge's two nodes and interpolated in numpy, a + w (b - a) - bit for bit, in every section
mode and both dtypes: the kernel evaluates stage and velocity by derive's own lines and rounds the product before the sum.
Shapes: STEPS = 5 levels, N from 2 to 41, B in 1, 65, 130 - one lane, just past a wave, just past two.

Same bits (uint64 view, NaN being one value): a gauge on node 0 or on the last node against the hydrograph block, and gauge_bands /
gauge_lookup there against bands / lookup (the same kernels on the same values); a member alone against the same member at place 77
of 130; a range of one level against the whole range; the current state marked after every single step against the history range.

gauge_bands is held to numpy at the bars of envelope_checks.check_profile, gauge_score to the sequential restatement of
tests/gauge_checks.py bit for bit (tests/test_gauge_host.py holds that restatement to the host code and to vectorised numpy)."""
import copy
import os

import numpy as np
import pytest

from conftest import GOLDEN
import gauge_checks as G
from envelope_checks import EPS, STEPS, fields_of, ragged_batch
from failure_recipes import K_STAR, edited
from fixture_batch import batch_from_problems
from flowsim_amd import _abi as A
from flowsim_amd.batch import BoundarySpec, PreissmannBatch
from kernel_harness import TOL, rel_err
from oracle import preissmann_oracle as O
from synth import rect_problem, trap_problem

pytestmark = pytest.mark.gpu

NAN = float("nan")
NT = STEPS + 1


def same(a, b):
    """the same float64 values, NaN being one value"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def fixture_problem(name, tol=None):
    fx, meta = O.load_fixture(os.path.join(GOLDEN, name + ".npz"))
    p = O.problem_from_fixture(fx, meta)
    if tol is not None:
        p = copy.deepcopy(p)
        p.tol = tol
    return p


def rect_batch(lengths, dtype="f64", steps=STEPS, history=True, bad=None, seeds=None, N=None):
    """RECT_UNIFORM batch of seeded prismatic reaches with an inflow hydrograph (envelope_checks.ragged_batch with the seeds and the
    history flag free); bad: the reach whose target is NaN at K_STAR"""
    seeds = [900 + s for s in range(len(lengths))] if seeds is None else seeds
    probs = [rect_problem(n, seed=s, n_steps=steps) for s, n in zip(seeds, lengths)]
    if bad is not None:
        probs[bad] = edited(probs[bad], K_STAR, NAN)
    B, N, p0 = len(probs), N or max(lengths), probs[0]
    b = PreissmannBatch(B, N, p0.nt, dtype=dtype, section_mode="rect_uniform", history=history)
    b.set_scheme(p0.theta, p0.dt, p0.dx, 1e-3 if dtype == "f32" else p0.tol, p0.max_iter)
    b.set_geometry_uniform([p.geo["b_main"][0] for p in probs], [p.geo["n_main"][0] for p in probs], [p.geo["z_bed"][0] for p in probs],
                           [p.geo["z_bed"][-1] for p in probs])
    if len(set(lengths)) > 1 or N != lengths[0]:
        b.set_reach_nodes(list(lengths))
    b.set_boundary(A.UPSTREAM, BoundarySpec(A.BC_FLOW_HYDROGRAPH, {}, np.stack([p.us.target for p in probs], axis=1)))
    b.set_boundary(A.DOWNSTREAM, BoundarySpec(A.BC_NORMAL_DEPTH, dict(bed_slope=np.array([p.ds.bed_slope for p in probs]), bed_level=np.zeros(B))))
    pad = lambda a: np.concatenate([a, np.full(N - len(a), -777.0)])
    b.set_state(np.stack([pad(p.h0) for p in probs]), np.stack([pad(p.Q0) for p in probs]))
    return b


def mode_batch(mode, dtype, B):
    """(batch with history, N) of B members in one section mode, not yet stepped"""
    if mode == "rect_uniform":
        return rect_batch([33] * B, dtype), 33
    if mode == "trap_uniform":
        rng = np.random.default_rng(3)
        probs = [trap_problem(rng.uniform(20.0, 60.0), rng.uniform(0.5, 2.0), 0.03, 2e-4, rng.uniform(40.0, 90.0), 17, STEPS, tol=1e-3 if dtype == "f32" else 1e-6)
                 for _ in range(B)]
        return batch_from_problems(probs, mode="trap_uniform", dtype=dtype), 17
    if mode == "table":                                    # compound sections, over bank at every node from level 0 on
        p = fixture_problem("bc_compound_normal", tol=1e-3 if dtype == "f32" else None)
        assert np.all(p.geo["is_compound"] > 0.5) and np.all(p.h0 > p.geo["h_bf"])
        return batch_from_problems([p] * B, mode="table", dtype=dtype, n_main_override=p.geo["n_main"][0] * np.linspace(0.9, 1.1, B)), p.N
    p = fixture_problem("irr_mixed")                       # polylines at 16 of 17 nodes, one trapezoid node
    return batch_from_problems([p] * B, mode="irregular", n_main_override=p.geo["n_main"][0] * np.linspace(0.9, 1.1, B)), p.N


def five_gauges(N):
    """node 0; the last node; between the last two; an interior node at a quarter; that one again"""
    return np.array([0, N - 1, N - 2, N // 2, N // 2], dtype=np.int32), np.array([0.0, 0.0, 0.5, 0.25, 0.25])


# ---- 1. rows against numpy on the derived fields --------------------------------------------------------------------------------------
CASES = [("rect_uniform", "f64", 1), ("rect_uniform", "f64", 65), ("rect_uniform", "f64", 130), ("rect_uniform", "f32", 65),
         ("trap_uniform", "f64", 65), ("trap_uniform", "f32", 65), ("table", "f64", 65), ("table", "f32", 65), ("irregular", "f64", 65)]


@pytest.mark.parametrize("mode,dtype,B", CASES)
def test_rows_are_numpy_on_the_derived_fields_bit_for_bit(mode, dtype, B):
    b, N = mode_batch(mode, dtype, B)
    with b:
        b.step(STEPS)
        assert np.all(b.status() == A.OK), b.status()
        node, weight = five_gauges(N)
        b.set_gauges(node=node, weight=weight)
        assert np.all(np.isnan(b.gauge_rows(0, 0, NT)))                              # every row NaN until evaluated
        b.gauges(0, NT)
        assert b.last_step_ms() >= 0.0
        fields = fields_of(b, 0, NT)
        rows = [b.gauge_rows(g, 0, NT) for g in range(len(node))]
        for g, got in enumerate(rows):
            want = G.rows_numpy(fields, node[g], weight[g])
            assert got.shape == (NT, 4, B) and not np.any(np.isnan(got[:, :3])), (mode, dtype, g)
            for q, name in enumerate(A.GAUGE_ROWS):
                assert same(got[:, q], want[:, q]), (mode, dtype, g, name, np.max(np.abs(got[:, q] - want[:, q])))
        assert same(rows[3], rows[4])                                                # the duplicated gauge
        assert np.all(np.isfinite(rows[1]))                                          # a gauge on the last node: node + 1 is not read
        assert np.any(rows[3][1:, 2] != rows[3][:-1, 2])                             # the wave moves the stage at the interior gauge


# ---- 2. identities with the hydrograph block ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 65, 130])
def test_gauges_on_the_end_nodes_are_the_hydrograph_block(B):
    N = 20
    with rect_batch([N] * B) as b:
        b.step(STEPS)
        b.set_gauges(node=[0, N - 1], weight=[0.0, 0.0])
        b.gauges()
        hyd = b.hydrographs(0, NT)
        up, down = b.gauge_rows(0), b.gauge_rows(1)
        assert same(up[:, :2], hyd[:, :2]) and same(down[:, :2], hyd[:, 2:])
        q = (0.05, 0.5, 0.95, 0.0, 1.0)
        ref, gu, gd = b.bands(q, 0, NT), b.gauge_bands(0, q, 0, NT), b.gauge_bands(1, q, 0, NT)
        for k in ("min", "max", "mean", "std", "quantiles"):
            assert same(gu[k][:, :2], ref[k][:, :2]) and same(gd[k][:, :2], ref[k][:, 2:]), k      # the same kernel on the same values
        assert np.array_equal(gu["n_members"], ref["n_members"]) and np.array_equal(gd["n_members"], ref["n_members"])
        xq = np.linspace(np.min(hyd[:, 1]), np.max(hyd[:, 1]), 7)
        tgt = np.linspace(1.0, 3.0, 7)
        for g, (x_row, y_row) in ((0, (A.ROW_Q_IN, A.ROW_H_IN)), (1, (A.ROW_Q_OUT, A.ROW_H_OUT))):
            ref = b.lookup(x_row, y_row, xq, y_offset=2.5, target=tgt, first=0, n=NT)
            got = b.gauge_lookup(g, "flow", "depth", xq, y_offset=2.5, target=tgt, first=0, n=NT)
            assert same(got["values"], ref["values"]) and same(got["rmse"], ref["rmse"]) and np.array_equal(got["monotone"], ref["monotone"])


# ---- 3. a ragged batch with per-reach gauges ------------------------------------------------------------------------------------------
def test_a_ragged_batch_with_per_reach_gauges():
    lengths = (9, 2, 33, 17)
    B, N = len(lengths), 33
    # the reach's own last node; between its last two nodes (the two-node reach: its only cell); node 10 at a quarter, which the
    # reaches of 9 and 2 nodes do not have
    node = np.array([[n - 1, n - 2, 10] for n in lengths], dtype=np.int32)
    weight = np.array([[0.0, 0.5, 0.25]] * B)
    with ragged_batch(lengths, "f64") as b:
        b.step(STEPS)
        assert np.all(b.status() == A.OK)
        b.set_gauges(node=node, weight=weight)
        b.gauges()
        fields = fields_of(b, 0, NT)
        rows = [b.gauge_rows(g) for g in range(3)]
        for g in range(3):
            assert same(rows[g], G.rows_numpy(fields, node[:, g], weight[:, g], lengths)), g
        assert not np.any(np.isnan(rows[0])) and not np.any(np.isnan(rows[1]))
        has = np.array([False, False, True, True])
        assert np.all(np.isnan(rows[2][:, :, ~has])) and not np.any(np.isnan(rows[2][:, :, has]))
        obs = np.full(NT, 3.0)
        for g in range(3):
            count = b.gauge_score(g, "stage", obs)["count"]
            assert count.tolist() == [NT if (g < 2 or h) else 0 for h in has], g       # the marks: 0 where the reach has no such gauge
        q = (0.0, 0.5, 1.0)
        bands = b.gauge_bands(2, q)
        assert bands["n_members"].tolist() == [2] * NT                               # left out, as numpy leaves a NaN out (np.nanmin ...)
        v = rows[2][:, :, has]
        assert same(bands["min"], np.min(v, axis=2)) and same(bands["max"], np.max(v, axis=2))
        assert same(bands["quantiles"][:, :, 0], np.min(v, axis=2)) and same(bands["quantiles"][:, :, 2], np.max(v, axis=2))
        assert np.all(np.abs(bands["mean"] - np.mean(v, axis=2)) <= 4 * EPS * np.max(np.abs(v), axis=2))
        assert b.gauge_bands(0, q)["n_members"].tolist() == [B] * NT


# ---- 4. the same bits -----------------------------------------------------------------------------------------------------------------
def test_a_member_alone_is_the_same_member_at_place_77_of_130():
    N, place = 33, 77
    node, weight = five_gauges(N)
    out = []
    for seeds in ([900 + s for s in range(130)], [900 + place]):
        with rect_batch([N] * len(seeds), seeds=seeds) as b:
            b.step(STEPS)
            b.set_gauges(node=node, weight=weight)
            b.gauges()
            member = place if len(seeds) > 1 else 0
            out.append(np.stack([b.gauge_rows(g)[:, :, member] for g in range(len(node))]))
    assert not np.any(np.isnan(out[0])) and same(out[0], out[1])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_one_level_of_the_range_and_the_marked_current_state_are_the_history_range(dtype):
    lengths = (33, 20, 9, 2, 17)
    node = np.array([[0, n - 1, n - 2, (n - 1) // 2] for n in lengths], dtype=np.int32)
    weight = np.array([[0.0, 0.0, 0.5, 0.25 if n > 2 else 0.0] for n in lengths])
    G_ = node.shape[1]
    with rect_batch(lengths, dtype) as b:
        b.set_gauges(node=node, weight=weight)
        marked = []
        b.gauges(current=True)
        marked.append([b.gauge_rows(g, 0, 1)[0] for g in range(G_)])
        for k in range(1, NT):
            b.step(1)
            b.gauges(current=True)                                                   # the current state into row k
            marked.append([b.gauge_rows(g, k, 1)[0] for g in range(G_)])             # downloaded in between
        assert np.all(b.status() == A.OK)
        current = [b.gauge_rows(g) for g in range(G_)]
        b.set_gauges(node=node, weight=weight)                                       # every row NaN again
        assert all(np.all(np.isnan(b.gauge_rows(g))) for g in range(G_))
        b.gauges(3, 1)
        one = [b.gauge_rows(g) for g in range(G_)]
        b.gauges(0, NT)
        whole = [b.gauge_rows(g) for g in range(G_)]
        again = (b.gauges(0, NT), [b.gauge_rows(g) for g in range(G_)])[1]
        for g in range(G_):
            assert not np.any(np.isnan(whole[g])), g
            assert same(current[g], whole[g]) and same(again[g], whole[g]), g
            assert same(np.stack([m[g] for m in marked]), whole[g]), g
            assert same(one[g][3], whole[g][3]) and np.all(np.isnan(np.delete(one[g], 3, axis=0))), g


# ---- 5. a member that fails at level 2 ------------------------------------------------------------------------------------------------
def test_a_member_that_fails_at_level_2_stops_there_and_leaves_its_neighbours_alone():
    N = 33
    node, weight = five_gauges(N)
    out = {}
    for bad in (None, 1):
        with rect_batch([N] * 3, bad=bad) as b:
            b.step(STEPS)
            b.set_gauges(node=node, weight=weight)
            b.gauges()
            rows = [b.gauge_rows(g) for g in range(len(node))]
            b.gauges(current=True)
            cur = b.gauge_rows(3, STEPS, 1)
            out[bad] = (b.status(), rows, b.gauge_bands(3, (0.5,)), b.gauge_score(3, "stage", np.full(NT, 3.0)), cur)
    st, rows, bands, score, cur = out[1]
    good = out[None]
    assert st.tolist() == [A.OK, A.NAN, A.OK] and np.all(good[0] == A.OK)
    for g in range(len(node)):
        assert not np.any(np.isnan(rows[g][:K_STAR, :, 1])) and np.all(np.isnan(rows[g][K_STAR:, :, 1])), g
        assert same(rows[g][:, :, [0, 2]], good[1][g][:, :, [0, 2]]), g
        assert same(rows[g][:K_STAR, :, 1], good[1][g][:K_STAR, :, 1]), g            # its rows before the failure are what they were
    assert bands["n_members"].tolist() == [2] * NT and good[2]["n_members"].tolist() == [3] * NT
    assert same(bands["max"], np.max(rows[3][:, :, [0, 2]], axis=2)) and not np.any(np.isnan(bands["quantiles"]))
    assert score["count"].tolist() == [NT, K_STAR, NT]
    for k in G.GS_ROWS:
        assert same(score[k][[0, 2]], good[3][k][[0, 2]]), k
    assert np.all(np.isnan(cur[0][:, 1])) and same(cur[0][:, [0, 2]], rows[3][STEPS][:, [0, 2]])


# ---- 6. bands across the members against numpy ----------------------------------------------------------------------------------------
def test_gauge_bands_of_130_members_against_numpy():
    """the bars of envelope_checks.check_profile: min, max and order statistics exact, quantiles between their neighbours and within
    4 eps of numpy's, mean and std within (m + 2) eps max|x|"""
    B, N = 130, 20
    levels = (0.05, 0.5, 0.95, 0.0, 1.0, 43 / 129)
    with rect_batch([N] * B) as b:
        b.step(STEPS)
        b.set_gauges(node=[N // 2, 3], weight=[0.25, 0.0])
        b.gauges()
        for g in range(2):
            rows = b.gauge_rows(g)
            got = b.gauge_bands(g, levels)
            only = b.gauge_bands(g, ())
            assert only["quantiles"].shape == (NT, 4, 0) and all(same(only[k], got[k]) for k in ("min", "max", "mean", "std"))
            assert got["n_members"].tolist() == [B] * NT
            for k in range(NT):
                for i in range(4):
                    v = rows[k, i]
                    srt, big = np.sort(v), np.max(np.abs(v))
                    assert got["min"][k, i] == srt[0] and got["max"][k, i] == srt[-1], (g, k, i)
                    assert abs(got["mean"][k, i] - np.mean(v)) <= (B + 2) * EPS * big, (g, k, i)
                    assert abs(got["std"][k, i] - np.std(v)) <= (B + 2) * EPS * big, (g, k, i)
                    assert got["quantiles"][k, i, 3] == srt[0] and got["quantiles"][k, i, 4] == srt[-1] and got["quantiles"][k, i, 5] == srt[43]
                    for j, q in enumerate(levels[:3]):
                        vi = (B - 1) * q
                        lo, hi = srt[int(np.floor(vi))], srt[min(int(np.floor(vi)) + 1, B - 1)]
                        x = got["quantiles"][k, i, j]
                        assert lo <= x <= hi and abs(x - np.quantile(v, q)) <= 4 * EPS * max(abs(lo), abs(hi)), (g, k, i, q)


# ---- 7. scores against the restatement ------------------------------------------------------------------------------------------------
def test_gauge_score_is_the_restatement_bit_for_bit():
    """B = 65 on a batch without history, marked every two levels (levels 0, 2, 4 and the last, 5): shared observations with NaN gaps,
    per-reach observations, a member none of whose levels is observed (m = 0) and one observed at a single level"""
    B, N = 65, 20
    rng = np.random.default_rng(8)
    with rect_batch([N] * B, history=False) as b:
        with pytest.raises(A.FlowsimError, match="fs_batch_gauges: this batch has no gauges"):
            b.gauges(current=True)
        b.set_gauges(node=[N // 2, N - 1], weight=[0.25, 0.0])
        with pytest.raises(A.FlowsimError, match="fs_batch_gauges: batch was created without FS_FLAG_HISTORY"):
            b.gauges(0, 1)
        levels = [0]
        b.gauges(current=True)
        while b.level < STEPS:
            b.step(min(2, STEPS - b.level), sync=False)
            b.gauges(current=True)
            levels.append(b.level)
        b.sync()
        assert levels == [0, 2, 4, 5] and np.all(b.status() == A.OK)
        marked = np.isin(np.arange(NT), levels)
        for g in range(2):
            rows = b.gauge_rows(g)
            assert np.all(np.isnan(rows[~marked])) and not np.any(np.isnan(rows[marked])), g
            for signal, name in enumerate(A.GAUGE_ROWS):
                sim = rows[:, signal]
                shared = np.nanmean(sim[marked], axis=1)[np.searchsorted(levels, np.arange(NT)).clip(0, 3)] + rng.normal(0.0, 0.05, NT)
                shared[2] = NAN                                                      # a marked level without an observation
                per = sim.copy()
                per[~marked] = np.nanmean(sim[marked], axis=0)                        # observed where nothing was evaluated: does not count
                per += rng.normal(0.0, 0.05, per.shape)
                per[4, 3] = NAN
                per[:, 7] = NAN                                                      # m = 0
                per[[0, 2, 4], 9] = NAN                                              # m = 1
                for obs, per_reach in ((shared, False), (per, True)):
                    got = b.gauge_score(g, name, obs)
                    part = b.gauge_score(g, signal, obs[1:4], first=1, n=3)           # levels relative to `first`
                    for r in range(B):
                        o = obs[:, r] if per_reach else obs
                        want = G.score_series(marked, sim[:, r], o)
                        for k in G.GS_ROWS:
                            assert G.same(got[k][r], want[k]), (g, name, per_reach, r, k, got[k][r], want[k])
                        want = G.score_series(marked[1:4], sim[1:4, r], o[1:4])
                        assert all(G.same(part[k][r], want[k]) for k in G.GS_ROWS), (g, name, per_reach, r)
                    if per_reach:
                        assert got["count"][7] == 0 and got["peak_sim_level"][7] == -1 and np.isnan(got["rmse"][7]) and got["count"][9] == 1
                        assert got["count"][3] == 3 and got["count"][0] == 4
                    else:
                        assert np.all(got["count"] == 3)


# ---- 8. misuse ------------------------------------------------------------------------------------------------------------------------
def test_misuse_is_refused_with_a_text_that_names_the_entry_point():
    N = 20
    with rect_batch([N] * 2) as b:
        q, obs, bad_q, mom = (0.5,), np.zeros(1), np.array([1.5]), np.zeros(16)
        for call, text in ((lambda: b.gauges(), "fs_batch_gauges: this batch has no gauges"),
                           (lambda: b.gauge_rows(0, 0, 1), "fs_batch_get_gauges: this batch has no gauges"),
                           (lambda: b.gauge_bands(0, q, 0, 1), "fs_batch_gauge_bands: this batch has no gauges"),
                           (lambda: b.gauge_lookup(0, 0, 1, [1.0], first=0, n=1), "fs_batch_gauge_lookup: this batch has no gauges"),
                           (lambda: b.gauge_score(0, 0, obs, 0, 1), "fs_batch_gauge_score: this batch has no gauges"),
                           (lambda: b.set_gauges(node=[3], weight=[1.0]), r"fs_batch_set_gauges: weights must be finite and in \[0, 1\)"),
                           (lambda: b.set_gauges(node=[3], weight=[-0.1]), r"fs_batch_set_gauges: weights must be finite and in \[0, 1\)"),
                           (lambda: b.set_gauges(node=[3], weight=[NAN]), r"fs_batch_set_gauges: weights must be finite and in \[0, 1\)"),
                           (lambda: b.set_gauges(node=[N], weight=[0.0]), "fs_batch_set_gauges: node 20 is not inside 0 .. 19"),
                           (lambda: b.set_gauges(node=[-1], weight=[0.0]), "fs_batch_set_gauges: node -1 is not inside 0 .. 19"),
                           (lambda: b.set_gauges(node=[N - 1], weight=[0.5]), "fs_batch_set_gauges: a gauge with a weight that is not 0 reads node"),
                           (lambda: b.set_gauges(node=[0] * (A.GAUGE_MAX + 1), weight=[0.0] * (A.GAUGE_MAX + 1)),
                            "fs_batch_set_gauges: n_gauges must be 0 .. 32, not 33")):
            with pytest.raises((A.FlowsimError, ValueError), match=text):
                call()
        assert b.gauges_device_ptr(0) is None
        b.set_gauges(node=[0, 5], weight=[0.0, 0.5])
        assert b.gauges_device_ptr(0) and b.gauges_device_ptr(1) and b.gauges_device_ptr(2) is None
        assert b.gauges_device_ptr(1) - b.gauges_device_ptr(0) == b.L * 4 * b.B * 8
        b.step(2)
        for call, text in ((lambda: b.gauge_rows(2, 0, 1), "fs_batch_get_gauges: gauge 2 is not one of 0 .. 1"),
                           (lambda: b.gauge_bands(-1, q, 0, 1), "fs_batch_gauge_bands: gauge -1 is not one of 0 .. 1"),
                           (lambda: b.gauge_score(2, 0, obs, 0, 1), "fs_batch_gauge_score: gauge 2 is not one of 0 .. 1"),
                           (lambda: b.gauge_score(0, 4, obs, 0, 1), "fs_batch_gauge_score: signal 4 is not one of"),
                           (lambda: b.gauge_score(0, -1, obs, 0, 1), "fs_batch_gauge_score: signal -1 is not one of"),
                           (lambda: b.gauge_lookup(0, 4, 0, [1.0], first=0, n=1), "fs_batch_gauge_lookup: x_row and y_row are 0..3"),
                           (lambda: b.gauges(0, 4), r"fs_batch_gauges: levels \[0, 4\) are not inside 0 .. 2"),
                           (lambda: b.gauge_bands(0, q, 1, 3), r"fs_batch_gauge_bands: levels \[1, 4\) are not inside 0 .. 2"),
                           (lambda: b.gauge_bands(0, (1.5,), 0, 1), "quantile levels must be in"),      # (the binding's own check)
                           (lambda: A.check(b._lib.fs_batch_gauge_bands(b._h, 0, 0, 1, bad_q.ctypes.data_as(A._D), 1, mom.ctypes.data_as(A._D), None, None)),
                            "fs_batch_gauge_bands: quantile levels must be in"),
                           (lambda: b.gauge_score(0, 0, np.zeros(4), 0, 4), r"fs_batch_gauge_score: levels \[0, 4\) are not inside 0 .. 2"),
                           (lambda: b.gauge_rows(0, 0, b.L + 1), "fs_batch_get_gauges: level range out of bounds"),
                           (lambda: A.check(b._lib.fs_batch_gauges(b._h, -1, 2), "gauges"), "fs_batch_gauges: first = -1 evaluates the current state, one row: n must be 1"),
                           (lambda: b.gauge_lookup(0, 1, 0, [1.0], first=0, n=3), "fs_batch_gauge_lookup: level 0 of the range was never evaluated")):
            with pytest.raises((A.FlowsimError, ValueError), match=text):
                call()
        b.gauges(0, 2)
        with pytest.raises(A.FlowsimError, match="fs_batch_gauge_lookup: level 2 of the range was never evaluated"):
            b.gauge_lookup(0, 1, 0, [1.0], first=0, n=3)
        assert b.gauge_lookup(0, 1, 0, [1.0], first=0, n=2)["values"].shape == (1, 2)
        assert np.all(np.isnan(b.gauge_rows(0, 2, 1))) and not np.any(np.isnan(b.gauge_rows(0, 0, 2)))      # nothing was launched by the refused calls
    p = fixture_problem("bc_compound_normal")                                        # (fs_batch_iterate steps table batches)
    with batch_from_problems([p] * 2, mode="table") as b:
        b.set_gauges(node=[0, 5], weight=[0.0, 0.5])
        b.step(1)
        assert b.iterate() > 0                                                       # one Newton iteration does not close the level
        with pytest.raises(A.FlowsimError, match="fs_batch_gauges: a level opened with fs_batch_iterate must be closed first"):
            b.gauges(current=True)
        for _ in range(50):
            if b.iterate() == 0:
                break
        assert b.level == 2
        b.gauges(current=True)
        assert not np.any(np.isnan(b.gauge_rows(1, 2, 1))) and np.all(np.isnan(b.gauge_rows(1, 0, 2)))
    with rect_batch([N] * 2, history=False) as b:
        b.set_gauges(node=[0], weight=[0.0])
        b.step(1)
        with pytest.raises(A.FlowsimError, match="fs_batch_gauges: batch was created without FS_FLAG_HISTORY"):
            b.gauges(0, 2)
        b.set_gauges(node=[], weight=[])                                             # no gauges: the block is freed
        assert b.gauges_device_ptr(0) is None
        with pytest.raises(A.FlowsimError, match="fs_batch_gauges: this batch has no gauges"):
            b.gauges(current=True)


# ---- 9. a new state resets the rows ---------------------------------------------------------------------------------------------------
def test_set_state_init_state_and_restart_reset_the_rows():
    lengths = (33, 20)
    probs = [rect_problem(n, seed=900 + s, n_steps=STEPS) for s, n in enumerate(lengths)]
    node = np.array([[n // 2, n - 1] for n in lengths], dtype=np.int32)
    weight = np.array([[0.25, 0.0]] * 2)
    with rect_batch(lengths) as b:
        b.set_gauges(node=node, weight=weight)
        b.step(STEPS)
        b.gauges()
        first = [b.gauge_rows(g) for g in range(2)]
        full = np.full(NT, 3.0)
        assert not np.any(np.isnan(first[0])) and np.all(b.gauge_score(0, "stage", full)["count"] == NT)
        h, Q = b.state()
        gh, gQ = b.guess()
        b.restart(2, h, Q, gh, gQ)
        assert b.level == 2 and all(np.all(np.isnan(b.gauge_rows(g, 0, NT))) for g in range(2))
        assert np.all(b.gauge_score(0, "stage", full[:1], 2, 1)["count"] == 0)        # ... and every mark 0
        b.gauges(current=True)
        after = b.gauge_rows(0, 0, NT)
        assert np.flatnonzero(~np.isnan(after[:, 0, 0])).tolist() == [2] and same(after[2], first[0][STEPS])      # the state it was restarted with
        b.init_state("linear", [p.Q0[0] for p in probs], depth_ds=[p.h0[-1] for p in probs], depth_us=[p.h0[0] for p in probs])
        assert b.level == 0 and all(np.all(np.isnan(b.gauge_rows(g, 0, NT))) for g in range(2))
        b.gauges(0, 1)
        assert not np.any(np.isnan(b.gauge_rows(1, 0, 1)))
        pad = lambda a, n: np.concatenate([a, np.full(b.N - n, -777.0)])
        b.set_state(np.stack([pad(p.h0, p.N) for p in probs]), np.stack([pad(p.Q0, p.N) for p in probs]))
        assert all(np.all(np.isnan(b.gauge_rows(g, 0, NT))) for g in range(2))
        with pytest.raises(A.FlowsimError, match="was never evaluated"):
            b.gauge_lookup(0, 1, 0, [1.0], first=0, n=1)
        b.step(STEPS)
        b.gauges()
        assert all(same(b.gauge_rows(g), first[g]) for g in range(2))               # the same run, the same bits


# ---- 10. the runners' gauges= keyword -------------------------------------------------------------------------------------------------
def test_the_manning_runner_returns_the_gauges_of_a_direct_batch_and_changes_nothing_else():
    from cases.gerd_roseires import settings as S
    from cases.gerd_roseires.model import build as build_model
    from flowsim_amd.ensemble import run_manning_ensemble
    solver, _ = build_model(inflow_hyd_func=None, sim_duration=6 * 3600)
    n_vals = np.linspace(0.025, 0.035, 8)
    nt, N, dx = solver.number_of_time_levels, solver.number_of_nodes, solver.spatial_step
    chainage = np.array([0.0, 10.25 * dx, (N - 1.5) * dx, (N - 1) * dx])
    plain = run_manning_ensemble(solver, n_vals, tolerance=S.tolerance)
    assert np.all(plain["status"] == 0)
    observed = np.full((4, nt), NAN)
    observed[:, ::2] = 480.0 + np.arange(0, nt, 2) * 0.01
    kw = dict(chainage=chainage, quantiles=(0.5,), observed=observed)
    whole = run_manning_ensemble(solver, n_vals, tolerance=S.tolerance, envelope=dict(quantities=("depth",)), gauges=kw)
    marked = run_manning_ensemble(solver, n_vals, tolerance=S.tolerance, gauges=dict(every=2, **kw))
    assert list(marked) == list(plain) + ["gauges"] and sorted(marked["gauges"]) == ["bands", "node", "rows", "score", "weight"]
    for k in plain:                                                                   # stepping in chunks changes none of the old bits
        assert np.array_equal(marked[k], plain[k]), k
    g = whole["gauges"]
    assert g["node"].tolist() == [0, 10, N - 2, N - 1] and np.allclose(g["weight"], [0.0, 0.25, 0.5, 0.0], rtol=0, atol=1e-12)
    assert g["rows"].shape == (4, nt, 4, 8) and not np.any(np.isnan(g["rows"][:, :, :3]))
    assert same(g["rows"][0][:, :2], whole["hydrographs"][:, :2]) and same(g["rows"][3][:, :2], whole["hydrographs"][:, 2:])
    levels = sorted(set(range(0, nt, 2)) | {nt - 1})
    rows = marked["gauges"]["rows"]
    on = np.isin(np.arange(nt), levels)
    assert np.all(np.isnan(rows[:, ~on])) and not np.any(np.isnan(rows[:, on, :3]))
    floor = dict(depth=1e-3, flow=1.0, stage=1e-3, velocity=1e-3)
    for q, name in enumerate(A.GAUGE_ROWS):                                           # different step instantiations, chunked stepping
        assert rel_err(rows[:, on, q], g["rows"][:, on, q], floor[name]) <= TOL, name
    assert len(g["bands"]) == len(g["score"]) == 4
    assert same(g["bands"][1]["max"], np.max(g["rows"][1], axis=2)) and g["bands"][1]["quantiles"].shape == (nt, 4, 1)
    n_obs = len(range(0, nt, 2))
    for i in range(4):
        assert np.all(g["score"][i]["count"] == n_obs) and np.all(marked["gauges"]["score"][i]["count"] == n_obs)
        for r in range(8):
            want = G.score_series(np.ones(nt), g["rows"][i][:, 2, r], observed[i])
            assert all(G.same(g["score"][i][k][r], want[k]) for k in G.GS_ROWS), (i, r)
    no_rows = run_manning_ensemble(solver, n_vals, tolerance=S.tolerance, gauges=dict(every=2, rows=False, chainage=chainage))
    assert sorted(no_rows["gauges"]) == ["bands", "node", "weight"]
    with pytest.raises(ValueError, match="unknown keys"):
        run_manning_ensemble(solver, n_vals, tolerance=S.tolerance, gauges=dict(chainge=chainage))
    with pytest.raises(ValueError, match="every=4 and every=2 differ"):
        run_manning_ensemble(solver, n_vals, tolerance=S.tolerance, balance=dict(every=4), gauges=dict(every=2, chainage=chainage))
    both = run_manning_ensemble(solver, n_vals, tolerance=S.tolerance, balance=dict(every=2), gauges=dict(every=2, chainage=chainage))
    assert same(both["gauges"]["rows"], rows) and np.flatnonzero(~np.isnan(both["balance"]["rows"]["volume"][:, 0])).tolist() == levels
