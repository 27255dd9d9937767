"""Host side of the interior gauges (fs_batch_set_gauges, fs_batch_gauges, fs_batch_gauge_score): the value of a gauge between its two
nodes, the validation of a gauge list, the layouts of the gauge block and its marks, and the walk of one member's series against its
observations are the plain-C++ half of flow-sim_amd/csrc/fs_gauge.hpp.  tests/gauges/gauge_driver.cpp is built here with the system
compiler under AddressSanitizer and UBSan and run as a program on made-up records.

score_series is held bit for bit to the sequential Python restatement of tests/gauge_checks.py (which the device is held to as well,
tests/test_gpu_gauges.py), and that restatement to vectorised numpy within (m + 2) 2^-52 times the scale of each sum."""
import os

import numpy as np
import pytest

from conftest import ROOT

import gauge_checks as G
import host_driver

DRIVER = os.path.join(ROOT, "tests", "gauges", "gauge_driver.cpp")
NAN, INF = float("nan"), float("inf")


def numbers(a):
    return " ".join(repr(float(v)) for v in a)


def value_cases():
    return {
        "between": (2.0, 4.0, 0.25), "at_the_node": (2.0, 4.0, 0.0), "b_nan_is_not_read": (2.0, NAN, 0.0), "b_inf_is_not_read": (2.0, INF, 0.0),
        "b_minus_inf_is_not_read": (-3.5, -INF, 0.0), "a_minus_zero": (-0.0, 7.0, 0.0), "a_nan": (NAN, 1.0, 0.5), "b_nan": (1.0, NAN, 0.5),
        "inf_between": (1.0, INF, 0.5), "rounds_the_product": (1.0, 1.0 + 2.0 ** -52, 1.0 / 3.0), "descending": (412.75, 409.125, 0.9),
        "tiny_weight": (1e300, -1e300, 2.0 ** -1074), "unfused": (0.1, 0.7, 0.3),
    }


def check_cases():
    """name -> (n_gauges, N, null, node, weight, text or None)"""
    return {
        "none": (0, 10, 1, [], [], None),
        "none_with_arrays": (0, 10, 0, [], [], None),
        "too_many": (33, 10, 0, [0] * 33, [0.0] * 33, "entry: n_gauges must be 0 .. 32, not 33"),
        "negative_count": (-1, 10, 0, [], [], "entry: n_gauges must be 0 .. 32, not -1"),
        "the_most": (32, 10, 0, [3] * 32, [0.5] * 32, None),
        "null": (2, 10, 1, [], [], "entry: null node or weight"),
        "good": (4, 10, 0, [0, 9, 8, 3], [0.0, 0.0, 0.5, 0.25], None),
        "node_negative": (2, 10, 0, [0, -1], [0.0, 0.0], "entry: node -1 is not inside 0 .. 9 (entry 1)"),
        "node_beyond": (2, 10, 0, [10, 0], [0.0, 0.0], "entry: node 10 is not inside 0 .. 9 (entry 0)"),
        "weight_one": (1, 10, 0, [3], [1.0], "entry: weights must be finite and in [0, 1) (entry 0)"),
        "weight_negative": (1, 10, 0, [3], [-0.1], "entry: weights must be finite and in [0, 1) (entry 0)"),
        "weight_nan": (2, 10, 0, [3, 3], [0.5, NAN], "entry: weights must be finite and in [0, 1) (entry 1)"),
        "weight_inf": (1, 10, 0, [3], [INF], "entry: weights must be finite and in [0, 1) (entry 0)"),
        "weight_minus_zero": (1, 10, 0, [9], [-0.0], None),
        "last_node_with_a_weight": (1, 10, 0, [9], [0.5], "entry: a gauge with a weight that is not 0 reads node + 1 = 10, which is not inside 0 .. 9 (entry 0)"),
        "per_reach_third_row": (2, 5, 0, [0, 1, 2, 3, 4, 4], [0.0, 0.5, 0.0, 0.5, 0.0, 0.25],
                                "entry: a gauge with a weight that is not 0 reads node + 1 = 5, which is not inside 0 .. 4 (entry 5)"),
        "two_nodes": (2, 2, 0, [0, 1], [0.999, 0.0], None),
    }


def score_cases():
    """name -> (marked, sim, obs)"""
    rng = np.random.default_rng(21)
    m = 12
    sim, obs = 400.0 + rng.uniform(0.0, 5.0, m), 400.0 + rng.uniform(0.0, 5.0, m)
    ones = np.ones(m)
    out = {"every_level": (ones, sim, obs)}
    gaps = obs.copy(); gaps[[0, 4, 5, 11]] = NAN
    out["nan_gaps"] = (ones, sim, gaps)
    out["unmarked_levels"] = ((np.arange(m) % 3 == 0).astype(float), sim, obs)
    out["unmarked_and_gaps"] = ((np.arange(m) % 2 == 0).astype(float), sim, gaps)
    unread = sim.copy(); unread[np.arange(m) % 3 != 0] = NAN                       # rows nobody evaluated hold NaN and are not read
    out["unmarked_levels_hold_nan"] = ((np.arange(m) % 3 == 0).astype(float), unread, obs)
    out["nothing_marked"] = (np.zeros(m), sim, obs)
    out["nothing_observed"] = (ones, sim, np.full(m, NAN))
    out["no_level"] = (np.zeros(0), np.zeros(0), np.zeros(0))
    one = np.zeros(m); one[7] = 1
    out["one_level"] = (one, sim, obs)
    out["constant_observations"] = (ones, sim, np.full(m, 402.5))
    out["constant_and_exact"] = (ones, np.full(m, 402.5), np.full(m, 402.5))
    ties = sim.copy(); ties[[2, 6, 9]] = 410.0
    tied_obs = obs.copy(); tied_obs[[3, 8]] = 411.0
    out["ties_for_the_peak"] = (ones, ties, tied_obs)
    bad = sim.copy(); bad[5] = NAN
    out["nan_simulated"] = (ones, bad, obs)
    late = sim.copy(); late[5] = NAN; late[2] = 500.0
    out["nan_simulated_after_the_peak"] = (ones, late, obs)
    skipped = bad.copy()
    out["nan_simulated_where_not_observed"] = (ones, skipped, np.where(np.arange(m) == 5, NAN, obs))
    out["infinite_simulated"] = (ones, np.where(np.arange(m) == 4, INF, sim), obs)
    out["flows"] = (ones, rng.uniform(-50.0, 9000.0, m), rng.uniform(0.0, 9000.0, m))
    long = 385
    out["long"] = (np.ones(long), 480.0 + np.sin(np.arange(long) / 30.0), 480.0 + np.sin(np.arange(long) / 30.0 - 0.2) + rng.normal(0, 0.05, long))
    return out


@pytest.fixture(scope="module")
def driver_output(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("gauges")
    exe = host_driver.build(DRIVER, tmp, extra_flags=["-ffp-contract=off"])
    lines = [f"V {name} {numbers(v)}" for name, v in value_cases().items()]
    lines += [f"C {name} {n} {N} {len(node)} {null} {numbers(node)} {numbers(weight)}" for name, (n, N, null, node, weight, _) in check_cases().items()]
    lines += ["L c4 4 385 32768 2 17 3", "L one 1 2 1 0 1 0", "R inside 3 0.5 10", "R last 9 0.0 10", "R last_with_weight 9 0.5 10", "R beyond 10 0.0 10",
              "R two_nodes 0 0.9 2", "R short_reach 4 0.0 3", "R next_is_beyond 2 0.25 3", "R negative -1 0.0 3"]
    lines += [f"S {name} {len(mk)} {numbers(mk)} {numbers(sim)} {numbers(obs)}" for name, (mk, sim, obs) in score_cases().items()]
    path = tmp / "records.txt"
    path.write_text("\n".join(lines) + "\n")
    got = {}
    for line in host_driver.run(exe, [path], timeout=60).splitlines():
        kind, name, rest = (line.split(" ", 2) + [""])[:3]
        got[(kind, name)] = rest
    assert len(got) == len(lines)
    return got


def test_a_gauge_between_two_nodes_and_on_one(driver_output):
    for name, (a, b, w) in value_cases().items():
        got = float(driver_output[("V", name)])
        with np.errstate(invalid="ignore", over="ignore"):
            want = a if w == 0.0 else float(np.float64(a) + np.float64(w) * (np.float64(b) - np.float64(a)))
        assert G.same(got, want), (name, got, want)
    assert float(driver_output[("V", "b_nan_is_not_read")]) == 2.0 and float(driver_output[("V", "b_inf_is_not_read")]) == 2.0
    assert np.signbit(float(driver_output[("V", "a_minus_zero")]))                 # a itself: not a + 0 * (b - a), which is +0.0
    assert float(driver_output[("V", "inf_between")]) == INF


def test_every_branch_of_the_validation(driver_output):
    for name, (*_, text) in check_cases().items():
        assert driver_output[("C", name)] == (text or "ok"), name


def test_the_layouts(driver_output):
    G_, L, B = 4, 385, 32768
    per, block, marks, row, mark = (int(v) for v in driver_output[("L", "c4")].split())
    assert (per, block, marks) == (L * 4 * B, G_ * L * 4 * B, L * B)
    assert row == np.ravel_multi_index((2, 17, 3, 0), (G_, L, 4, B)) and mark == 17 * B
    assert driver_output[("L", "one")].split() == ["8", "8", "2", "4", "1"]
    want = dict(inside=1, last=1, last_with_weight=0, beyond=0, two_nodes=1, short_reach=0, next_is_beyond=0, negative=0)
    for name, v in want.items():
        assert int(driver_output[("R", name)]) == v, name


def test_the_walk_is_the_restatement_bit_for_bit(driver_output):
    for name, (mk, sim, obs) in score_cases().items():
        f = driver_output[("S", name)].split()
        got, stray = [float(v) for v in f[:-1]], int(f[-1])
        want = G.score_series(mk, sim, obs)
        assert stray == 0, name                                                     # a level that does not count is not read
        for v, key in zip(got, G.GS_ROWS):
            assert G.same(v, want[key]), (name, key, v, want[key])


def test_the_restatement_is_numpys_within_the_bar_of_its_sums():
    for name, (mk, sim, obs) in score_cases().items():
        counted = (np.asarray(mk) != 0) & ~np.isnan(obs)
        if np.any(np.isnan(np.asarray(sim)[counted])) or np.any(np.isinf(np.asarray(sim)[counted])):
            continue
        seq = G.score_series(mk, sim, obs)
        ref, bars = G.score_numpy(mk, sim, obs)
        for key in G.GS_ROWS:
            if key == "nse" and not np.isfinite(ref[key]):
                assert not np.isfinite(seq[key]), (name, key)                       # constant observations: whatever IEEE gives
                continue
            assert G.same(seq[key], ref[key]) or abs(seq[key] - ref[key]) <= bars[key], (name, key, seq[key], ref[key], bars[key])


def test_what_the_cases_are_there_for(driver_output):
    row = lambda name: dict(zip(G.GS_ROWS, (float(v) for v in driver_output[("S", name)].split()[:-1])))
    for name in ("nothing_marked", "nothing_observed", "no_level"):
        r = row(name)
        assert r["count"] == 0 and r["peak_sim_level"] == -1 and all(np.isnan(r[k]) for k in G.GS_ROWS if k not in ("count", "peak_sim_level")), name
    mk, sim, obs = score_cases()["one_level"]
    r = row("one_level")
    assert (r["count"], r["peak_sim_level"], r["peak_lag"]) == (1, 7, 0) and r["bias"] == sim[7] - obs[7] and r["rmse"] == abs(sim[7] - obs[7])
    assert r["nse"] == -INF                                                         # one observation has no variance: 1 - sq / 0
    assert row("constant_observations")["nse"] == -INF and np.isnan(row("constant_and_exact")["nse"])      # 1 - 0 / 0
    r = row("ties_for_the_peak")
    assert (r["peak_sim"], r["peak_sim_level"], r["peak_lag"], r["peak_error"]) == (410.0, 2, -1, -1.0)    # first indices: 2 and 3
    r = row("nan_simulated")
    assert r["count"] == 12 and r["peak_sim_level"] == 5 and all(np.isnan(r[k]) for k in ("bias", "rmse", "nse", "peak_sim", "peak_error"))
    assert row("nan_simulated_after_the_peak")["peak_sim_level"] == 5               # np.argmax: the first NaN, whatever stood before
    r = row("nan_simulated_where_not_observed")
    assert r["count"] == 11 and not np.isnan(r["rmse"])
    r = row("unmarked_levels")
    assert r["count"] == 4 and r["peak_sim_level"] in (0, 3, 6, 9)
    assert row("unmarked_levels_hold_nan") == r
    assert row("nan_gaps")["count"] == 8 and row("unmarked_and_gaps")["count"] == 4
