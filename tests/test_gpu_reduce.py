"""Ensemble post-processing on the device (fs_batch_summarize, fs_batch_lookup, fs_batch_bands; flow-sim_amd/csrc/fs_reduce.hpp).

The reference in every comparison is numpy applied to what b.hydrographs() and b.status() return from the SAME batch - an existing,
tested path - so the bars are those of tests/test_reduce_host.py: peaks, levels and order statistics exact, sums within the
sequential-against-pairwise bound m eps sum|Q|, interpolated values within 8 eps max|fp|.

Batches: the rectangular akbari problem as B = 1, 3, 67, 257 members (widths and Manning n drawn with a fixed seed, two members
identical) in fp64 and fp32, and example (storage boundary, negative outflow at level 1) as B = 5; 21 levels each."""
import copy
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN
import failure_recipes as FR
from fixture_batch import batch_from_problems
from flowsim_amd import _abi as A
from oracle import preissmann_oracle as O

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
NT = 21
RANGES = ((0, 21), (0, 1), (0, 2), (3, 7))
BATCHES = [("akbari", B, dtype) for dtype in ("f64", "f32") for B in (1, 3, 67, 257)] + [("example", 5, "f64")]
IDS = [f"{c}-{d}-B{B}" for c, B, d in BATCHES]
SIGNALS = ("h_in", "q_in", "h_out", "q_out")


def members(case, B, dtype):
    """B copies of the fixture's reach that differ in width and Manning n (+-10 %, fixed seed); the last repeats the first"""
    fx, meta = O.load_fixture(os.path.join(GOLDEN, case + ".npz"))
    base = O.problem_from_fixture(fx, meta)
    base.nt = NT
    if dtype == "f32":
        base.tol = 1e-3          # (fp32 cannot resolve the residual norm below ~1e-4 on these reaches: include/flowsim_abi.h, FS_F32)
    rng = np.random.default_rng(20261019)
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


_open = []


@functools.lru_cache(maxsize=None)
def run(case, B, dtype):
    """(batch, hydrographs [NT, 4, B], status [B]) of a batch stepped to level NT - 1; the batch stays open for the module"""
    b = batch_from_problems(members(case, B, dtype), mode="auto", dtype=dtype, history=False)
    _open.append(b)
    b.step(NT - 1)
    return b, b.hydrographs(0, NT), b.status()


@pytest.fixture(scope="module", autouse=True)
def close_batches():
    yield
    run.cache_clear()
    while _open:
        _open.pop().close()


def failed(status):
    return (status != A.OK) & (status != A.ILL_CONDITIONED)


def reference_median_level(q):
    """solver.py:219-229 as written"""
    cumulative = [np.sum(q[:i]) for i in range(q.size)]
    for i in range(len(cumulative)):
        if cumulative[i] >= 0.5 * cumulative[-1]:
            return i
    raise AssertionError("the reference's loop found no level")


def median_margin_ok(q):
    """no cum_i lies within the summation bound (sequential against pairwise over m levels) of its threshold; sums of at most two
    terms (m <= 3) round the same in any order, so there the levels are defined without a margin"""
    if q.size <= 3:
        return True
    cum = np.array([np.sum(q[:i]) for i in range(q.size)])
    return bool(np.all(np.abs(cum - 0.5 * cum[-1]) > q.size * EPS * np.sum(np.abs(q))))


def check_summary(s, r, cols):
    """member r of the summaries dict s against numpy on its four columns [m]"""
    h_in, q_in, h_out, q_out = cols
    m = len(q_in)
    assert s["levels"][r] == m
    for key, col in zip(SIGNALS, cols):
        assert s["peak_" + key][r] == np.max(col), (r, key)
        assert s["peak_" + key + "_level"][r] == np.argmax(col), (r, key)
    for key, terms in (("q_in", q_in), ("q_out", q_out), ("q_net", q_in - q_out)):
        assert abs(s[key][r] - np.sum(terms)) <= m * EPS * np.sum(np.abs(terms)), (r, key, s[key][r], np.sum(terms))
    # first on the numpy side: no cumulative sum lies within the summation bound of its threshold; a column that fails this is left
    # out of the median assertion and returned
    left_out = []
    for side, q in (("in", q_in), ("out", q_out)):
        if median_margin_ok(q):
            assert s["median_" + side + "_level"][r] == reference_median_level(q), (r, side)
        else:
            left_out.append(side)
    return left_out


@pytest.mark.parametrize("case,B,dtype", BATCHES, ids=IDS)
def test_summaries(case, B, dtype):
    b, hyd, status = run(case, B, dtype)
    assert b.level == NT - 1 and not np.any(failed(status))
    for first, n in RANGES:
        s = b.summaries(first, n)
        assert sorted(s) == sorted(A.SUM_ROWS) and all(v.shape == (B,) for v in s.values())
        left_out = {side for r in range(B) for side in check_summary(s, r, [hyd[first:first + n, i, r] for i in range(4)])}
        # example's inflow is 10 000 m3/s at each of the levels 3 .. 9: the cumulative inflow of level 3 + 3 IS half of the six levels
        # counted, a tie by construction, so that column is left out of the median assertion; every other column of every batch is in
        assert left_out == ({"in"} if (case, first, n) == ("example", 3, 7) else set()), (first, n, left_out)
    full = b.summaries()
    assert all(np.array_equal(full[k], b.summaries(0, NT)[k]) for k in A.SUM_ROWS)
    if B > 1:      # the two identical members
        assert all(full[k][0] == full[k][-1] for k in A.SUM_ROWS)


def rising_limb(hyd):
    """levels [0, n) over which every member's upstream flow never descends (at least two levels)"""
    q = hyd[:, 1, :]
    n = 2
    while n < len(q) and np.all(np.diff(q[:n + 1], axis=0) >= 0):
        n += 1
    return n


@pytest.mark.parametrize("case,B,dtype", BATCHES, ids=IDS)
def test_lookup(case, B, dtype):
    b, hyd, _ = run(case, B, dtype)
    covered = 0
    for first, n in ((0, NT), (0, rising_limb(hyd)), (3, 7)):
        xp0 = hyd[first:first + n, 1, 0]
        lo, hi = np.min(hyd[first:first + n, 1, :]), np.max(hyd[first:first + n, 1, :])
        # below, inside, on a sample of member 0, inside, above
        xq = np.array([lo - 1.0, lo + 0.3 * (hi - lo), xp0[min(2, n - 1)], lo + 0.71 * (hi - lo), hi + 1.0])
        target = np.array([1.0, 2.0, 3.0, 2.0, 1.0])
        offset = np.linspace(5.0, 17.69, B)
        got = b.lookup(A.ROW_Q_IN, A.ROW_H_IN, xq, y_offset=offset, target=target, first=first, n=n)
        assert got["values"].shape == (5, B) and got["rmse"].shape == (B,) and got["monotone"].shape == (B,)
        for r in range(B):
            xp, fp = hyd[first:first + n, 1, r], hyd[first:first + n, 0, r] + offset[r]
            monotone = bool(np.all(np.diff(xp) >= 0))
            assert got["monotone"][r] == monotone, (r, first, n)
            if monotone:
                want = np.interp(xq, xp, fp)
                assert np.all(np.abs(got["values"][:, r] - want) <= 8 * EPS * np.max(np.abs(fp))), (r, got["values"][:, r], want)
                covered += 1
            assert np.all(np.isfinite(got["values"][:, r]))
            rmse = np.mean((got["values"][:, r] - target) ** 2) ** 0.5
            assert abs(got["rmse"][r] - rmse) <= 8 * EPS * rmse, (r, got["rmse"][r], rmse)
        plain = b.lookup(A.ROW_Q_IN, A.ROW_H_IN, xq, first=first, n=n)          # no offset, no target
        assert plain["rmse"] is None and np.array_equal(plain["monotone"], got["monotone"])
    print(case, B, dtype, "values compared on", covered, "nondecreasing series")
    assert covered >= B          # the rising limb at least


def check_bands(b, hyd, keep, first, n):
    x = hyd[first:first + n][:, :, keep]                 # [n, 4, m]
    m = x.shape[2]
    srt = np.sort(x, axis=2)
    big = np.max(np.abs(x), axis=2)
    got = b.bands((0.05, 0.5, 0.95, 0.0, 1.0), first, n)
    assert np.array_equal(got["n_members"], np.full(n, m))
    assert np.array_equal(got["min"], srt[:, :, 0]) and np.array_equal(got["max"], srt[:, :, -1])
    assert np.all(np.abs(got["mean"] - np.mean(x, axis=2)) <= (m + 2) * EPS * big)
    assert np.all(np.abs(got["std"] - np.std(x, axis=2)) <= (m + 2) * EPS * big)
    assert np.array_equal(got["quantiles"][:, :, 3], srt[:, :, 0]) and np.array_equal(got["quantiles"][:, :, 4], srt[:, :, -1])
    for i, q in enumerate((0.05, 0.5, 0.95)):
        vi = (m - 1) * q
        a, c = srt[:, :, int(np.floor(vi))], srt[:, :, min(int(np.floor(vi)) + 1, m - 1)]
        v = got["quantiles"][:, :, i]
        assert np.all((a <= v) & (v <= c)), q
        assert np.all(np.abs(v - np.quantile(x, q, axis=2)) <= 4 * EPS * np.maximum(np.abs(a), np.abs(c))), q
    # quantile levels k / (m - 1) whose virtual index is the integer k in floating point: they land on samples
    if m > 1:
        ks = [k for k in sorted(set(np.linspace(0, m - 1, A.BANDS_MAX_Q).astype(int).tolist() + [1, m - 2])) if 0 <= k <= m - 1]
        ks = [k for k in ks if (m - 1) * (k / (m - 1)) == k][:A.BANDS_MAX_Q]
        assert len(ks) >= min(m, 3)
        got = b.bands([k / (m - 1) for k in ks], first, n)
        for i, k in enumerate(ks):
            assert np.array_equal(got["quantiles"][:, :, i], srt[:, :, k]), k
    only = b.bands((), first, n)
    assert only["quantiles"].shape == (n, 4, 0) and np.array_equal(only["min"], srt[:, :, 0])


@pytest.mark.parametrize("case,B,dtype", BATCHES, ids=IDS)
def test_bands(case, B, dtype):
    b, hyd, status = run(case, B, dtype)
    assert np.all(hyd[0, 1, :] == hyd[0, 1, 0])          # level 0: every member starts from the same flow - rows of equal values
    check_bands(b, hyd, np.arange(B), 0, NT)
    check_bands(b, hyd, np.arange(B), 3, 7)


def test_one_failing_member_between_good_ones():
    good = members("akbari", 4, "f64")[:3]
    assert FR.K_STAR == 2
    bad = FR.edited(good[1], FR.K_STAR, np.nan)          # NaN in the target hydrograph at level 2
    with batch_from_problems(good, history=False) as b:
        b.step(NT - 1)
        assert not np.any(failed(b.status()))
        alone = b.summaries()
    with batch_from_problems([good[0], bad, good[1], good[2]], history=False) as b:
        b.step(NT - 1)
        status, hyd = b.status(), b.hydrographs(0, NT)
        assert status.tolist() == [A.OK, A.NAN, A.OK, A.OK]
        s = b.summaries()
        assert s["levels"].tolist() == [NT, 2, NT, NT]
        assert check_summary(s, 1, [hyd[:2, i, 1] for i in range(4)]) == []          # rows 0 and 1 only
        for first, n, rows in ((1, 5, 1), (2, 3, 0), (0, 1, 1)):
            assert b.summaries(first, n)["levels"].tolist() == [n, rows, n, n]
        none = b.summaries(2, 3)
        assert np.isnan(none["peak_q_in"][1]) and none["peak_q_in_level"][1] == -1 and none["q_in"][1] == 0
        keep = [0, 2, 3]
        for k in A.SUM_ROWS:                              # the other members: bit for bit those of the batch without the failing one
            assert np.array_equal(s[k][keep], alone[k]), k
        check_bands(b, hyd, np.array(keep), 0, NT)       # n_members = B - 1 at every level, numpy on the remaining members
        got = b.lookup(A.ROW_Q_IN, A.ROW_H_IN, [hyd[0, 1, 1] + 1.0], first=0, n=NT)
        xp, fp = hyd[:2, 1, 1], hyd[:2, 0, 1]
        assert got["monotone"][1] == bool(xp[1] >= xp[0])
        if got["monotone"][1]:
            assert abs(got["values"][0, 1] - np.interp(hyd[0, 1, 1] + 1.0, xp, fp)) <= 8 * EPS * np.max(np.abs(fp))


def test_calibration_scores_on_the_device():
    """cases/gerd_roseires/n_calibrate.py with device_score=True: levels at the gauge flows and RMSE from fs_batch_lookup, no
    hydrograph download; the bar is the one the download path is held to (tests/test_gpu_dropin.py)."""
    from cases.gerd_roseires.n_calibrate import rmse_curve
    fx = np.load(os.path.join(GOLDEN, "rmse_curve.npz"))
    details = {}
    got = np.array(rmse_curve(fx["n_values"], device_score=True, details=details))
    assert details["monotone"].shape == (10,) and np.all(details["monotone"])          # info == 0 for all ten members
    np.testing.assert_allclose(got, fx["rmse"], rtol=1e-8, atol=0)
    np.testing.assert_allclose(details["levels"], fx["levels"], rtol=1e-8, atol=0)


def test_argument_errors_leave_the_batch_usable():
    b, hyd, _ = run("akbari", 3, "f64")
    lib, h = b._lib, b._h
    B = 3
    out = np.empty((len(A.SUM_ROWS), B))
    val, rm, info = np.empty((2, B)), np.empty(B), np.empty(B, dtype=np.int32)
    xq = np.array([150.0, 250.0])
    q = np.linspace(0, 1, 17)
    mom, qu, cnt = np.empty((NT, 4, 4)), np.empty((NT, 4, 17)), np.empty(NT, dtype=np.int32)
    D = lambda a: a.ctypes.data_as(A._D)
    I = lambda a: a.ctypes.data_as(A._I)
    calls = {
        "range past the current level (summarize)": lambda: lib.fs_batch_summarize(h, 0, NT + 1, D(out)),
        "range past the current level (lookup)": lambda: lib.fs_batch_lookup(h, 15, 7, 1, 0, None, D(xq), 2, None, D(val), None, None),
        "range past the current level (bands)": lambda: lib.fs_batch_bands(h, NT, 1, D(q), 3, D(mom), D(qu), I(cnt)),
        "empty range": lambda: lib.fs_batch_summarize(h, 0, 0, D(out)),
        "negative first": lambda: lib.fs_batch_summarize(h, -1, 2, D(out)),
        "n_q = 17": lambda: lib.fs_batch_bands(h, 0, NT, D(q), 17, D(mom), D(qu), I(cnt)),
        "n_q = 0 (lookup)": lambda: lib.fs_batch_lookup(h, 0, NT, 1, 0, None, D(xq), 0, None, D(val), None, None),
        "quantile level outside [0, 1]": lambda: lib.fs_batch_bands(h, 0, NT, D(np.array([0.5, 1.5])), 2, D(mom), D(qu), I(cnt)),
        "rmse without target": lambda: lib.fs_batch_lookup(h, 0, NT, 1, 0, None, D(xq), 2, None, D(val), D(rm), I(info)),
        "row out of range": lambda: lib.fs_batch_lookup(h, 0, NT, 4, 0, None, D(xq), 2, None, D(val), None, None),
        "all outputs NULL (summarize)": lambda: lib.fs_batch_summarize(h, 0, NT, None),
        "all outputs NULL (lookup)": lambda: lib.fs_batch_lookup(h, 0, NT, 1, 0, None, D(xq), 2, None, None, None, None),
        "all outputs NULL (bands)": lambda: lib.fs_batch_bands(h, 0, NT, D(q), 3, None, None, None),
        "NULL handle": lambda: lib.fs_batch_summarize(None, 0, NT, D(out)),
    }
    before = b.summaries()
    for what, call in calls.items():
        assert call() == -1, what
        assert len(A.last_error()) > 10, what
    after = b.summaries()
    assert all(np.array_equal(before[k], after[k]) for k in A.SUM_ROWS)
    assert lib.fs_batch_bands(h, 0, NT, None, 0, D(mom), None, None) == 0          # n_q = 0 is allowed
    assert np.array_equal(mom[:, :, 0], np.min(hyd, axis=2))
    assert np.array_equal(b.hydrographs(0, NT), hyd)
