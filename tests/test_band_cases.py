"""The band kernels' cases and their numpy model (tests/band_cases.py), checked on the CPU: the restated radix select returns np.sort's
order statistics on every case, the key is monotone and round-trips, and the cases - as written - reach every path of the kernels'
counting loop that tests/test_gpu_band_select.py is there to run.  A row of the census that no case reaches is named in the failure."""
import numpy as np
import pytest

import band_cases as BC


def test_the_key_is_monotone_and_round_trips():
    rng = np.random.default_rng(7)
    v = np.concatenate([rng.uniform(-1, 1, 500), rng.choice([-1.0, 1.0], 500) * 10.0 ** rng.uniform(-300, 300, 500),
                        [0.0, -0.0, 5e-324, -5e-324, 1e-320, -1e-320, np.inf, -np.inf, 1.7976931348623157e308, -1.7976931348623157e308,
                         2.2250738585072014e-308, -2.2250738585072014e-308, 1.0, np.nextafter(1.0, 2.0), -1.0, np.nextafter(-1.0, -2.0)]])
    v = np.sort(v)
    k = BC.band_key(v)
    assert k.dtype == np.uint64
    assert np.all(k[1:] >= k[:-1]) and np.array_equal(k[1:] == k[:-1], v[1:] == v[:-1])          # strictly monotone; equal only where equal
    back = BC.band_unkey(k)
    assert np.array_equal(back.view(np.uint64), (v + 0.0).view(np.uint64))                       # bit for bit, -0.0 folded into +0.0
    assert BC.band_key(np.array([-0.0]))[0] == BC.band_key(np.array([0.0]))[0] == np.uint64(1) << np.uint64(63)
    assert BC.band_key(np.array([-5e-324]))[0] == (np.uint64(1) << np.uint64(63)) - np.uint64(2)   # the negative branch: ~u


def test_lead_and_ranks_are_the_kernels():
    assert BC.lead_bytes(0x8000000000000000, 0x7fffffffffffffff) == 0
    assert BC.lead_bytes(0xbff0000000000000, 0xbff00000000000ff) == 7
    assert BC.lead_bytes(0xbff0000000000000, 0xbff0000000000100) == 6
    assert BC.lead_bytes(0xbf00000000000000, 0xbfff000000000000) == 1
    assert BC.ranks(1, 0.3) == (0, 0, 0.0) and BC.ranks(5, 1.0) == (4, 4, 0.0) and BC.ranks(5, 0.0) == (0, 1, 0.0)
    lo, hi, g = BC.ranks(5, 0.6)
    assert (lo, hi) == (2, 3) and g == np.float64(4) * np.float64(0.6) - 2.0
    # quantile_lerp: the upper form from gamma = 0.5 on, kept inside [a, b]
    assert BC.quantile_lerp(1.0, 3.0, 0.25) == 1.5 and BC.quantile_lerp(1.0, 3.0, 0.75) == 3.0 - 2.0 * 0.25
    assert BC.quantile_lerp(2.0, 2.0, 0.3) == 2.0
    # an order statistic itself is not computed: an infinite member stays that infinity (numpy's inf - inf and inf * 0 are NaN)
    inf = np.inf
    assert BC.quantile_lerp(inf, inf, 0.0) == inf and BC.quantile_lerp(-inf, 1.0, 0.0) == -inf and BC.quantile_lerp(1.0, inf, 0.0) == 1.0
    assert BC.quantile_lerp(-inf, -inf, 0.7) == -inf and BC.quantile_lerp(-1.7e308, 1.7e308, 0.0) == -1.7e308
    # ... and on finite members returning a is what the arithmetic gives, bit for bit
    for a, b in ((1.0, 3.0), (-3.0, -1.0), (0.0, 5e-324), (-1e300, 1e300), (2.5, 2.5)):
        d = np.float64(b) - np.float64(a)
        assert np.float64(a) + d * np.float64(0.0) == a and (a != b or np.float64(b) - d * np.float64(0.25) == a)


def test_case_names_are_unique_and_every_size_and_pattern_occurs():
    names = [c.name for c in BC.ALL_CASES]
    assert len(set(names)) == len(names)
    for fam in "adf":
        sizes = {c.B for c in BC.ALL_CASES if c.family == fam}
        assert set(BC.B_SMALL) <= sizes, fam
        assert (set(BC.B_LARGE) <= sizes) == (fam in "ad"), fam
        for pat in BC.PATTERNS:
            assert any(c.name.endswith("-" + pat) for c in BC.ALL_CASES if c.family == fam), (fam, pat)
    assert all(c.B in BC.B_LARGE for c in BC.ALL_CASES if c.large) and all(c.family in "ad" for c in BC.ALL_CASES if c.large)
    assert {c.family for c in BC.CASES_F64} == set("abcdefghi") and {c.family for c in BC.CASES_F32} == {"j"}
    assert all(c.x.dtype == np.float32 for c in BC.CASES_F32) and all(c.x.dtype == np.float64 for c in BC.CASES_F64)
    for c in BC.ALL_CASES:
        q = c.q("q16")
        assert len(q) == BC.MAX_Q and len(set(q.tolist())) == BC.MAX_Q and np.all((q >= 0) & (q <= 1)), c


_CENSUS = {}


def census(case, qset):
    key = (case.name, qset)
    if key not in _CENSUS:
        q = case.q(qset)
        got, cen = BC.select(case.x, case.kept, q)
        if got is not None:
            s = np.sort(case.values())
            m = len(s)
            want = np.array([s[r] for t in q for r in BC.ranks(m, t)[:2]], dtype=np.float64).reshape(-1)
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (case, qset)       # bit for bit: np.sort's order statistics
        _CENSUS[key] = cen
    return _CENSUS[key]


@pytest.mark.parametrize("family", BC.FAMILIES)
def test_the_restated_select_returns_np_sorts_order_statistics(family):
    n = 0
    for case in (c for c in BC.ALL_CASES if c.family == family):
        for qset in BC.Q_SETS:
            cen = census(case, qset)
            e = BC.expected(case.values(), case.q(qset))
            assert e["none"] == cen["no_row"], (case, qset)
            n += 1
    assert n > 0


def test_the_cases_reach_every_path_of_the_counting_loop():
    """every row of this table must be reached by the cases as written; none may be skipped"""
    rows = {f"lead == {k} ({8 - k} passes)": False for k in range(8)}
    rows.update({name: False for name in (
        "negative keys only", "positive keys only", "keys of both signs in one row", "-0.0 among the members",
        "select skipped (kmin == kmax)", "a wave adds its popcount once", "a wave adds lane by lane",
        "both counting paths in one pass", "a wave's first active lane is not lane 0", "a wave with no member at all",
        "a rank at the first position of a run of ties", "a rank at the last position of a run of ties",
        "a rank inside a run of ties", "the same in fp32 rows: both counting paths in one pass")})
    for case in BC.ALL_CASES:
        for qset in BC.Q_SETS:
            c = census(case, qset)
            if c["lead"] is not None:
                rows[f"lead == {c['lead']} ({c['passes']} passes)"] = True
            rows["negative keys only"] |= c["negative_keys"] and not c["positive_keys"]
            rows["positive keys only"] |= c["positive_keys"] and not c["negative_keys"]
            rows["keys of both signs in one row"] |= c["negative_keys"] and c["positive_keys"]
            rows["-0.0 among the members"] |= c["negative_zero"]
            rows["select skipped (kmin == kmax)"] |= c["select_skipped"]
            rows["a wave adds its popcount once"] |= c["popcount_waves"] > 0
            rows["a wave adds lane by lane"] |= c["perlane_waves"] > 0
            rows["both counting paths in one pass"] |= c["both_paths_in_one_pass"]
            rows["the same in fp32 rows: both counting paths in one pass"] |= c["both_paths_in_one_pass"] and case.x.dtype == np.float32
            rows["a wave's first active lane is not lane 0"] |= c["first_lane_nonzero"]
            rows["a wave with no member at all"] |= c["wave_without_member"] and c["passes"] > 0
            rows["a rank at the first position of a run of ties"] |= c["rank_first_of_run"] and c["passes"] > 0
            rows["a rank at the last position of a run of ties"] |= c["rank_last_of_run"] and c["passes"] > 0
            rows["a rank inside a run of ties"] |= c["rank_inside_run"] and c["passes"] > 0
    missed = sorted(name for name, hit in rows.items() if not hit)
    assert not missed, ("no case reaches", missed)


def test_exact_moments_against_a_rational_sum():
    from fractions import Fraction
    v = np.array([0.1, -0.2, 1e150, 3.0, -1e150, 5e-324, 0.7])
    mean, std = BC.exact_moments(v)
    fr = [Fraction(float(t)) for t in v]
    mu = sum(fr) / len(fr)
    var = sum((t - mu) ** 2 for t in fr) / len(fr)
    assert mean == float(mu) and std == float(var) ** 0.5
    assert BC.exact_moments(np.full(9, 3.25)) == (3.25, 0.0)
