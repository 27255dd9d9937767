"""bands_kernel (fs_reduce.hpp) and profile_bands_kernel (fs_envelope.hpp) on the adversarial rows of tests/band_cases.py, and the other
post-processing launchers on inputs no stepped batch produces - all through the probe library (tests/device_probe/probe_reduce.hip,
linked with the library's own objects: the kernels run here are the shipped machine code).

Per row (finite rows; a NaN or no member: every output NaN; an infinity: only what does not interpolate):
  exact    n_members, exceed, min, max, and every quantile whose virtual index (m - 1) q is an integer, against np.sort of the kept members
  exact    every other quantile, bit for bit against band_cases.quantile_lerp (plain float64 arithmetic on two exact order statistics),
           and within 4 eps max(|a|, |b|) of np.quantile
  mean     within (ceil(B / 256) + 9) eps sum|x| / m of the exactly rounded mean: ceil(B / 256) additions per thread, eight levels of
           the tree, one division
  std      within (ceil(B / 256) + 13) eps max|x| of the exactly rounded population standard deviation: the two-pass sum above plus
           the rounding of each x - mean and the square root
The row under test sits at one (level, signal) of a block of four levels; the seven other rows of the range hold unrelated data and
are held to the same assertions on their own data.

Worst measured share of the mean and std bars per family, on an MI355X (printed with -s as BAND family (x) | kernel | ...; for
bands the neighbour rows count too; 0.000: every partial sum of the family is exact).  Nothing was tightened to these:

  family                                   bands: mean  std      profile_bands: mean  std
  (a) uniform, mixed sign, to 32 769       0.086        0.036    0.019                0.037
  (b) 300 decades, lead == 0               0.086        0.021    0.082                0.007
  (c) base + k ulp, lead 1 .. 7            0.094        0.021    0.094                0.009
  (d) few values, long ties, to 32 769     0.086        0.023    0.000                0.020
  (e) one value, +-0, subnormals           0.075        0.012    0.000                0.000
  (f) equal waves between distinct waves   0.086        0.034    0.080                0.036
  (g) integers                             0.086        0.017    0.000                0.024
  (h) one NaN (neighbour rows only)        0.077        0.021    -                    -
  (i) +-inf (finite rows only)             0.077        0.021    0.006                0.034
  (j) fp32 rows                            0.000        0.034    0.000                0.036

Every derived bar held.  Found by family (i): with an infinite member the kernels returned NaN for the quantiles that are that member
itself (q = 1 above a +inf maximum: inf - inf) or its neighbour at an integer virtual index (inf * 0), as np.quantile does;
quantile_lerp now returns the order statistic where nothing is to be interpolated (finite rows: the same bits).
"""
import zlib

import numpy as np
import pytest

import band_cases as BC

pytestmark = pytest.mark.gpu
EPS = BC.EPS
LEVELS, LEVEL, FIRST, N_RANGE = 5, 3, 1, 2          # the block holds five levels, rows 0 .. 3 exist, the range is levels 1 and 2


@pytest.fixture(scope="module")
def P():
    import device_probe
    device_probe.lib()            # RuntimeError "probe library not built" fails the tests: no skip
    return device_probe


def same_bits(a, b):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes() == np.ascontiguousarray(b, dtype=np.float64).tobytes()


class Shares:
    """the worst share of the mean and std bars seen"""
    def __init__(self):
        self.mean = self.std = 0.0


def check_row(what, e, B, moments, quantiles, shares):
    """one row's outputs (moments [4], quantiles [n_q]) against band_cases.expected"""
    if e["none"]:
        assert np.all(np.isnan(moments)) and np.all(np.isnan(quantiles)), (what, moments, quantiles)
        return
    assert same_bits(moments[0], e["min"]) and same_bits(moments[1], e["max"]), (what, moments[:2], e["min"], e["max"])
    whole = e["integer"]
    assert same_bits(quantiles[whole], e["lo"][whole]), (what, "order statistics", e["q"][whole], quantiles[whole], e["lo"][whole])
    if not e["finite"]:
        return
    assert same_bits(quantiles, e["quantiles"]), (what, "quantile_lerp", e["q"], quantiles, e["quantiles"])
    if len(e["q"]):
        bar = 4 * EPS * np.maximum(np.abs(e["lo"]), np.abs(e["hi"]))
        assert np.all(np.abs(quantiles - np.quantile(e["sorted"], e["q"])) <= bar), (what, "np.quantile", e["q"])
    terms = -(-B // BC.THREADS)
    bar_mean, bar_std = (terms + 9) * EPS * e["abs_sum"] / e["m"], (terms + 13) * EPS * e["abs_max"]
    err_mean, err_std = abs(moments[2] - e["mean"]), abs(moments[3] - e["std"])
    if bar_mean > 0:
        shares.mean = max(shares.mean, err_mean / bar_mean)
    if bar_std > 0:
        shares.std = max(shares.std, err_std / bar_std)
    assert err_mean <= bar_mean, (what, "mean", moments[2], e["mean"], err_mean, bar_mean)
    assert err_std <= bar_std, (what, "std", moments[3], e["std"], err_std, bar_std)


# ---- fsp_bands ------------------------------------------------------------------------------------------------------------------
_FILLER, _STATS = {}, {}


def filler(B, D):
    """the block's unrelated data for B members of type D: every row its own magnitude and offset"""
    if (B, D) not in _FILLER:
        rng = np.random.default_rng(1000 + B)
        scale = 10.0 ** rng.uniform(-2, 3, (LEVELS, 4, 1))
        _FILLER[B, D] = (rng.standard_normal((LEVELS, 4, B)) * scale + scale * rng.uniform(-2, 2, (LEVELS, 4, 1))).astype(D)
    return _FILLER[B, D]


def stats_of(key, v):
    if key not in _STATS:
        _STATS[key] = BC.row_stats(v)
    return _STATS[key]


def where_of(case):
    """the (level, signal) of the range at which the case's row sits"""
    h = zlib.crc32(case.name.encode())
    return FIRST + h % N_RANGE, (h // N_RANGE) % 4


def run_bands(P, case, shares):
    D = case.x.dtype.type
    fill = filler(case.B, D)
    level, signal = where_of(case)
    hydro = fill.copy()
    hydro[level, signal] = case.x
    iters = np.ones((LEVELS, case.B), dtype=np.int32)
    kept = case.kept
    for qset in BC.Q_SETS:
        q = case.q(qset)
        got = P.bands(hydro, case.status, iters, LEVEL, FIRST, N_RANGE, q)
        assert np.array_equal(got["n_members"], np.full(N_RANGE, int(np.sum(kept)))), (case, got["n_members"])
        for lv in range(FIRST, FIRST + N_RANGE):
            for sg in range(4):
                if (lv, sg) == (level, signal):
                    e = BC.expected(None, q, stats_of(("case", case.name), case.values()))
                else:
                    e = BC.expected(None, q, stats_of(("fill", case.B, D, lv, sg, kept.tobytes()), fill[lv, sg][kept].astype(np.float64) + 0.0))
                check_row((case, qset, lv, sg, "under test" if (lv, sg) == (level, signal) else "neighbour"), e, case.B,
                          got["moments"][lv - FIRST, sg], got["quantiles"][lv - FIRST, sg], shares)


# ---- fsp_profile_bands ------------------------------------------------------------------------------------------------------------
def profile_inputs(case):
    """three nodes on the case's members.  Node 0 holds the case's row and leaves out the case's members, a third of them through the
    status, a third through levels == 0, a third through reach_nodes == 0.  Node 1 holds the row rolled by 37 and loses every seventh
    member more (reach_nodes == 1), node 2 holds it reversed and loses the second wave as well (reach_nodes == 2)."""
    B = case.B
    i = np.arange(B)
    out = ~case.kept
    x = np.ascontiguousarray(np.stack([case.x, np.roll(case.x, 37), case.x[::-1]]).astype(np.float64))
    status = np.where(out & (i % 3 == 0), case.status, np.where(case.kept, case.status, BC.OK)).astype(np.int32)
    levels = np.where(out & (i % 3 == 1), 0, 1 + i % 4).astype(np.int32)
    nodes = np.full(B, 3, dtype=np.int32)
    nodes[(i >= 64) & (i < 128)] = 2
    nodes[i % 7 == 3] = 1
    nodes[out & (i % 3 == 2)] = 0
    enters = [case.kept & (nodes > node) for node in range(3)]
    count = np.random.default_rng(zlib.crc32(case.name.encode()) ^ 5).integers(0, 3, (3, B)).astype(np.float64)
    return x, count, status, levels, nodes, enters


def run_profile(P, case, shares):
    x, count, status, levels, nodes, enters = profile_inputs(case)
    for qset in BC.Q_SETS:
        q = case.q(qset)
        got = P.profile_bands(x, count, status, levels, nodes, q)
        for node in range(3):
            m = int(np.sum(enters[node]))
            assert got["n_members"][node] == m, (case, node, got["n_members"][node], m)
            want = np.float64(np.sum(count[node][enters[node]] > 0)) / np.float64(m) if m else np.nan
            assert same_bits(got["exceed"][node], want), (case, node, got["exceed"][node], want)
            e = BC.expected(None, q, stats_of(("profile", case.name, node), x[node][enters[node]] + 0.0))
            check_row((case, qset, "node", node), e, case.B, got["moments"][node], got["quantiles"][node], shares)


@pytest.mark.parametrize("kernel", ["bands", "profile_bands"])
@pytest.mark.parametrize("family", BC.FAMILIES)
def test_band_kernels_on_adversarial_rows(P, family, kernel):
    shares = Shares()
    cases = [c for c in BC.ALL_CASES if c.family == family]
    assert cases
    try:
        for case in cases:
            (run_bands if kernel == "bands" else run_profile)(P, case, shares)
    finally:
        print(f"BAND family ({family}) | {kernel} | {len(cases)} rows | worst share of the mean bar {shares.mean:.3f} | of the std bar {shares.std:.3f}")


def test_profile_bands_without_counts_and_without_reach_nodes(P):
    case = next(c for c in BC.CASES_F64 if c.name == "f-blocks-B257-every2nd")
    x = np.ascontiguousarray(np.stack([case.x, case.x[::-1], -case.x]))
    levels = np.ones(case.B, dtype=np.int32)
    q = case.q("q16")
    got = P.profile_bands(x, None, case.status, levels, None, q)
    assert got["exceed"] is None
    for node in range(3):
        assert got["n_members"][node] == np.sum(case.kept)
        check_row((case, "plain", node), BC.expected(x[node][case.kept] + 0.0, q), case.B, got["moments"][node], got["quantiles"][node], Shares())


# ---- fsp_transpose_rows -------------------------------------------------------------------------------------------------------------
def test_transpose_rows_is_np_transpose(P):
    sizes = (1, 31, 32, 33, 65)
    rng = np.random.default_rng(11)
    for B in sizes:
        for N in sizes:
            rows = [rng.standard_normal((B, N)), rng.standard_normal((B, N))]
            rows[0][0, 0], rows[1][-1, -1] = -0.0, np.nan          # bit patterns, not values, are moved
            for n_rows in (1, 2):
                got = P.transpose_rows(rows[:n_rows])
                want = np.stack([np.ascontiguousarray(r.T) for r in rows[:n_rows]])
                assert got.shape == (n_rows, N, B) and got.tobytes() == want.tobytes(), (B, N, n_rows)


# ---- red_rows, through fsp_summarize and fsp_lookup ---------------------------------------------------------------------------------
def red_rows(status, iters, level, first, n, r):
    """the comment above red_rows (fs_reduce.hpp): a failed reach stops at the last level that holds a Newton count"""
    complete = level + 1
    if status[r] not in (BC.OK, BC.ILL_CONDITIONED):
        complete = max([k for k in range(1, level + 1) if iters[k, r] > 0], default=1)
    return min(max(complete - first, 0), n)


STORAGE_RANGE = 3
# (status, failing level or None): the Newton counts are positive up to and including the failing level and 0 after it
REACHES = [(BC.OK, None), (BC.NAN, 1), (BC.MAX_ITER, 5), (BC.NAN, 0), (BC.ILL_CONDITIONED, None), (BC.MAX_ITER, 3), (STORAGE_RANGE, 2), (BC.OK, None)]
RANGES = [(0, 6), (0, 1), (1, 3), (3, 3), (4, 2), (5, 1), (2, 1), (3, 1), (1, 1), (2, 4)]


def synthetic_block(D):
    L, B = 6, len(REACHES)
    status = np.array([s for s, _ in REACHES], dtype=np.int32)
    iters = np.full((L, B), 3, dtype=np.int32)
    iters[0] = 0                                          # level 0 is the initial state: no Newton count
    for r, (_, fail) in enumerate(REACHES):
        if fail is not None:
            iters[fail + 1:, r] = 0
            if fail == 0:
                iters[:, r] = 0                           # a failed reach whose counts are all zero
    k = np.arange(L, dtype=np.float64)[:, None]
    r = np.arange(B, dtype=np.float64)[None, :]
    hydro = np.empty((L, 4, B), dtype=D)
    hydro[:, 0] = 2.0 + 0.25 * k + 0.0 * r                # depth in: rises with the level
    hydro[:, 1] = 10.0 * k + r                            # flow in: the level can be read off a clamped lookup
    hydro[:, 2] = 3.0 - 0.125 * k + 0.0 * r
    hydro[:, 3] = 5.0 + k * k + r
    return hydro, status, iters


@pytest.mark.parametrize("D", [np.float64, np.float32], ids=["f64", "f32"])
def test_red_rows_on_synthetic_status_and_newton_counts(P, D):
    hydro, status, iters = synthetic_block(D)
    L, B = iters.shape
    level = L - 1
    assert red_rows(status, iters, level, 0, 6, 3) == 1 and red_rows(status, iters, level, 0, 6, 1) == 1          # counts all zero / failure at level 1
    assert red_rows(status, iters, level, 0, 6, 2) == 5 and red_rows(status, iters, level, 0, 6, 4) == 6          # last level / a warning only
    assert [red_rows(status, iters, level, f, n, 5) for f, n in ((1, 3), (3, 3), (4, 2))] == [2, 0, 0]          # before, at, after level 3
    for first, n in RANGES:
        want = np.array([red_rows(status, iters, level, first, n, r) for r in range(B)], dtype=np.float64)
        s = P.summarize(hydro, status, iters, level, first, n)
        assert same_bits(s[0], want), (first, n, s[0], want)
        # the last flow a reach completed, through a lookup beyond the end of its series; no row: NaN
        got = P.lookup(hydro, status, iters, level, first, n, 0, 1, np.array([1e9]))
        last = np.array([hydro[first + int(m) - 1, 1, r] if m > 0 else np.nan for r, m in enumerate(want)], dtype=np.float64)
        assert same_bits(got["values"][0], last), (first, n, got["values"][0], last)
        assert np.array_equal(got["info"], np.zeros(B, dtype=np.int32))
        # peaks of the rows that entered, no more: the flow out rises with the level, so its peak level is the last row's
        assert same_bits(s[7], np.where(want > 0, want - 1, -1.0)), (first, n, s[7])
    # a lower current level hides the rows above it, whatever they hold
    s = P.summarize(hydro, status, iters, 2, 0, 3)
    assert same_bits(s[0], np.array([red_rows(status, iters, 2, 0, 3, r) for r in range(B)], dtype=np.float64))


# ---- fsp_lookup / fsp_summarize on series no stepped batch produces -----------------------------------------------------------------
SERIES_X = {
    "repeated": [0.0, 1.0, 1.0, 2.0, 2.0, 2.0, 3.0, 4.0],
    "rising": [-3.0, -2.5, -1.0, 0.5, 0.75, 2.0, 3.5, 4.0],
    "descending": [4.0, 3.0, 2.5, 2.0, 1.0, 0.5, 0.25, 0.0],
    "dip": [0.0, 1.0, 2.0, 1.5, 3.0, 4.0, 5.0, 6.0],
    "flat": [2.0] * 8,
}
QUERIES = [-5.0, -3.0, 0.0, 0.3, 1.0, 1.7, 2.0, 2.0000000001, 3.0, 3.9, 4.0, 7.0, np.nan]


@pytest.mark.parametrize("D", [np.float64, np.float32], ids=["f64", "f32"])
def test_lookup_and_summarize_on_series_of_the_tests_choosing(P, D):
    names = list(SERIES_X)
    L, B = 8, len(names)
    rng = np.random.default_rng(3)
    hydro = np.empty((L, 4, B), dtype=D)
    for r, name in enumerate(names):
        hydro[:, 0, r] = SERIES_X[name]
    hydro[:, 1] = -rng.uniform(1.0, 50.0, (L, B))         # negative flows throughout
    hydro[:, 2] = rng.uniform(0.5, 3.0, (L, B))
    hydro[:, 3] = -rng.uniform(1.0, 50.0, (L, B))
    status = np.zeros(B, dtype=np.int32)
    iters = np.ones((L, B), dtype=np.int32)
    xq = np.array(QUERIES)
    target = rng.uniform(-50.0, -1.0, 7)          # fewer than eight pairs: np.mean adds them in order, as mean_square_series does
    for first, n in ((0, 8), (2, 5), (3, 1)):             # (3, 1): m = 1, the only sample whatever the query
        got = P.lookup(hydro, status, iters, L - 1, first, n, 0, 1, xq)
        fin = P.lookup(hydro, status, iters, L - 1, first, n, 0, 1, xq[:7], target=target)
        assert same_bits(fin["values"], got["values"][:7])
        for r, name in enumerate(names):
            xp, fp = hydro[first:first + n, 0, r].astype(np.float64), hydro[first:first + n, 1, r].astype(np.float64)
            assert got["info"][r] == int(np.any(np.diff(xp) < 0)), (name, first, n)
            v = got["values"][:, r]
            assert np.isnan(v[-1])                        # the NaN query
            if got["info"][r]:
                continue                                  # a series that descends: the flag only
            want = np.interp(xq[:-1], xp, fp)
            exact = (xq[:-1] <= xp[0]) | (xq[:-1] >= xp[-1]) | np.isin(xq[:-1], xp)          # clamps and hits on a sample, a repeated one included
            assert same_bits(v[:-1][exact], want[exact]), (name, first, n, v[:-1], want)
            assert np.all(np.abs(v[:-1] - want) <= 8 * EPS * np.max(np.abs(fp))), (name, first, n, v[:-1], want)
            rmse = np.sqrt(np.mean((want[:7] - target) ** 2))
            assert abs(fin["rmse"][r] - rmse) <= 8 * EPS * rmse, (name, first, n)
        s = P.summarize(hydro, status, iters, L - 1, first, n)
        for r in range(B):
            cols = [hydro[first:first + n, c, r].astype(np.float64) for c in range(4)]
            assert s[0, r] == n
            for row, col in ((4, cols[1]), (6, cols[3]), (8, cols[0]), (10, cols[2])):
                assert s[row, r] == np.max(col) and s[row + 1, r] == np.argmax(col), (r, row, first, n)          # first index of the maximum, ties included
            for row, terms in ((1, cols[1]), (2, cols[3]), (3, cols[1] - cols[3])):
                assert abs(s[row, r] - np.sum(terms)) <= n * EPS * np.sum(np.abs(terms)), (r, row, first, n)
            for row, qcol in ((12, cols[1]), (13, cols[3])):
                # solver.py:219-229 as written, on negative flows: the first i with sum(Q[:i]) >= half of sum(Q[:m-1]); i = 0 passes
                cum = [np.sum(qcol[:i]) for i in range(n)]
                assert s[row, r] == next(i for i in range(n) if cum[i] >= 0.5 * cum[-1]) == 0, (r, row, first, n)
    # m = 0: a failed reach and a range beyond its failing level
    status[1] = BC.NAN
    iters[3:, 1] = 0
    got = P.lookup(hydro, status, iters, L - 1, 4, 3, 0, 1, xq)
    assert np.all(np.isnan(got["values"][:, 1])) and got["info"][1] == 0
    s = P.summarize(hydro, status, iters, L - 1, 4, 3)
    assert s[0, 1] == 0 and s[1, 1] == 0 and np.isnan(s[4, 1]) and s[5, 1] == -1 and s[12, 1] == -1
    assert np.all(s[0, [0, 2, 3, 4]] == 3)
