"""Host side of fs_batch_assimilate: what the host can refuse, the layouts of the partial sums and of the outputs, and the coefficients
of the analysis (anomalies, innovation covariance, its square-root-free Cholesky factor, Z = C^-1 D) are the plain-C++ half of
flow-sim_amd/csrc/fs_assim.hpp.  tests/assim/assim_driver.cpp is built here with the system compiler under AddressSanitizer and UBSan
and run as a program on made-up records; nothing is loaded into python.

analysis_coefficients is held bit for bit to the sequential Python restatement of tests/assim_checks.py (which the device is held to
as well, tests/test_gpu_assimilate.py).  The restatement itself is held to numpy.linalg.solve within kappa_1(C) m 2^-52 max|Z|, its
moments and update to math.fsum within bars counted from the additions, and the whole analysis to the textbook form
x + P H^T (H P H^T + R)^-1 (d - H x) on the example of the prototype."""
import math
import os

import numpy as np
import pytest

from conftest import ROOT

import assim_checks as K
import host_driver

DRIVER = os.path.join(ROOT, "tests", "assim", "assim_driver.cpp")
NAN, INF = float("nan"), float("inf")
U = 2.0 ** -53


def numbers(a):
    return " ".join(repr(float(v)) for v in np.asarray(a, dtype=np.float64).ravel())


def check_cases():
    """name -> (n_obs, n_gauges, B, N, null, floor, gauge, signal, value, variance, perturb, taper, text or None)"""
    B, N = 3, 4
    ok = dict(n_obs=2, n_gauges=3, null=0, floor=1e-3, gauge=[0, 2], signal=[2, 1], value=[412.5, -30.0], variance=[0.01, 25.0], perturb=None, taper=None)
    at = lambda j: f" (observation {j})"
    edits = {
        "good": ({}, None),
        "good_with_everything": (dict(perturb=np.linspace(-1, 1, 6), taper=[0.0, 1.0, 0.5, 1.0, 1.0, 0.0, 0.25, 1.0], floor=0.0), None),
        "the_most": (dict(n_obs=16, gauge=[1] * 16, signal=[3] * 16, value=[1.0] * 16, variance=[1e-300] * 16), None),
        "none": (dict(n_obs=0, gauge=[], signal=[], value=[], variance=[]), "entry: n_obs must be 1 .. 16, not 0"),
        "negative_count": (dict(n_obs=-2, gauge=[], signal=[], value=[], variance=[]), "entry: n_obs must be 1 .. 16, not -2"),
        "too_many": (dict(n_obs=17, gauge=[0] * 17, signal=[0] * 17, value=[1.0] * 17, variance=[1.0] * 17), "entry: n_obs must be 1 .. 16, not 17"),
        "null": (dict(null=1), "entry: null gauge, signal, value or variance"),
        "gauge_negative": (dict(gauge=[-1, 0]), "entry: gauge -1 is not one of 0 .. 2" + at(0)),
        "gauge_beyond": (dict(gauge=[0, 3]), "entry: gauge 3 is not one of 0 .. 2" + at(1)),
        "signal_negative": (dict(signal=[0, -1]), "entry: signal -1 is not one of FS_GAUGE_DEPTH .. FS_GAUGE_VELOCITY (0 .. 3)" + at(1)),
        "signal_beyond": (dict(signal=[4, 0]), "entry: signal 4 is not one of FS_GAUGE_DEPTH .. FS_GAUGE_VELOCITY (0 .. 3)" + at(0)),
        "variance_zero": (dict(variance=[0.0, 1.0]), "entry: variances must be finite and > 0" + at(0)),
        "variance_negative": (dict(variance=[1.0, -1.0]), "entry: variances must be finite and > 0" + at(1)),
        "variance_nan": (dict(variance=[NAN, 1.0]), "entry: variances must be finite and > 0" + at(0)),
        "variance_inf": (dict(variance=[1.0, INF]), "entry: variances must be finite and > 0" + at(1)),
        "value_nan": (dict(value=[1.0, NAN]), "entry: values must be finite" + at(1)),
        "value_inf": (dict(value=[-INF, 1.0]), "entry: values must be finite" + at(0)),
        "perturb_nan": (dict(perturb=[0.0, 0.0, 0.0, 0.0, NAN, 0.0]), "entry: perturbations must be finite (observation 1, member 1)"),
        "perturb_inf": (dict(perturb=[0.0, 0.0, INF, 0.0, 0.0, 0.0]), "entry: perturbations must be finite (observation 0, member 2)"),
        "taper_above": (dict(taper=[1.0] * 7 + [1.0 + 2.0 ** -52]), "entry: tapers must be finite and in [0, 1] (observation 1, node 3)"),
        "taper_below": (dict(taper=[-1e-300] + [1.0] * 7), "entry: tapers must be finite and in [0, 1] (observation 0, node 0)"),
        "taper_nan": (dict(taper=[1.0] * 5 + [NAN, 1.0, 1.0]), "entry: tapers must be finite and in [0, 1] (observation 1, node 1)"),
        "taper_minus_zero": (dict(taper=[-0.0] * 8), None),
        "floor_negative": (dict(floor=-1e-9), "entry: depth_floor must be finite and >= 0"),
        "floor_nan": (dict(floor=NAN), "entry: depth_floor must be finite and >= 0"),
        "floor_inf": (dict(floor=INF), "entry: depth_floor must be finite and >= 0"),
    }
    out = {}
    for name, (edit, text) in edits.items():
        c = dict(ok, **edit)
        out[name] = (c, B, N, text)
    return out


def analysis_cases():
    """name -> (y [m, B], active [B], value, variance, perturb or None, refused text or None)"""
    rng = np.random.default_rng(5)
    out = {}

    def case(name, m, B, inactive=(), perturb=False, scale=1.0):
        y = 400.0 + scale * rng.normal(0.0, 1.0, (m, B)) + np.arange(m)[:, None] * 3.0
        active = np.ones(B, dtype=bool); active[list(inactive)] = False
        y[:, ~active] = NAN                                                          # not read: the driver counts the reads
        out[name] = (y, active, 400.0 + rng.normal(0, 1, m) + np.arange(m) * 3.0, rng.uniform(0.01, 0.5, m), rng.normal(0, 0.3, (m, B)) if perturb else None, None)

    case("one_observation", 1, 9)
    case("three", 3, 40, perturb=True)
    case("sixteen", 16, 64, perturb=True)
    case("sixteen_plain", 16, 40)
    case("inactive_front", 3, 12, inactive=(0, 1), perturb=True)
    case("inactive_middle", 3, 130, inactive=(4, 77))
    case("inactive_end", 1, 12, inactive=(11,), perturb=True)
    case("two_active", 3, 6, inactive=(0, 2, 3, 5), perturb=True)
    case("two_members", 1, 2)
    case("across_a_chunk", 3, 300, inactive=(255, 256), perturb=True)
    y = np.array([[-2.0, 0.0, 2.0], [-2.0, 0.0, 2.0]])                             # S S^T / 2 = 4 everywhere; 4 + 1e-30 is 4: the second pivot is 0
    out["not_positive_definite"] = (y, np.ones(3, dtype=bool), [0.0, 0.0], [1e-30, 1e-30], None,
                                    "entry: the innovation covariance is not positive definite (pivot 1 of its Cholesky factor)")
    out["one_active"] = (np.array([[1.0, 2.0, 3.0]]), np.array([False, True, False]), [0.0], [1.0], None,
                         "entry: 1 active member(s): an analysis needs at least two members that hold every observed gauge")
    out["nobody"] = (np.array([[1.0, 2.0]]), np.array([False, False]), [0.0], [1.0], None,
                     "entry: 0 active member(s): an analysis needs at least two members that hold every observed gauge")
    out["nan_in_an_active_member"] = (np.array([[1.0, 2.0, 3.0], [1.0, NAN, 2.0]]), np.ones(3, dtype=bool), [0.0, 0.0], [1.0, 1.0], None,
                                      "entry: member 1 holds a NaN in observation 1")
    out["overflowing_pivot"] = (np.array([[-1e200, 0.0, 1e200]]), np.ones(3, dtype=bool), [0.0], [1.0], None,
                                "entry: the innovation covariance is not positive definite (pivot 0 of its Cholesky factor)")
    return out


@pytest.fixture(scope="module")
def driver_output(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("assim")
    exe = host_driver.build(DRIVER, tmp, extra_flags=["-ffp-contract=off"])
    lines = []
    for name, (c, B, N, _) in check_cases().items():
        count = len(c["gauge"])
        lines.append(f"K {name} {c['n_obs']} {count} {c['n_gauges']} {B} {N} {c['null']} {int(c['perturb'] is not None)} {int(c['taper'] is not None)} "
                     f"{c['floor']!r} {numbers(c['gauge'])} {numbers(c['signal'])} {numbers(c['value'])} {numbers(c['variance'])} "
                     f"{numbers(c['perturb'] if c['perturb'] is not None else [])} {numbers(c['taper'] if c['taper'] is not None else [])}")
    lines += ["L big 8192 4096 16 31 1 17 15 8191", "L small 600 121 3 2 0 4 2 599", "L one 2 2 1 0 1 2 0 1", "L five 257 5 5 1 1 0 4 256"]
    for name, (y, active, value, variance, perturb, _) in analysis_cases().items():
        m, B = y.shape
        lines.append(f"A {name} {m} {B} {int(perturb is not None)} {numbers(active)} {numbers(y)} {numbers(value)} {numbers(variance)} "
                     f"{numbers(perturb if perturb is not None else [])}")
    path = tmp / "records.txt"
    path.write_text("\n".join(lines) + "\n")
    got = {}
    for line in host_driver.run(exe, [path], timeout=120).splitlines():
        kind, name, rest = (line.split(" ", 2) + [""])[:3]
        got[(kind, name)] = rest
    assert len(got) == len(lines)
    return got


def test_every_branch_of_the_validation(driver_output):
    for name, (_, _, _, text) in check_cases().items():
        assert driver_output[("K", name)] == (text or "ok"), name


def test_the_layouts(driver_output):
    for name, (B, N, m, chunk, field, row, j, r) in dict(big=(8192, 4096, 16, 31, 1, 17, 15, 8191), small=(600, 121, 3, 2, 0, 4, 2, 599),
                                                         one=(2, 2, 1, 0, 1, 2, 0, 1), five=(257, 5, 5, 1, 1, 0, 4, 256)).items():
        got = [int(v) for v in driver_output[("L", name)].split()]
        chunks = -(-B // 256)
        bucket = next(k for k in (1, 2, 4, 8, 16) if k >= m)
        want = [chunks, m + 2, chunks * 2 * (m + 2) * N, int(np.ravel_multi_index((chunk, field, row, 0), (chunks, 2, m + 2, N))), 4 * N,
                int(np.ravel_multi_index((2 * field + 1, 0), (4, N))), 2 * m * N, int(np.ravel_multi_index((field, j, 0), (2, m, N))), bucket, B * bucket,
                r * bucket]
        assert got == want, name


def test_the_coefficients_are_the_restatement_bit_for_bit(driver_output):
    for name, (y, active, value, variance, perturb, text) in analysis_cases().items():
        fields = driver_output[("A", name)].split(" ", 2)
        if text is not None:
            assert fields[0] == "refused" and fields[2] == text and int(fields[1]) == int(np.sum(active)), (name, fields)
            with pytest.raises(K.Refused):
                K.coefficients(y, active, value, variance, perturb)
            continue
        assert fields[0] == "ok", (name, fields[:2])
        v = fields[2].split() if len(fields) > 2 else []
        rest = [fields[1]] + v
        na, stray, nums = int(rest[0]), int(rest[1]), np.array([float(x) for x in rest[2:]])
        m, B = y.shape
        want = K.coefficients(y, active, value, variance, perturb)
        assert na == want["n_active"] == int(np.sum(active)) and stray == 0, name     # an inactive member's sample is not read
        sizes = [m, m * B, m * m, m * m, m * B]
        assert len(nums) == sum(sizes), name
        parts = np.split(nums, np.cumsum(sizes)[:-1])
        for got, key in zip(parts, ("ybar", "S", "C", "L", "Z")):
            assert K.same(got, want[key].ravel()), (name, key, np.max(np.abs(got - want[key].ravel())))
        assert np.all(want["S"][:, ~np.asarray(active)] == 0.0) and np.all(want["Z"][:, ~np.asarray(active)] == 0.0), name
        assert np.all(np.triu(want["L"], 1) == 0.0), name


def test_the_restatement_is_numpys_solve_within_the_bar_of_the_condition_number():
    """kappa_1(C) m 2^-52 max|Z|: the forward error of a backward-stable solve of an m x m system"""
    held = 0
    for name, (y, active, value, variance, perturb, text) in analysis_cases().items():
        if text is not None:
            continue
        co = K.coefficients(y, active, value, variance, perturb)
        m, B = y.shape
        kappa = np.linalg.cond(co["C"], 1)
        assert kappa <= 1e6, (name, kappa)
        act = np.flatnonzero(active)
        D = np.asarray(value)[:, None] + (perturb[:, act] if perturb is not None else 0.0) - y[:, act]
        ref = np.linalg.solve(co["C"], D)
        bar = kappa * m * K.EPS * np.max(np.abs(ref))
        err = np.max(np.abs(co["Z"][:, act] - ref))
        print(f"{name}: kappa_1 {kappa:.3g}  max|Z| {np.max(np.abs(ref)):.3g}  err {err:.3g}  bar {bar:.3g}")
        assert err <= bar, (name, err, bar)
        unit = np.tril(co["L"], -1) + np.eye(m)
        assert np.allclose(unit @ np.diag(np.diag(co["L"])) @ unit.T, co["C"], rtol=1e-12, atol=0)
        held += 1
    assert held >= 10


def moment_problem(B, N, m, inactive, seed):
    rng = np.random.default_rng(seed)
    active = np.ones(B, dtype=bool); active[list(inactive)] = False
    x = 400.0 + rng.normal(0.0, 1.5, (B, N))
    S = rng.normal(0.0, 1.0, (m, B)); S[:, ~active] = 0.0
    return x, active, S


@pytest.mark.parametrize("B,N,m,inactive", [(2, 3, 1, ()), (130, 7, 3, (4, 77)), (257, 5, 3, (0, 256)), (600, 4, 16, (255, 256, 599))])
def test_the_restated_moments_are_fsums_within_the_bar_of_their_additions(B, N, m, inactive):
    """a sequential (or chunked) sum of n rounded terms is within n 2^-53 sum|t| of math.fsum of the exact terms, to first order: (n - 1)
    additions and one rounding of each product; the quotients and the last differences add 2^-53 of their operands each"""
    x, active, S = moment_problem(B, N, m, inactive, 11)
    mean, var, P = K.moments(x, active, S)
    act = np.flatnonzero(active)
    n, c = len(act), x[act[0]]
    for i in range(N):
        d = [float(x[r, i] - c[i]) for r in act]                                     # the subtraction is the restatement's own: its terms
        s1, abs1 = math.fsum(d), math.fsum(abs(v) for v in d)
        s2 = math.fsum(np.longdouble(v) * np.longdouble(v) for v in d)
        ref_mean = float(np.longdouble(c[i]) + np.longdouble(s1) / n)
        bar_mean = n * U * abs1 / n + 2 * U * abs(ref_mean)
        assert abs(mean[i] - ref_mean) <= bar_mean, (i, mean[i] - ref_mean, bar_mean)
        ref_var = float((np.longdouble(s2) - np.longdouble(s1) * np.longdouble(s1) / n) / (n - 1))
        bar_s1sq = 2 * abs(s1) * n * U * abs1 / n + 2 * U * s1 * s1 / n
        bar_var = (n * U * float(s2) + bar_s1sq + U * (float(s2) + s1 * s1 / n)) / (n - 1) + U * abs(ref_var)
        assert abs(var[i] - ref_var) <= bar_var, (i, var[i] - ref_var, bar_var)
        assert abs(var[i] - np.var(x[act, i], ddof=1)) <= bar_var + 4 * n * U * float(s2) / (n - 1)     # numpy's own pairwise sums
        for j in range(m):
            t = [np.longdouble(v) * np.longdouble(S[j, r]) for v, r in zip(d, act)]
            ref = float(math.fsum(t) / (n - 1))
            bar = n * U * float(math.fsum(abs(v) for v in t)) / (n - 1) + U * abs(ref)
            assert abs(P[j, i] - ref) <= bar, (i, j, P[j, i] - ref, bar)


def test_the_restated_update_is_the_long_double_sum_within_the_bar_of_its_additions():
    rng = np.random.default_rng(12)
    B, N, m = 5, 9, 16
    active = np.array([True, False, True, True, True])
    xk = rng.uniform(0.5, 3.0, (B, N)); xg = xk + rng.normal(0, 1e-3, (B, N))
    P, Z, taper = rng.normal(0, 1, (m, N)), rng.normal(0, 1, (m, B)), rng.uniform(0, 1, (m, N))
    for tp in (None, taper):
        nk, ng, clamped = K.update(xk, xg, active, P, Z, tp, np.float64, floor=0.0)
        assert K.same(nk[1], xk[1]) and K.same(ng[1], xg[1])                        # the inactive member keeps every bit
        for r in np.flatnonzero(active):
            terms = np.array([(np.longdouble(1.0 if tp is None else tp[j]) * np.longdouble(P[j])) * np.longdouble(Z[j, r]) for j in range(m)])
            inc = terms.sum(axis=0)
            bar = 3 * m * U * np.abs(terms).sum(axis=0).astype(np.float64)           # two roundings per term and one per addition
            for old, new in ((xk, nk), (xg, ng)):
                ref = (np.longdouble(old[r]) + inc).astype(np.float64)
                low = ref < 0.0
                assert np.all(np.abs(new[r] - ref)[~low] <= (bar + U * np.abs(ref))[~low]), r
                assert np.all(new[r][low & (np.abs(ref) > bar)] == 0.0)
            assert clamped[r] == int(np.sum(nk[r] == 0.0))


def test_the_example_of_the_prototype_is_the_textbook_analysis():
    """B = 130 with members 4 and 77 inactive, N = 7; a stage between nodes 2 and 3 at weight 0.25, a flow at node 5, a depth at node 0:
    all three are linear in (h, Q), so the restated analysis is x + P H^T (H P H^T + R)^-1 (d - H x), to 1e-12 relative"""
    rng = np.random.default_rng(1999)
    B, N = 130, 7
    active = np.ones(B, dtype=bool); active[[4, 77]] = False
    z = 400.0 - 0.1 * np.arange(N)
    h = 2.0 + 0.3 * rng.standard_normal((B, 1)) + 0.05 * rng.standard_normal((B, N))
    Q = 50.0 + 5.0 * rng.standard_normal((B, 1)) + 0.5 * rng.standard_normal((B, N))
    H = np.zeros((3, 2 * N))
    H[0, 2], H[0, 3] = 0.75, 0.25
    H[1, N + 5] = 1.0
    H[2, 0] = 1.0
    offset = np.array([0.75 * z[2] + 0.25 * z[3], 0.0, 0.0])
    X = np.concatenate([h, Q], axis=1)
    stage = h + z
    y = np.stack([stage[:, 2] + 0.25 * (stage[:, 3] - stage[:, 2]), Q[:, 5], h[:, 0]])
    value, variance = np.array([402.0, 53.0, 2.2]), np.array([0.01, 4.0, 0.0025])
    perturb = rng.standard_normal((3, B)) * np.sqrt(variance)[:, None]
    got = K.analysis(y, active, h, Q, h, Q, value, variance, perturb, None, floor=0.0)
    want = K.textbook(X, H, value - offset, variance, perturb, active)
    new = np.concatenate([got["hk"], got["Qk"]], axis=1)
    rel = np.max(np.abs(new - want) / np.maximum(np.abs(want), 1.0))
    print(f"restatement against the textbook form: {rel:.3g} relative")
    assert rel <= 1e-12, rel
    assert got["n_active"] == 128 and K.same(new[[4, 77]], X[[4, 77]]) and not np.any(got["clamped"])
    assert np.max(np.abs(new[active] - X[active])) > 1e-3                            # and it is an analysis: the members moved
