"""Host side of the reach integrals and the water balance (fs_batch_reach_integrals, fs_batch_water_balance): the trapezoid weights of
one row, the nodes a lane takes, the fold of the lanes and the walk over one reach's spans are the plain-C++ half of
flow-sim_amd/csrc/fs_balance.hpp.  tests/balance/balance_driver.cpp is built here with the system compiler under AddressSanitizer and
UBSan, run as a program on made-up rows and spans, and held to numpy.

The closure bound the balance rests on is asserted with numpy alone on the reference's stored histories: the Preissmann continuity
row is conservative, so the residual of one level is dt dx times the sum over the cells of the continuity residuals at the accepted
iterate, whose 2-norm the Newton tolerance bounds:  |residual_k| <= dt dx sqrt(N - 1) tolerance  (+ the rounding of the two volumes).
The bound is derived, not tuned.  ratio = max_k |residual_k| / (dt dx sqrt(N - 1) tolerance), measured with this file's formulas
(in brackets: the figures the bound was proposed with):

    gerd_full, gerd      N = 121   max |residual| 14.3 m3     ratio 0.361    (14.3, 0.361)
    bc_compound_normal   N = 41    6.4e-2                     3.4e-2         (6.4e-2, 3.4e-2)
    bc_trap_poly         N = 26    5.2e-3                     1.5e-3         (5.2e-3, 1.5e-3)
    c5_512 (two reaches) N = 512   1.3e-3, 1.1e-4             6.2e-5, 5.6e-6 (1.3e-3, 6.2e-5)
    c3_4096 (two)        N = 4096  5.8e-7, 5.1e-7             6.0e-8, 5.3e-8 (<= 5e-7, <= 5.4e-8: rounding noise, the bar there is 1e-3)
    akbari               N = 30    2.4e-9                     1.2e-12
    example              N = 21    1.4e-7                     8.6e-11
    bc_stage_fixed       N = 25    6.6e-10                    3.0e-10
    irr_levee (polyline) N = 11    2.6e-7                     5.5e-7"""
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from oracle import preissmann_oracle as O

import derived_reference as D
import host_driver

DRIVER = os.path.join(ROOT, "tests", "balance", "balance_driver.cpp")
NAN = float("nan")
LANES = 64
BAL_ROWS = ("spans", "first_level", "last_level", "storage_change", "net_inflow", "inflow", "residual", "worst", "worst_level", "relative")


# ---- the reference: numpy, written out ----
def lane_fold(t, V):
    """the sum of w_i t_i as the kernel adds it: lane l takes the packs p = l, l + 64 ... of V nodes in node order, then the xor tree"""
    n = len(t)
    w = np.ones(n); w[0] = w[-1] = 0.5
    part = np.zeros(LANES)
    for i in range(n):
        lane = (i // V) % LANES
        part[lane] = part[lane] + w[i] * t[i]
    m = LANES // 2
    while m >= 1:
        part = part + part[np.arange(LANES) ^ m]
        m //= 2
    return part[0]


def walk(ev, vol, qi, qo, theta, dt):
    """(totals dict, rows [m]) of one reach: spans between evaluated rows, level by level"""
    m = len(ev)
    rows = np.full(m, NAN)
    idx = [k for k in range(m) if ev[k]]
    tot = dict(spans=0.0, first_level=-1.0, last_level=-1.0, storage_change=NAN, net_inflow=0.0, inflow=0.0, residual=0.0, worst=NAN,
               worst_level=-1.0, relative=NAN)
    if not idx:
        return tot, rows
    rows[idx[0]] = 0.0
    res = []
    for a, b in zip(idx[:-1], idx[1:]):
        net = inn = 0.0
        for k in range(a + 1, b + 1):
            net += dt * (theta * (qi[k] - qo[k]) + (1.0 - theta) * (qi[k - 1] - qo[k - 1]))
            inn += dt * (theta * qi[k] + (1.0 - theta) * qi[k - 1])
        r = (vol[b] - vol[a]) - net
        rows[b] = r
        res.append(r)
        tot["net_inflow"] += net; tot["inflow"] += inn; tot["residual"] += r
    tot.update(spans=float(len(res)), first_level=float(idx[0]), last_level=float(idx[-1]), storage_change=vol[idx[-1]] - vol[idx[0]])
    if res:
        with np.errstate(invalid="ignore"):
            mag = np.abs(np.array(res))
            tot.update(worst=float(np.max(mag)), worst_level=float(idx[1:][int(np.argmax(mag))]), relative=tot["residual"] / tot["inflow"])
    return tot, rows


def row_cases():
    rng = np.random.default_rng(12)
    out = {}
    for n in (2, 3, 4, 63, 64, 65, 121, 127, 128, 129, 130, 257, 511):
        for V in (2, 4):
            out[f"ones_{n}_{V}"] = (np.ones(n), V)
            out[f"random_{n}_{V}"] = (rng.uniform(0.0, 5000.0, n), V)
    out["two_nodes"] = (np.array([3.0, 5.0]), 2)
    out["nan_node"] = (np.array([1.0, 2.0, NAN, 4.0, 5.0]), 2)
    out["halves_and_ones"] = ((rng.uniform(0, 1, 121) > 0.5).astype(float), 2)          # the terms of FS_INT_LENGTH_OVER
    return out


def balance_cases():
    rng = np.random.default_rng(7)

    def series(m):
        return rng.uniform(1e5, 2e5, m), rng.uniform(50.0, 500.0, m), rng.uniform(50.0, 500.0, m)
    out = {}
    v, qi, qo = series(8)
    out["every_level"] = (np.ones(8), v, qi, qo, 0.6, 300.0)
    out["theta_one"] = (np.ones(8), v, qi, qo, 1.0, 300.0)
    gap = np.ones(8); gap[3] = 0
    out["unevaluated_row_inside"] = (gap, v, qi, qo, 0.6, 300.0)
    vn = v.copy(); vn[4] = NAN
    out["nan_volume"] = (np.ones(8), vn, qi, qo, 0.6, 300.0)
    vn2 = v.copy(); vn2[4] = NAN
    out["nan_volume_in_an_unevaluated_row"] = (gap * (np.arange(8) != 4), vn2, qi, qo, 0.6, 300.0)
    v, qi, qo = series(11)
    out["every_3"] = ((np.arange(11) % 3 == 0).astype(float), v, qi, qo, 0.55, 600.0)      # marks at 0 3 6 9; level 10 is past the last
    out["every_3_late_start"] = ((np.arange(11) % 3 == 1).astype(float), v, qi, qo, 0.55, 600.0)
    v, qi, qo = series(2)
    out["failed_at_level_2"] = (np.ones(2), v, qi, qo, 0.6, 300.0)      # red_rows hands the walk the rows before the failing level
    v, qi, qo = series(1)
    out["one_row"] = (np.ones(1), v, qi, qo, 0.6, 300.0)
    out["no_row"] = (np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0), 0.6, 300.0)
    v, qi, qo = series(5)
    out["nothing_evaluated"] = (np.zeros(5), v, qi, qo, 0.6, 300.0)
    qn = qi.copy(); qn[2] = NAN
    out["nan_flow"] = (np.ones(5), v, qn, qo, 0.6, 300.0)
    # a balance that closes: the volumes are the integrated net inflow, exactly representable
    qi, qo = np.array([4.0, 8.0, 16.0, 8.0, 4.0]), np.array([4.0, 4.0, 8.0, 16.0, 8.0])
    net = 64.0 * (0.5 * (qi[1:] - qo[1:]) + 0.5 * (qi[:-1] - qo[:-1]))
    out["closes_exactly"] = (np.ones(5), 1024.0 + np.concatenate([[0.0], np.cumsum(net)]), qi, qo, 0.5, 64.0)
    return out


def numbers(a):
    return " ".join(repr(float(v)) for v in a)


@pytest.fixture(scope="module")
def driver_output(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("balance")
    exe = host_driver.build(DRIVER, tmp, extra_flags=["-ffp-contract=off"])
    lines = [f"W {name} {len(t)} {V} {numbers(t)}" for name, (t, V) in row_cases().items()]
    lines += [f"B {name} {len(ev)} {theta!r} {dt!r} {numbers(ev)} {numbers(vol)} {numbers(qi)} {numbers(qo)}"
              for name, (ev, vol, qi, qo, theta, dt) in balance_cases().items()]
    path = tmp / "records.txt"
    path.write_text("\n".join(lines) + "\n")
    got = {}
    for line in host_driver.run(exe, [path], timeout=60).splitlines():
        f = line.split()
        got[f[1]] = np.array([float(v) for v in f[2:]])
    assert len(got) == len(lines)
    return got


def same(a, b):
    return (np.isnan(a) and np.isnan(b)) or a == b


def test_every_node_of_a_row_goes_to_one_lane_once(driver_output):
    for name, (t, _) in row_cases().items():
        _, visited, most, same_bits = driver_output[name]
        assert (visited, most) == (len(t), 1), name
        assert same_bits == 1 or np.isnan(driver_output[name][0]), name


def test_rows_are_the_trapezoid_sum_in_the_kernels_order(driver_output):
    for name, (t, V) in row_cases().items():
        got = driver_output[name][0]
        assert same(got, lane_fold(t, V)), name                         # the same additions in the same order: the same bits
        if not np.isnan(got):
            w = np.ones(len(t)); w[0] = w[-1] = 0.5
            exact = math.fsum(w * t)
            assert abs(got - exact) <= (len(t) + 2) * 2.0 ** -53 * math.fsum(np.abs(w * t)), name
    assert driver_output["two_nodes"][0] == 4.0                          # half of each end
    assert driver_output["ones_121_2"][0] == 120.0 and driver_output["ones_2_4"][0] == 1.0
    assert np.isnan(driver_output["nan_node"][0])
    t = row_cases()["halves_and_ones"][0]
    assert driver_output["halves_and_ones"][0] == t.sum() - 0.5 * (t[0] + t[-1])      # halves and ones add exactly


def test_the_walk_over_the_spans_is_numpys(driver_output):
    for name, (ev, vol, qi, qo, theta, dt) in balance_cases().items():
        tot, rows = walk(ev, vol, qi, qo, theta, dt)
        got = driver_output[name]
        for i, key in enumerate(BAL_ROWS):
            assert same(got[i], tot[key]), (name, key, got[i], tot[key])
        assert all(same(g, w) for g, w in zip(got[len(BAL_ROWS):], rows)), (name, got[len(BAL_ROWS):], rows)


def test_spans_first_rows_and_gaps(driver_output):
    n = len(BAL_ROWS)
    got = driver_output["every_level"]
    assert tuple(got[:3]) == (7, 0, 7) and got[n] == 0.0 and not np.any(np.isnan(got[n:]))
    got = driver_output["unevaluated_row_inside"]
    assert tuple(got[:3]) == (6, 0, 7) and np.isnan(got[n + 3]) and not np.isnan(got[n + 4])      # the span 2 -> 4 covers two levels
    got = driver_output["every_3"]
    assert tuple(got[:3]) == (3, 0, 9) and np.flatnonzero(~np.isnan(got[n:])).tolist() == [0, 3, 6, 9]
    got = driver_output["every_3_late_start"]
    assert tuple(got[:3]) == (3, 1, 10) and got[n + 1] == 0.0
    got = driver_output["failed_at_level_2"]
    assert tuple(got[:3]) == (1, 0, 1)
    got = driver_output["one_row"]
    assert tuple(got[:3]) == (0, 0, 0) and got[3] == 0.0 and np.isnan(got[7]) and got[8] == -1 and got[n] == 0.0
    for name in ("no_row", "nothing_evaluated"):
        got = driver_output[name]
        assert tuple(got[:3]) == (0, -1, -1) and np.isnan(got[3]) and tuple(got[4:7]) == (0, 0, 0) and np.all(np.isnan(got[n:]))
    got = driver_output["closes_exactly"]
    assert np.all(got[n:] == 0.0) and got[6] == 0.0 and got[7] == 0.0 and got[9] == 0.0


def test_a_nan_volume_or_flow_stays_in_its_spans(driver_output):
    n = len(BAL_ROWS)
    got = driver_output["nan_volume"]
    assert np.flatnonzero(np.isnan(got[n:])).tolist() == [4, 5]                 # the span into the row and the span out of it
    assert np.isnan(got[6]) and np.isnan(got[7]) and got[8] == 4               # as np.max / np.argmax: the first NaN's level
    got = driver_output["nan_volume_in_an_unevaluated_row"]
    assert np.flatnonzero(np.isnan(got[n:])).tolist() == [3, 4] and not np.isnan(got[6])      # a volume nobody evaluated is not read
    got = driver_output["nan_flow"]
    assert np.flatnonzero(np.isnan(got[n:])).tolist() == [2, 3] and got[8] == 2


# ---- the closure bound, on the reference's stored histories ----
def fixture_members(name):
    """[(geo, depth [nt, N], flow, theta, dt, dx, tolerance)] of the reaches of one golden fixture"""
    fx, meta = O.load_fixture(os.path.join(GOLDEN, name + ".npz"))
    if fx["depth"].ndim == 3:
        return [({k: np.array(fx["geo_" + k][j], dtype=np.float64) for k in O.GEO_KEYS}, fx["depth"][j], fx["flow"][j], meta["theta"], meta["dt"],
                 meta["dx"], meta["tolerance"]) for j in range(fx["depth"].shape[0])]
    p = O.problem_from_fixture(fx, meta)
    return [(p.geo, np.array(fx["depth"]), np.array(fx["flow"]), p.theta, p.dt, p.dx, p.tol)]


CLOSURE = ("gerd_full", "gerd", "bc_compound_normal", "bc_trap_poly", "c5_512", "c3_4096", "akbari", "example", "bc_stage_fixed", "irr_levee")


@pytest.mark.parametrize("name", CLOSURE)
def test_the_stored_histories_close_within_the_newton_tolerance(name):
    """|residual_k| <= dt dx sqrt(N - 1) tolerance + 4 (N + 2) 2^-53 V at every level of every reach; the measured ratio is printed
    (the module's docstring holds the figures)."""
    for geo, h, Q, theta, dt, dx, tol in fixture_members(name):
        N = h.shape[1]
        A, _ = D.area_top(geo, h)
        w = np.ones(N); w[0] = w[-1] = 0.5
        V = np.array([dx * math.fsum(w * row) for row in A])
        net = Q[:, 0] - Q[:, -1]
        res = (V[1:] - V[:-1]) - dt * (theta * net[1:] + (1.0 - theta) * net[:-1])
        bound = dt * dx * math.sqrt(N - 1) * tol
        bar = 4 * (N + 2) * 2.0 ** -53 * np.maximum(V[1:], V[:-1])
        ratio = np.max(np.abs(res)) / bound
        print(f"{name}: N = {N}, max |residual| = {np.max(np.abs(res)):.3g} m3, ratio = {ratio:.3g}")
        assert np.all(np.abs(res) <= bound + bar), (name, ratio)
