"""Reach integrals and the discrete water balance on the device (flow-sim_amd/csrc/fs_balance.hpp: fs_batch_reach_integrals,
fs_batch_water_balance, fs_batch_integral_bands).

Integrals.  The reference is the path the library had before: fs_batch_derive's downloaded area, top width and level, and numpy on
them with exact summation (math.fsum).  The kernel evaluates A_i, T_i and h_i + z_i by derive's own lines, so what is compared is the
weighting and the sum.  Bar per row: (N_r + 2) 2^-53 dx_r sum_i w_i |term_i| - N_r additions, the product with dx and one unit for a
last-bit difference of a term.  FS_INT_LENGTH_OVER is exact: its terms are halves and ones, and the threshold is held against the
same h_i + z_i bits (thresholds are put ON samples, next to them and NaN).
Shapes: N in 2, 3, 63, 64, 65, 121, 127, 128, 129, 257 - one lane, the wave's edge, odd rows (every other row starts off a 16-byte
boundary), short last packs, the second trip of a lane - and B in 1, 5, 130.

Same bits (uint64 view): the current-state evaluation against the history row of the same level; a reach alone against the same reach
at place 77 of 130; one call over a range against two calls over its halves; a second run against the first.

Closure.  Stepped fp64 batches are held per level to the derived bound  dt dx sqrt(N - 1) tolerance  plus the rounding bar
4 (N + 2) 2^-53 V of the two volumes, with the device's own rows (tests/test_balance_host.py derives the bound and holds the
reference's stored histories to it).  fp32 batches: the closure is printed, not held - nothing bounds how the float areas evaluated
here relate to those of the step kernel's residual.
"""
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN
import band_cases as BC
from failure_recipes import K_STAR, edited
from fixture_batch import batch_from_problems, per_reach_polyline_batch
from flowsim_amd import _abi as A
from flowsim_amd.batch import BoundarySpec, PreissmannBatch
from oracle import preissmann_oracle as O
from synth import rect_problem

pytestmark = pytest.mark.gpu

EPS53 = 2.0 ** -53
SIZES = (2, 3, 63, 64, 65, 121, 127, 128, 129, 257)
NAN = float("nan")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_rows(a, b, names=("volume", "surface", "length_over")):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in names)


def weights(n):
    w = np.ones(n)
    w[0] = w[-1] = 0.5
    return w


def fixture_problem(name):
    fx, meta = O.load_fixture(os.path.join(GOLDEN, name + ".npz"))
    return O.problem_from_fixture(fx, meta)


# ---- batches that are not stepped: geometry, scheme and a state of the test's choosing ----------------------------------------------
def depths(rng, B, N, scale=4.0):
    """[B, N]: wet, dry (exactly 0) and negative depths, over-bank ones, and one NaN in the last reach that has room for it"""
    h = rng.uniform(0.05, scale, (B, N))
    h[rng.uniform(0, 1, (B, N)) < 0.1] = 0.0
    h[rng.uniform(0, 1, (B, N)) < 0.1] *= -1.0
    if N >= 3:
        h[B - 1, N // 2] = NAN
    return h


def uniform_batch(mode, B, N, dtype, rng, nodes=None, dx=None):
    b = PreissmannBatch(B, N, 2, dtype=dtype, section_mode=mode, history=True)
    b.set_scheme(0.6, 600.0, 250.0, 1e-6, 100)
    kw = dict(side_slope=rng.uniform(0.5, 2.5, B)) if mode == "trap_uniform" else {}
    b.set_geometry_uniform(rng.uniform(20.0, 200.0, B), np.full(B, 0.03), rng.uniform(3.0, 9.0, B), rng.uniform(0.0, 1.0, B), **kw)
    if nodes is not None:
        b.set_reach_nodes(nodes)
    if dx is not None:
        b.set_reach_scheme(dx=dx)
    return b


def compound_geo(rng, lead, N):
    """table rows [*lead, N]: trapezoids, every other node compound with floodplains that the deeper depths of depths() reach"""
    shape = tuple(lead) + (N,)
    geo = {k: np.zeros(shape) for k in A.GEO_ROWS}
    geo["z_bed"] = np.broadcast_to(np.linspace(5.0, 0.0, N), shape) + rng.uniform(0.0, 0.2, shape)
    geo["b_main"] = rng.uniform(20.0, 60.0, shape)
    geo["m_main"] = rng.uniform(0.0, 2.0, shape)
    for k in ("n_main", "n_left", "n_right"):
        geo[k] = np.full(shape, 0.03)
    geo["is_compound"] = np.broadcast_to((np.arange(N) % 2 == 0).astype(float), shape).copy()
    geo["h_bf"] = rng.uniform(1.0, 3.0, shape)
    geo["b_fp_l"], geo["b_fp_r"], geo["m_fp"] = rng.uniform(10.0, 80.0, shape), rng.uniform(10.0, 80.0, shape), rng.uniform(1.0, 4.0, shape)
    return geo


def table_batch(B, N, dtype, rng, per_reach, nodes=None, dx=None):
    b = PreissmannBatch(B, N, 2, dtype=dtype, section_mode="table", history=True)
    b.set_scheme(0.6, 600.0, 250.0, 1e-6, 100)
    b.set_geometry_table(compound_geo(rng, (B,) if per_reach else (), N))
    if nodes is not None:
        b.set_reach_nodes(nodes)
    if dx is not None:
        b.set_reach_scheme(dx=dx)
    return b


def thresholds(level, rng, per_reach):
    """a stage threshold from the downloaded stages [B, N] (or their first reach): a third ON the sample, a third NaN ("not
    assessed"), the rest a little above or below"""
    base = level if per_reach else level[0]
    u = rng.uniform(0, 1, base.shape)
    thr = np.where(np.isnan(base), 1.0, base) + rng.uniform(-0.5, 0.5, base.shape)
    thr = np.where(u < 1 / 3, np.where(np.isnan(base), 1.0, base), thr)
    return np.where(u > 2 / 3, NAN, thr)


def check_against_derive(b, nodes, dx, dtype, rng, first=0, n=1, what="", per_reach_threshold=True):
    """rows [first, first + n) of the integral block against numpy on derive's fields; returns the rows"""
    B = b.B
    d = b.derive(first, n, fields=("level", "area", "top_width"))
    thr = thresholds(d["level"][0], rng, per_reach_threshold)
    rows = b.reach_integrals(first, n, threshold=thr)
    t = thr.astype(np.float32).astype(np.float64) if dtype == "f32" else thr                 # rounded once to the batch's type
    t = np.broadcast_to(t, (B, b.N))
    assert set(rows) == set(A.INT_ROWS) and all(v.shape == (n, B) for v in rows.values())
    assert np.all(np.isnan(rows["balance"]))
    worst = 0.0
    for k in range(n):
        for r in range(B):
            nr, w = nodes[r], weights(nodes[r])
            for name, field in (("volume", "area"), ("surface", "top_width")):
                term, got = d[field][k, r, :nr], rows[name][k, r]
                if np.any(np.isnan(term)):
                    assert np.isnan(got), (what, name, k, r)
                    continue
                want = dx[r] * math.fsum(w * term)
                bar = (nr + 2) * EPS53 * dx[r] * math.fsum(w * np.abs(term))
                assert abs(got - want) <= bar, (what, name, k, r, got, want, bar)
                worst = max(worst, abs(got - want) / bar) if bar > 0 else worst
            with np.errstate(invalid="ignore"):
                over = d["level"][k, r, :nr] >= t[r, :nr]
            assert rows["length_over"][k, r] == dx[r] * math.fsum(w * over), (what, "length_over", k, r)
    print(f"INTEGRALS {what}: worst share of the bar {worst:.3f}")
    return rows


# ---- integrals against derive ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("N", SIZES)
def test_rectangular_rows_of_every_size(N, dtype):
    rng = np.random.default_rng(1000 + N)
    B = 5
    with uniform_batch("rect_uniform", B, N, dtype, rng) as b:
        h = depths(rng, B, N)
        b.set_state(h, np.ones((B, N)))
        rows = check_against_derive(b, [N] * B, [250.0] * B, dtype, rng, what=f"rect N={N} {dtype}")
        if N >= 3:
            assert np.isnan(rows["volume"][0, B - 1]) and not np.any(np.isnan(rows["volume"][0, :B - 1]))
        no_thr = b.reach_integrals(0, 1)
        assert np.all(np.isnan(no_thr["length_over"])) and same_rows(no_thr, rows, ("volume", "surface"))
        shared = check_against_derive(b, [N] * B, [250.0] * B, dtype, rng, what=f"rect N={N} {dtype}, shared threshold", per_reach_threshold=False)
        assert same_rows(shared, rows, ("volume", "surface"))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("mode", ["trap_uniform", "table", "tables_per_reach"])
def test_trapezoids_shared_and_per_reach_tables_ragged_with_their_own_spacing(mode, dtype):
    rng = np.random.default_rng(77)
    nodes = [129, 2, 64, 121, 3, 65, 127]
    B, N = len(nodes), 129
    dx = rng.uniform(100.0, 900.0, B)
    if mode == "trap_uniform":
        b = uniform_batch(mode, B, N, dtype, rng, nodes, dx)
    else:
        b = table_batch(B, N, dtype, rng, mode == "tables_per_reach", nodes, dx)
    with b:
        h = depths(rng, B, N, scale=6.0)
        h[np.arange(N)[None, :] >= np.array(nodes)[:, None]] = -777.0           # the padding of a ragged batch is not read
        b.set_state(h, np.ones((B, N)))
        rows = check_against_derive(b, nodes, dx, dtype, rng, what=f"{mode} {dtype}")
        assert np.sum(~np.isnan(rows["volume"])) >= B - 1
        b.reach_integrals(current=True)                                           # no threshold: the row is NaN, the others the same bits
        cur = b.integral_rows(0, 1)
        assert np.all(np.isnan(cur["length_over"])) and same_rows(cur, rows, ("volume", "surface"))


@pytest.mark.parametrize("kind", ["shared", "per_reach"])
def test_polyline_sections(kind):
    rng = np.random.default_rng(5)
    if kind == "shared":
        p = fixture_problem("irr_mixed")
        b, nodes = batch_from_problems([p] * 5, mode="irregular"), [p.N] * 5
        h0 = np.tile(p.h0, (5, 1))
    else:
        probs = [fixture_problem(t) for t in ("irr_single", "irr_mixed", "irr_single")]
        b, nodes = per_reach_polyline_batch(probs), [p.N for p in probs]
        h0 = np.stack([np.concatenate([p.h0, np.full(b.N - p.N, p.h0[-1])]) for p in probs])
    with b:
        h = h0 * rng.uniform(0.2, 1.6, h0.shape)
        h[0, 1], h[1, 2], h[b.B - 1, 3] = 0.0, -0.3, NAN
        b.set_state(h, np.ones(h.shape))
        dx = [fixture_problem("irr_mixed").dx] * b.B
        rows = check_against_derive(b, nodes, dx, "f64", rng, what=f"polylines {kind}")
        assert np.all(rows["volume"][0, :b.B - 1] > 0)        # (a polyline under a NaN stage is what derive makes of it: held above)


# ---- the same bits --------------------------------------------------------------------------------------------------------------------
def stepped_rect(lengths, dtype="f64", n_steps=5, history=True, bad=None, N=None, seed=900):
    """ragged RECT_UNIFORM batch of seeded prismatic reaches with an inflow hydrograph; bad: the reach whose target is NaN at K_STAR"""
    probs = [rect_problem(n, seed=seed + s, n_steps=n_steps) for s, n in enumerate(lengths)]
    if bad is not None:
        probs[bad] = edited(probs[bad], K_STAR, NAN)
    B, N, p0 = len(probs), N or max(lengths), probs[0]
    b = PreissmannBatch(B, N, p0.nt, dtype=dtype, section_mode="rect_uniform", history=history)
    b.set_scheme(p0.theta, p0.dt, p0.dx, 1e-3 if dtype == "f32" else p0.tol, p0.max_iter)
    b.set_geometry_uniform([p.geo["b_main"][0] for p in probs], [p.geo["n_main"][0] for p in probs], [p.geo["z_bed"][0] for p in probs],
                           [p.geo["z_bed"][-1] for p in probs])
    b.set_reach_nodes(list(lengths))
    b.set_boundary(A.UPSTREAM, BoundarySpec(A.BC_FLOW_HYDROGRAPH, {}, np.stack([p.us.target for p in probs], axis=1)))
    b.set_boundary(A.DOWNSTREAM, BoundarySpec(A.BC_NORMAL_DEPTH, dict(bed_slope=np.array([p.ds.bed_slope for p in probs]), bed_level=np.zeros(B))))
    pad = lambda a: np.concatenate([a, np.full(N - len(a), -777.0)])
    b.set_state(np.stack([pad(p.h0) for p in probs]), np.stack([pad(p.Q0) for p in probs]))
    return b, probs


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_current_state_halves_and_a_second_run_give_the_same_bits(dtype):
    lengths, steps = (121, 63, 33, 20, 65), 5
    b, _ = stepped_rect(lengths, dtype, steps)
    thr = 3.0
    with b:
        marks = [None] * (steps + 1)
        b.reach_integrals(threshold=thr, current=True)
        marks[0] = b.integral_rows(0, 1)
        for k in range(1, steps + 1):
            b.step(1)
            b.reach_integrals(threshold=thr, current=True)                         # the current state into row k
            marks[k] = b.integral_rows(k, 1)
        assert np.all(b.status() == 0)
        halves = [b.reach_integrals(0, 3, threshold=thr), b.reach_integrals(3, 3, threshold=thr)]
        whole = b.reach_integrals(0, steps + 1, threshold=thr)
        again = b.reach_integrals(0, steps + 1, threshold=thr)
        assert not np.any(np.isnan(whole["volume"])) and np.all(whole["volume"] > 0) and np.any(whole["length_over"] > 0)
        assert same_rows(again, whole)
        for name in ("volume", "surface", "length_over"):
            assert np.array_equal(bits(np.concatenate([halves[0][name], halves[1][name]])), bits(whole[name])), name
            assert np.array_equal(bits(np.concatenate([m[name] for m in marks])), bits(whole[name])), name
        one = b.reach_integrals(4, 1, threshold=thr)
        assert all(np.array_equal(bits(one[k][0]), bits(whole[k][4])) for k in ("volume", "surface", "length_over"))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("N", [121, 64])
def test_a_reach_alone_is_the_same_reach_at_place_77_of_130(N, dtype):
    rng = np.random.default_rng(31 + N)
    width, z_us, z_ds = rng.uniform(20.0, 200.0, 130), rng.uniform(3.0, 9.0, 130), rng.uniform(0.0, 1.0, 130)
    h = depths(rng, 130, N)
    h[77] = np.abs(np.nan_to_num(h[77], nan=1.0)) + 0.01
    thr = np.linspace(4.0, 12.0, N)
    out = []
    for members in (np.arange(130), np.array([77])):
        B = len(members)
        with PreissmannBatch(B, N, 2, dtype=dtype, section_mode="rect_uniform", history=True) as b:
            b.set_scheme(0.6, 600.0, 250.0, 1e-6, 100)
            b.set_geometry_uniform(width[members], np.full(B, 0.03), z_us[members], z_ds[members])
            b.set_state(h[members], np.ones((B, N)))
            rows = b.reach_integrals(0, 1, threshold=thr)
            b.reach_integrals(threshold=thr, current=True)
            assert same_rows(b.integral_rows(0, 1), rows)
            out.append({k: v[0, 77 if B == 130 else 0] for k, v in rows.items()})
    assert out[0]["volume"] > 0 and out[0]["length_over"] >= 0
    assert all(bits(out[0][k]) == bits(out[1][k]) for k in ("volume", "surface", "length_over")), out


# ---- closure of stepped batches -------------------------------------------------------------------------------------------------------
def c5_batch():
    from flowsim_amd.synthetic import c5_reach_parameters, inflow_table, normal_depth_trap
    fx, meta = O.load_fixture(os.path.join(GOLDEN, "c5_512.npz"))
    B, N, nt = meta["B"], meta["N"], meta["nt"]
    b_, m_, n_, S0, Qb = c5_reach_parameters(0, B)
    hn = normal_depth_trap(b_, m_, n_, S0, Qb)
    b = PreissmannBatch(B, N, nt, section_mode="trap_uniform", history=True)
    b.set_scheme(meta["theta"], meta["dt"], meta["dx"], 1e-6, 100)
    b.set_geometry_uniform(b_, n_, S0 * (N - 1) * meta["dx"], np.zeros(B), side_slope=m_)
    b.set_boundary(A.UPSTREAM, BoundarySpec(A.BC_FLOW_HYDROGRAPH, {}, inflow_table(Qb, nt, meta["dt"])))
    b.set_boundary(A.DOWNSTREAM, BoundarySpec(A.BC_RATING_POWER, dict(a=Qb / hn ** 1.6, b=np.full(B, 1.6), stage_shift=np.zeros(B), bed_level=np.zeros(B))))
    b.set_state_uniform(hn, Qb)
    return b, nt, meta["theta"], meta["dt"], meta["dx"], 1e-6


def closure_batch(name):
    """(batch with history, levels to hold, theta, dt, dx, tolerance)"""
    if name == "c5_512":
        return c5_batch()
    p = fixture_problem(name)
    levels = min(p.nt, 12) if name in ("gerd", "irr_levee") else p.nt
    return batch_from_problems([p]), levels, p.theta, p.dt, p.dx, p.tol


def level_bounds(V, N, dt, dx, tol):
    """per level k >= 1: dt dx sqrt(N - 1) tolerance + 4 (N + 2) 2^-53 max(V_k, V_k-1)"""
    return dt * dx * math.sqrt(N - 1) * tol + 4 * (N + 2) * EPS53 * np.maximum(V[1:], V[:-1])


@pytest.mark.parametrize("name", ["akbari", "c5_512", "bc_compound_normal", "gerd", "irr_levee"])
def test_stepped_fp64_batches_close_within_the_newton_tolerance(name):
    b, n, theta, dt, dx, tol = closure_batch(name)
    with b:
        b.step(n - 1)
        assert np.all(b.status() == 0), b.status()
        B, N = b.B, b.N
        b.reach_integrals(0, n)
        rows, tot = b.water_balance(0, n)
        hyd = b.hydrographs(0, n)
        V, res = rows["volume"], rows["balance"]
        assert np.all(res[0] == 0.0) and not np.any(np.isnan(res)) and np.all(V > 0)
        net = hyd[:, 1] - hyd[:, 3]
        inflow = dt * (theta * hyd[1:, 1] + (1.0 - theta) * hyd[:-1, 1])
        want = (V[1:] - V[:-1]) - dt * (theta * net[1:] + (1.0 - theta) * net[:-1])
        flows = dt * (np.abs(net[1:]) + np.abs(net[:-1]))
        assert np.all(np.abs(res[1:] - want) <= 8 * EPS53 * (np.maximum(V[1:], V[:-1]) + flows)), name      # the walk is this line, level by level
        for r in range(B):
            bound = level_bounds(V[:, r], N, dt, dx, tol)
            ratio = np.max(np.abs(res[1:, r]) / (dt * dx * math.sqrt(N - 1) * tol))
            print(f"CLOSURE {name} reach {r}: N = {N}, {n} levels, max |residual| = {np.max(np.abs(res[1:, r])):.3g} m3, ratio = {ratio:.3g}")
            assert np.all(np.abs(res[1:, r]) <= bound), (name, r, np.abs(res[1:, r]) / bound)
            assert (tot["spans"][r], tot["first_level"][r], tot["last_level"][r]) == (n - 1, 0, n - 1)
            assert tot["storage_change"][r] == V[-1, r] - V[0, r]
            assert tot["worst"][r] == np.max(np.abs(res[1:, r])) and tot["worst_level"][r] == 1 + np.argmax(np.abs(res[1:, r]))
            assert abs(tot["inflow"][r] - math.fsum(inflow[:, r])) <= (n + 2) * 2 * EPS53 * math.fsum(np.abs(inflow[:, r]))
            assert abs(tot["residual"][r] - math.fsum(res[1:, r])) <= (n + 2) * 2 * EPS53 * math.fsum(np.abs(res[1:, r]))
            assert abs(tot["relative"][r] - tot["residual"][r] / tot["inflow"][r]) <= 4 * EPS53 * abs(tot["relative"][r])
        part, _ = b.water_balance(2, n - 2)                                       # a range's first evaluated row gets 0, the later ones do not move
        assert np.all(part["balance"][0] == 0.0) and np.array_equal(bits(part["balance"][1:]), bits(res[3:]))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_marks_every_three_levels_on_a_batch_without_history(dtype):
    """the spans of a batch that keeps no history: each residual is held to the sum of the per-level bounds of its span (fp64; fp32:
    printed), the marked volumes to numpy on state() downloaded at each mark, so that nothing here leans on chunked stepping being
    bit-identical: the rectangular area b h is one product in the batch's type on both sides, the bar (N + 2) 2^-53 V is the sum's"""
    lengths, steps, every = (30, 63), 10, 3
    b, probs = stepped_rect(lengths, dtype, steps, history=False)
    R = np.float32 if dtype == "f32" else np.float64
    with b:
        with pytest.raises(A.FlowsimError, match="without FS_FLAG_HISTORY"):
            b.reach_integrals(0, 1)
        marked, states = [0], [b.state()[0].copy()]
        b.reach_integrals(current=True)
        while b.level < steps:
            b.step(min(every, steps - b.level))
            b.reach_integrals(current=True)
            marked.append(b.level)
            states.append(b.state()[0].copy())
        assert marked == [0, 3, 6, 9, 10] and np.all(b.status() == 0)
        rows, tot = b.water_balance(0, steps + 1)
        V, res = rows["volume"], rows["balance"]
        assert np.flatnonzero(~np.isnan(V[:, 0])).tolist() == marked and np.flatnonzero(~np.isnan(res[:, 1])).tolist() == marked
        for r, (p, n_r) in enumerate(zip(probs, lengths)):
            for k, h in zip(marked, states):
                area = (R(p.geo["b_main"][0]) * np.maximum(h[r, :n_r].astype(R), R(0))).astype(np.float64)      # b h in the batch's type
                want = p.dx * math.fsum(weights(n_r) * area)
                assert abs(V[k, r] - want) <= (n_r + 2) * EPS53 * want, (r, k, V[k, r], want)
            per_level = p.dt * p.dx * math.sqrt(n_r - 1) * (1e-3 if dtype == "f32" else p.tol) + 4 * (n_r + 2) * EPS53 * np.nanmax(V[:, r])
            assert res[0, r] == 0.0 and tot["spans"][r] == len(marked) - 1 and tot["last_level"][r] == steps
            for a, c in zip(marked[:-1], marked[1:]):
                print(f"SPAN {dtype} reach {r} levels {a} -> {c}: residual {res[c, r]:.3g} m3, bound {(c - a) * per_level:.3g}")
                if dtype == "f64":
                    assert abs(res[c, r]) <= (c - a) * per_level, (r, a, c, res[c, r])
        bands = b.integral_bands((0.5,), 0, steps + 1)
        assert np.flatnonzero(~np.isnan(bands["max"][:, 0])).tolist() == marked           # a level nobody evaluated is NaN, as numpy's


def test_the_closure_of_fp32_batches_is_computed_and_printed():
    b, probs = stepped_rect((63, 64, 65), "f32", 5)
    with b:
        b.step(5)
        b.reach_integrals(0, 6)
        rows, tot = b.water_balance(0, 6)
        assert not np.any(np.isnan(rows["balance"])) and np.all(tot["spans"] == 5)
        for r, p in enumerate(probs):
            print(f"CLOSURE fp32 reach {r}: worst {tot['worst'][r]:.3g} m3 at level {int(tot['worst_level'][r])}, "
                  f"dt dx sqrt(N - 1) tolerance = {p.dt * p.dx * math.sqrt(p.N - 1) * 1e-3:.3g}")


# ---- a failed reach between two good ones ---------------------------------------------------------------------------------------------
def test_a_reach_that_fails_at_level_2_stops_there_and_leaves_its_neighbours_alone():
    lengths, steps = (33, 33, 33), 5
    out = {}
    for bad in (None, 1):
        b, _ = stepped_rect(lengths, "f64", steps, bad=bad)
        with b:
            b.step(steps)
            st = b.status()
            b.reach_integrals(0, steps + 1, threshold=3.0)
            rows, tot = b.water_balance(0, steps + 1)
            b.reach_integrals(current=True)
            out[bad] = (st, rows, tot, b.integral_rows(steps, 1))
    st, rows, tot, cur = out[1]
    good = out[None]
    assert st.tolist() == [A.OK, A.NAN, A.OK] and np.all(good[0] == A.OK)
    for name in A.INT_ROWS:
        assert not np.any(np.isnan(rows[name][:K_STAR, 1])) and np.all(np.isnan(rows[name][K_STAR:, 1])), name
        assert np.array_equal(bits(rows[name][:, [0, 2]]), bits(good[1][name][:, [0, 2]])), name
        assert np.array_equal(bits(rows[name][:K_STAR, 1]), bits(good[1][name][:K_STAR, 1])), name       # its rows before the failure are what they were
    assert (tot["spans"][1], tot["first_level"][1], tot["last_level"][1]) == (K_STAR - 1, 0, K_STAR - 1)
    assert tot["storage_change"][1] == rows["volume"][K_STAR - 1, 1] - rows["volume"][0, 1]
    for name in A.BAL_ROWS:
        assert np.array_equal(bits(tot[name][[0, 2]]), bits(good[2][name][[0, 2]])), name
    assert np.all(np.isnan(cur["volume"][0, 1])) and np.array_equal(bits(cur["volume"][0, [0, 2]]), bits(rows["volume"][steps, [0, 2]]))


# ---- bands across the members ---------------------------------------------------------------------------------------------------------
def test_integral_bands_of_130_members_with_one_failed_against_numpy():
    """order statistics and quantiles bit for bit (band_cases.expected: np.sort and the documented lerp), and within 4 eps of
    np.quantile; mean and std within the bars of tests/test_gpu_band_select.py"""
    B, steps, bad = 130, 4, 40
    b, _ = stepped_rect([20] * B, "f64", steps, bad=bad)
    q = np.array([0.0, 0.05, 0.5, 0.95, 1.0, 64 / 128])
    with b:
        b.step(steps)
        st = b.status()
        assert st[bad] == A.NAN and np.sum(st != A.OK) == 1
        b.reach_integrals(0, steps + 1, threshold=np.linspace(2.0, 6.0, 20))
        rows, _ = b.water_balance(0, steps + 1)
        got = b.integral_bands(q, 0, steps + 1)
        none = b.integral_bands((), 1, 2)
        assert none["quantiles"].shape == (2, 4, 0) and np.array_equal(none["mean"], got["mean"][1:3])
    kept = st == A.OK
    assert got["n_members"].tolist() == [B - 1] * (steps + 1)
    terms = -(-B // BC.THREADS)
    for k in range(steps + 1):
        for i, name in enumerate(A.INT_ROWS):
            v = rows[name][k][kept] + 0.0
            e = BC.expected(v, q)
            assert not e["none"], (k, name)
            assert got["min"][k, i] == np.min(v) and got["max"][k, i] == np.max(v), (k, name)
            assert np.array_equal(bits(got["quantiles"][k, i]), bits(e["quantiles"])), (k, name)
            assert np.array_equal(got["quantiles"][k, i][e["integer"]], e["lo"][e["integer"]]), (k, name)
            assert np.all(np.abs(got["quantiles"][k, i] - np.quantile(v, q)) <= 4 * BC.EPS * np.maximum(np.abs(e["lo"]), np.abs(e["hi"]))), (k, name)
            assert abs(got["mean"][k, i] - e["mean"]) <= (terms + 9) * BC.EPS * e["abs_sum"] / e["m"], (k, name)
            assert abs(got["std"][k, i] - e["std"]) <= (terms + 13) * BC.EPS * e["abs_max"], (k, name)


# ---- a new state resets the rows ------------------------------------------------------------------------------------------------------
def test_set_state_init_state_and_restart_reset_the_rows():
    steps = 4
    b, probs = stepped_rect((33, 20), "f64", steps)
    with b:
        assert b.reach_integrals_device_ptr() is None                             # allocated by the first evaluation
        assert np.all(np.isnan(b.integral_rows(0, steps + 1)["volume"]))           # never evaluated: NaN
        assert b.reach_integrals_device_ptr()
        b.step(steps)
        first = b.reach_integrals(0, steps + 1)
        b.water_balance(0, steps + 1)
        h, Q = b.state()
        gh, gQ = b.guess()
        b.restart(2, h, Q, gh, gQ)                                                # the rows from that level on are NaN until evaluated again
        assert b.level == 2 and all(np.all(np.isnan(v)) for v in b.integral_rows(0, steps + 1).values())
        b.reach_integrals(current=True)
        after = b.integral_rows(0, steps + 1)
        assert np.flatnonzero(~np.isnan(after["volume"][:, 0])).tolist() == [2]
        assert np.array_equal(bits(after["volume"][2]), bits(first["volume"][steps]))     # the state it was restarted with
        b.init_state("linear", [p.Q0[0] for p in probs], depth_ds=[p.h0[-1] for p in probs], depth_us=[p.h0[0] for p in probs])
        assert b.level == 0 and all(np.all(np.isnan(v)) for v in b.integral_rows(0, steps + 1).values())
        b.reach_integrals(0, 1)
        assert not np.any(np.isnan(b.integral_rows(0, 1)["volume"]))
        pad = lambda a, n: np.concatenate([a, np.full(b.N - n, -777.0)])
        b.set_state(np.stack([pad(p.h0, p.N) for p in probs]), np.stack([pad(p.Q0, p.N) for p in probs]))
        assert all(np.all(np.isnan(v)) for v in b.integral_rows(0, steps + 1).values())
        b.step(steps)
        again = b.reach_integrals(0, steps + 1)
        assert same_rows(again, first)                                            # the same run, the same bits


def test_arguments_are_refused_with_a_text():
    b, _ = stepped_rect((20, 20), "f64", 3)
    with b:
        b.step(2)
        for call, text in ((lambda: b.reach_integrals(0, 4), "are not inside 0 .. 2"),
                           (lambda: b.water_balance(1, 3), "are not inside 0 .. 2"),
                           (lambda: b.integral_bands((0.5,), 0, 4), "are not inside 0 .. 2"),
                           (lambda: b.integral_bands((1.5,)), "quantile levels must be in"),
                           (lambda: b.integral_rows(0, 5), "level range out of bounds"),
                           (lambda: b._lib.fs_batch_reach_integrals(b._h, -1, 2, None, 0) and A.check(-1, "x"), "n must be 1"),
                           (lambda: b.reach_integrals(threshold=np.zeros(3)), "threshold must be a scalar")):
            with pytest.raises((A.FlowsimError, ValueError), match=text):
                call()


# ---- the runners' balance= keyword ----------------------------------------------------------------------------------------------------
def test_the_manning_runner_returns_the_balance_of_a_direct_batch_and_changes_nothing_else():
    from cases.gerd_roseires import settings as S
    from cases.gerd_roseires.model import build as build_model
    from flowsim_amd.ensemble import run_manning_ensemble
    solver, _ = build_model(inflow_hyd_func=None, sim_duration=12 * 3600)
    n_vals = np.array([0.025, 0.030, 0.035])
    nt, N = solver.number_of_time_levels, solver.number_of_nodes
    plain = run_manning_ensemble(solver, n_vals, tolerance=S.tolerance)
    assert np.all(plain["status"] == 0)
    marked = run_manning_ensemble(solver, n_vals, tolerance=S.tolerance, balance=dict(every=4, quantiles=(0.5,)))
    assert list(marked) == list(plain) + ["balance"] and sorted(marked["balance"]) == ["bands", "rows", "totals"]
    for k in plain:                                                               # stepping in chunks changes none of the old bits
        assert np.array_equal(marked[k], plain[k]), k
    rows, tot = marked["balance"]["rows"], marked["balance"]["totals"]
    levels = sorted(set(range(0, nt, 4)) | {nt - 1})
    assert np.flatnonzero(~np.isnan(rows["volume"][:, 0])).tolist() == levels and np.all(tot["spans"] == len(levels) - 1)
    whole = run_manning_ensemble(solver, n_vals, tolerance=S.tolerance, envelope=dict(quantities=("depth",)), balance=dict(threshold=480.0))
    w = whole["balance"]["rows"]
    assert not np.any(np.isnan(w["volume"])) and not np.any(np.isnan(w["length_over"]))
    assert np.array_equal(bits(w["volume"][levels]), bits(rows["volume"][levels]))          # history rows and marked states: the same bits
    per_level = S.time_step * solver.spatial_step * math.sqrt(N - 1) * S.tolerance
    assert np.all(np.abs(w["balance"][1:]) <= per_level + 4 * (N + 2) * EPS53 * np.max(w["volume"]))
    assert np.array_equal(whole["balance"]["bands"]["max"][:, 0], np.max(w["volume"], axis=1))
    with pytest.raises(ValueError, match="unknown keys"):
        run_manning_ensemble(solver, n_vals, tolerance=S.tolerance, balance=dict(evry=4))
