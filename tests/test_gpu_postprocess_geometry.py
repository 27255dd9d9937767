"""Post-processing on the geometries a flood study runs on: fs_batch_derive (flow-sim_amd/csrc/fs_derive.hpp), fs_batch_envelope and
fs_batch_profile_bands (fs_envelope.hpp) on batches whose reaches each have their own tables, their own polylines, or are members
built on the device - the three setters that make geo_reach_stride / poly_reach_stride non-zero -, in fp32, and in every unroll form
of the envelope kernel.

The reference is tests/derived_reference.py (the oracle's section functions in float64; held to the reference's own prepare_results
arrays by tests/test_derived_reference.py), evaluated on the DEVICE'S OWN downloaded history: what is compared is the
post-processing kernel, not the solver, and a water surface that sits on a vertex bit for bit stays there.

Bars.
  fp64 against the helper on the same history: ARITH = 1e-12 (floor 1e-6).  Both sides take the same inputs, so the difference is
    rounding alone: a polyline of at most 16 stations is some 50 fp64 operations (2^-53 each: 6e-15 if they all lined up), the
    quotients and the square root of the Froude number and the celerity a dozen more; the only cancellation is a water's-edge
    point next to its vertex, whose edge then carries a vanishing share of a section that is decimetres deep everywhere here.
    1e-12 is a hundred times that and ten thousand times below the 1e-8 any wrong stride, station count or formula would show at.
    level, amplitude and peak_amplitude are one addition / subtraction of the same two numbers on both sides: bit for bit.
  fp64 against the fixtures' derived_* arrays (their own histories): kernel_harness.TOL, floor 1e-6 - the bar of
    test_irregular_derived_fields.
  fp32: per batch and field, 4 x the worst rel_err (floor 1e-6) of derived_reference.derived_f32 - the same formulas operation by
    operation in numpy float32 on geometry rounded to float32 - against the float64 helper on the same fp32 history.  That is the
    noise of an honest fp32 implementation, measured from the reference and not from the kernel; the factor is for fused
    multiply-adds and another operation order.  Measured bars (4 x included) on the MI355X histories:
                       level    area     top_width froude   velocity celerity amplitude peak_amplitude
      rect, ragged     7.07e-7  3.27e-7  1.47e-7   8.71e-7  4.76e-7  4.04e-7  0         0
      trap_uniform     5.55e-7  4.78e-7  2.23e-7   8.24e-7  5.44e-7  4.29e-7  0         0
      five tables      3.48e-7  6.25e-7  4.23e-7   1.19e-6  7.23e-7  5.14e-7  2.31e-7   1.25e-7
    (0: the subtraction of two fp32 depths within a factor two of each other is exact in either precision).  A uniform batch is
    given the bed at its two ends only, so the restatement interpolates it in float32 too (the 63-node reach alone: 1.6e-7 of the
    level).  The kernel's worst share of a bar is 43 %, the level of the ragged rectangular batch at 3.02e-7: it interpolates the
    bed with node * (1 / (n - 1)), as the step kernels do, where the restatement divides; elsewhere its error is the restatement's own, a quarter;
    every one below kernel_harness.TOL_F32 = 5e-4, which budgets a whole Newton run and is not used here.

Edge census on the device's histories (derived_reference.surface_census), asserted below:
      multi_run (20 nodes, 3 members, 8 levels): the surface on a vertex at 20 of 20 nodes of the untransformed member at level 0
        and in 53 of 480 samples; two or more wetted runs in 447 of 480;
      on_vertex (24 nodes, 3 members, 6 levels): on a vertex at 24 of 24 nodes at level 0 and in 115 of 432 samples.
On these histories the fp64 kernels are within 8.6e-16 of the helper in every field."""
import dataclasses
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
import derived_reference as DR
from envelope_checks import assert_envelope_is_numpy_on, check_profile, crossings_of, fields_of, ragged_batch
from fixture_batch import batch_from_problems, hetero_batch_from_problems, per_reach_polyline_batch
from flowsim_amd import _abi as A
from flowsim_amd import _pack
from flowsim_amd.batch import BoundarySpec, PreissmannBatch
from kernel_harness import TOL, TOL_F32, rel_err
import member_cases as MC
from oracle import preissmann_oracle as O
import poly_edges as PE
from synth import rect_problem, trap_problem

pytestmark = pytest.mark.gpu

ARITH = 1e-12
FIELDS = DR.FIELDS
EXACT = ("level", "amplitude", "peak_amplitude")
PLAIN = ("depth", "stage", "flow")
TABLES = ("bc_compound_normal", "bc_trap_poly", "example", "akbari", "bc_stage_fixed")
POLYLINES = ("irr_single", "irr_mixed", "irr_single")
MEMBERS = [f"members-{c[0]}" for c in MC.ORACLE_CASES]
CASES = ["tables5", "tables4", "polylines3", "polylines2"] + MEMBERS


@dataclasses.dataclass
class Case:
    b: PreissmannBatch
    geos: list                      # one geo dict per reach, the reach's own nodes only
    nodes: list                     # node count per reach
    n: int                          # levels held: 0 .. n - 1
    fixtures: list                  # per reach: the fixture's arrays, or None
    h: np.ndarray = None            # the downloaded history [n, B, N]
    Q: np.ndarray = None
    d: dict = None                  # b.derive(0, n), every field

    @property
    def own(self):
        return np.arange(self.b.N)[None, :] < np.array(self.nodes)[:, None]


def fixture_problem(name):
    fx, meta = O.load_fixture(os.path.join(GOLDEN, name + ".npz"))
    return fx, O.problem_from_fixture(fx, meta)


def recorded_members(kind, N, seed):
    """(Problem, dz_left, dz_main, dz_right [3, N], n_scale [3, 3]) of a case of MC.ORACLE_CASES from the record: the channel from
    its builder and the recorded seeds - no oracle run"""
    rec = json.load(open(MC.CHOICES))[f"{kind}-{N}-{seed}"]
    p = PE.BUILDERS[kind](N, np.random.default_rng(rec["channel_seed"]))
    p.tol = rec["tol"]
    draws = [MC.member_draw(p, r, s)[0] for r, s in enumerate(rec["member_seeds"])]
    dzl, dzm, dzr = (np.concatenate([d[q] for d in draws]) for q in range(3))
    return p, dzl, dzm, dzr, np.concatenate([d[3] for d in draws], axis=1)


def build(name):
    if name.startswith("tables"):
        loaded = [fixture_problem(t) for t in TABLES[:int(name[-1])]]
        probs = [p for _, p in loaded]
        b = hetero_batch_from_problems(probs)
        return Case(b, [p.geo for p in probs], [p.N for p in probs], min(p.nt for p in probs), [fx for fx, _ in loaded])
    if name.startswith("polylines"):
        loaded = [fixture_problem(t) for t in POLYLINES[:int(name[-1])]]
        probs = [p for _, p in loaded]
        assert len({(p.theta, p.dt, p.dx, p.tol, p.nt) for p in probs}) == 1
        b = per_reach_polyline_batch(probs)
        return Case(b, [p.geo for p in probs], [p.N for p in probs], probs[0].nt, [fx for fx, _ in loaded])
    kind, N, seed = next(c for c in MC.ORACLE_CASES if name == f"members-{c[0]}")
    p, dzl, dzm, dzr, ns = recorded_members(kind, N, seed)
    sections = _pack.member_sections(p.geo, 3, dzl, dzm, dzr, ns)
    b = PreissmannBatch(3, p.N, p.nt, section_mode="irregular", history=True)
    b.set_scheme(p.theta, p.dt, p.dx, p.tol, p.max_iter)
    b.set_geometry_irregular_members(p.geo, dzl, dzm, dzr, ns)
    MC.with_member_beds(b, p)
    b.set_state(np.tile(p.h0, (3, 1)), np.tile(p.Q0, (3, 1)))
    return Case(b, [MC.member_geo(sections, r) for r in range(3)], [p.N] * 3, p.nt, [None] * 3)


_cases = {}


def case(name):
    """the batch of a case, stepped, with its history and derived fields downloaded: built once per module"""
    if name not in _cases:
        c = build(name)
        c.b.step(c.n - 1)
        c.h, c.Q = c.b.history_arrays(0, c.n)
        c.d = c.b.derive(0, c.n)
        _cases[name] = c
    return _cases[name]


@pytest.fixture(scope="module", autouse=True)
def batches_closed_at_the_end():
    yield
    for c in _cases.values():
        c.b.close()
    _cases.clear()


def field_of(d, f, r, n):
    return d[f][r, :n] if f == "peak_amplitude" else d[f][:, r, :n]


# ---- derive on per-reach geometry ------------------------------------------------------------------------------------------------
def test_the_batches_are_the_shapes_they_claim():
    shapes = {name: (case(name).b.B, case(name).b.N) for name in CASES}
    assert shapes == dict(tables5=(5, 41), tables4=(4, 41), polylines3=(3, 17), polylines2=(2, 17), **{MEMBERS[0]: (3, 20), MEMBERS[1]: (3, 24)})
    assert (5 * 41) % 2 == 1 and (4 * 41) % 2 == 0 and (3 * 17) % 2 == 1 and (2 * 17) % 2 == 0          # both access paths of the kernels
    assert case("tables5").n == 21 and [g["irr_x"].shape[1] for g in case("polylines2").geos] == [15, 16]
    assert len({c.n for c in (case("polylines3"), case("polylines2"))}) == 1 and case("polylines3").n == 37


@pytest.mark.parametrize("name", CASES)
def test_derived_fields_of_per_reach_geometry(name):
    c = case(name)
    assert np.all(c.b.status() == 0), c.b.status()
    assert set(c.d) == set(FIELDS)
    beds = c.b.bed_levels()
    for r, (geo, n) in enumerate(zip(c.geos, c.nodes)):
        h, Q = c.h[:, r, :n], c.Q[:, r, :n]
        want = DR.derived(geo, h, Q)
        for f in FIELDS:
            got = field_of(c.d, f, r, n)
            err = rel_err(got, want[f], 1e-6)
            print(name, "reach", r, f, "against the helper", err)
            assert err <= ARITH, (name, r, f, err)
            if f in EXACT:
                assert np.array_equal(got, want[f]), (name, r, f)
            # slots beyond the reach's own nodes
            assert np.all((c.d[f][r, n:] if f == "peak_amplitude" else c.d[f][:, r, n:]) == 0.0), (name, r, f)
        # the bed the kernel adds is the one the batch reports: level is the same one addition, so level - h is that bed within the
        # rounding of the sum and of the two differences taken here (2^-53 of at most |level| + |h| each)
        level = c.d["level"][:, r, :n]
        assert np.array_equal(beds[r, :n], np.asarray(geo["z_bed"], dtype=np.float64))
        assert np.array_equal(level, h + beds[r, :n])
        assert np.all(np.abs(level - h - beds[r, :n]) <= 3 * 2.0 ** -53 * (np.abs(level) + np.abs(h)))
        fx = c.fixtures[r]
        if fx is not None:
            for f in FIELDS:
                ref = fx["derived_amplitude"][:c.n].max(axis=0) if f == "peak_amplitude" else fx["derived_" + f][:c.n]
                err = rel_err(field_of(c.d, f, r, n), ref, 1e-6)
                print(name, "reach", r, f, "against the fixture", err)
                assert err <= TOL, (name, r, f, err)


@pytest.mark.parametrize("name", MEMBERS)
def test_the_member_batches_reach_the_edges(name):
    """the inputs put the surface on vertices and split it into several wetted runs - counted on the device's own history"""
    c = case(name)
    on, runs = zip(*[DR.surface_census(geo, c.h[:, r]) for r, geo in enumerate(c.geos)])
    on, runs = np.stack(on, axis=1), np.stack(runs, axis=1)              # [n, 3, N]
    print(name, "surface on a vertex: level 0 of member 0", int(on[0, 0].sum()), "of", on.shape[2], "; all samples", int(on.sum()), "of", on.size,
          "; samples with two or more wetted runs", int((runs >= 2).sum()))
    assert np.all(on[0, 0]), "at level 0 every node of the untransformed member has its surface on a vertex"
    if "multi_run" in name:
        assert (runs >= 2).sum() > 0 and runs.max() >= 3


# ---- envelopes and bands ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_envelopes_and_bands_of_per_reach_geometry(name):
    c = case(name)
    b, own, n = c.b, c.own, c.n
    B = b.B
    x = fields_of(b, 0, n)
    for q, f in (("stage", "level"), ("velocity", "velocity"), ("froude_number", "froude_number"), ("top_width", "top_width")):
        assert np.array_equal(x[q], c.d[f])                            # the anchored fields
    thr = np.where(own, 0.5 * (x["stage"].min(axis=0) + x["stage"].max(axis=0)), 0.0)          # [B, N]: each node's own stage range
    env = b.envelope(A.ENV_QUANTITIES, threshold=thr, first=0, n=n)
    assert env["levels"].tolist() == [n] * B
    for q in A.ENV_QUANTITIES:
        assert_envelope_is_numpy_on(env, x[q], q, own, name)
        assert np.all(env[q]["max"][~own] == 0) and np.all(env[q]["min"][~own] == 0)
        assert np.all(env[q]["max_level"][~own] == -1) and np.all(env[q]["min_level"][~own] == -1)
    first, last, count = crossings_of(x["stage"], thr)
    cr = env["crossing"]
    assert np.array_equal(cr["first"][own], first[own]) and np.array_equal(cr["last"][own], last[own]) and np.array_equal(cr["count"][own], count[own])
    assert np.all(cr["count"][~own] == 0) and np.all(cr["first"][~own] == -1) and np.all(cr["last"][~own] == -1)
    assert 0 < count[own].min() and count[own].max() <= n
    if name in MEMBERS:
        for q in ("stage", "velocity"):
            got = check_profile(b, env[q]["max"], own, q, "max", cr["count"])
            assert np.all(got["n_members"] == B)
    plain = b.envelope(PLAIN, threshold=thr, first=0, n=n)
    assert all(np.array_equal(plain[q][s], env[q][s]) for q in PLAIN for s in A.ENV_STATS)
    assert all(np.array_equal(plain["crossing"][k], cr[k]) for k in A.ENV_CROSS_ROWS)


# ---- every unroll form of the envelope kernel ------------------------------------------------------------------------------------
UNROLL_LENGTHS, UNROLL_STEPS = (20, 63, 33), 9
RANGES = ((0, 1), (0, 3), (0, 4), (0, 5), (1, 7), (0, 8), (0, 9), (2, 8))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_every_unroll_form_of_the_envelope_kernel(dtype, monkeypatch):
    """FS_ENVELOPE_UNROLL = 1, 4, 8 x (the plain quantities, all six): the five instantiations per precision (8 with all six runs
    the 4 again).  The ranges put the clamped tail row (k0 + u >= most) at every offset of each unroll form."""
    own = np.arange(max(UNROLL_LENGTHS))[None, :] < np.array(UNROLL_LENGTHS)[:, None]
    monkeypatch.delenv("FS_ENVELOPE_UNROLL", raising=False)
    with ragged_batch(UNROLL_LENGTHS, dtype, n_steps=UNROLL_STEPS) as b:
        b.step(UNROLL_STEPS)
        assert np.all(b.status() == 0)
        for first, n in RANGES:
            x = fields_of(b, first, n)
            thr = np.where(own, 0.5 * (x["stage"].min(axis=0) + x["stage"].max(axis=0)), 0.0)
            t = thr.astype(np.float32).astype(np.float64) if dtype == "f32" else thr              # rounded once to the batch's type
            crossings = crossings_of(x["stage"], t)
            monkeypatch.delenv("FS_ENVELOPE_UNROLL", raising=False)
            default = {names: b.envelope(names, threshold=thr, first=first, n=n) for names in (A.ENV_QUANTITIES, PLAIN)}
            for u in (1, 4, 8):
                monkeypatch.setenv("FS_ENVELOPE_UNROLL", str(u))
                for names in (A.ENV_QUANTITIES, PLAIN):
                    what = (dtype, first, n, u, len(names))
                    got = b.envelope(names, threshold=thr, first=first, n=n)
                    assert got["levels"].tolist() == [n] * len(UNROLL_LENGTHS), what
                    for q in names:
                        assert all(np.array_equal(got[q][s], default[names][q][s]) for s in A.ENV_STATS), (what, q)
                        assert_envelope_is_numpy_on(got, x[q], q, own, what)
                    for k, want in zip(A.ENV_CROSS_ROWS, crossings):
                        assert np.array_equal(got["crossing"][k], default[names]["crossing"][k]), (what, k)
                        assert np.array_equal(got["crossing"][k][own], want[own]), (what, k)


# ---- fp32 ------------------------------------------------------------------------------------------------------------------------
TRAPS = ((120.0, 1.5, 0.030, 4e-4, 300.0), (80.0, 2.0, 0.025, 6e-4, 150.0), (200.0, 1.0, 0.035, 3e-4, 500.0))


def fp32_tolerance(p, flow):
    """the convergence tolerance of an fp32 run of a fixture: 1e-3 unless fp32 cannot resolve it - the tolerance is held
    against the 2-norm of the 2 N residual rows, whose terms are flows: a row rounds at 2^-24 |Q| a handful (8) of times"""
    return max(1e-3, 8.0 * np.sqrt(2 * p.N) * 2.0 ** -24 * float(np.abs(flow).max()))


def fp32_batch(kind):
    """(batch, per reach the float64 geo of its own nodes, per reach the geo the float32 restatement starts from, node counts, levels
    to step).  A uniform batch is given its width, side slope and end bed levels, so an fp32 implementation has to interpolate the
    bed in fp32: the restatement does (uniform_geo in float32); a table batch is given every node's numbers, which it rounds."""
    if kind == "rect_ragged":
        lengths = (20, 63, 33)
        probs = [rect_problem(n, seed=900 + s, n_steps=5) for s, n in enumerate(lengths)]          # the reaches of ragged_batch
        geos, geos32 = ([DR.uniform_geo(p.geo["b_main"][0], p.geo["z_bed"][0], p.geo["z_bed"][-1], p.N, dtype=t) for p in probs] for t in (np.float64, np.float32))
        return ragged_batch(lengths, "f32"), geos, geos32, list(lengths), 5
    if kind == "trap_uniform":
        probs = [trap_problem(*t, 24, 6, tol=1e-3) for t in TRAPS]
        geos, geos32 = ([DR.uniform_geo(p.geo["b_main"][0], p.geo["z_bed"][0], p.geo["z_bed"][-1], p.N, p.geo["m_main"][0], dtype=t) for p in probs]
                        for t in (np.float64, np.float32))
        return batch_from_problems(probs, mode="trap_uniform", dtype="f32"), geos, geos32, [24] * 3, 6
    loaded = [fixture_problem(t) for t in TABLES]
    steps = min(p.nt for _, p in loaded) - 1
    probs = [dataclasses.replace(p, tol=fp32_tolerance(p, fx["flow"][:steps + 1])) for fx, p in loaded]
    return hetero_batch_from_problems(probs, dtype="f32"), [p.geo for p in probs], [p.geo for p in probs], [p.N for p in probs], steps


@pytest.mark.parametrize("kind", ["rect_ragged", "trap_uniform", "tables5"])
def test_fp32_derived_fields_against_the_float64_helper(kind):
    b, geos, geos32, nodes, steps = fp32_batch(kind)
    with b:
        b.step(steps)
        assert np.all(b.status() == 0), b.status()
        h, Q = b.history_arrays(0, steps + 1)
        d = b.derive(0, steps + 1)
    own = np.arange(b.N)[None, :] < np.array(nodes)[:, None]              # (slots beyond a reach's nodes are never written)
    assert np.array_equal(h[:, own].astype(np.float32).astype(np.float64), h[:, own]), "an fp32 history"
    assert (b.B * b.N) % 4 == (0 if kind == "trap_uniform" else 1)          # 16-byte accesses in one batch, single elements in two
    refs, noise = [], {f: 0.0 for f in FIELDS}
    for geo, geo32, n, r in zip(geos, geos32, nodes, range(b.B)):
        h32, Q32 = h[:, r, :n].astype(np.float32), Q[:, r, :n].astype(np.float32)
        refs.append(DR.derived(geo, h32, Q32))
        honest = DR.derived_f32(geo32, h32, Q32)
        for f in FIELDS:
            noise[f] = max(noise[f], rel_err(honest[f].astype(np.float64), refs[-1][f], 1e-6))
    bars = {f: 4.0 * noise[f] for f in FIELDS}
    print(kind, "fp32 bars (4 x the float32 restatement's noise):", {f: float(f"{v:.3g}") for f, v in bars.items()})
    assert all(v < TOL_F32 for v in bars.values()), bars
    for r, n in enumerate(nodes):
        for f in FIELDS:
            err = rel_err(field_of(d, f, r, n), refs[r][f], 1e-6)
            print(kind, "reach", r, f, err, "bar", bars[f])
            assert err <= bars[f], (kind, r, f, err, bars[f])
            assert np.all((d[f][r, n:] if f == "peak_amplitude" else d[f][:, r, n:]) == 0.0), (kind, r, f)


# ---- the runners' envelope= keyword ----------------------------------------------------------------------------------------------
def assert_end_nodes_are_numpy_on_the_hydrographs(env, hyd, last):
    """depth and flow of the envelope at node 0 and at each member's last node against numpy over hydrographs [nt, 4, B], bit for bit"""
    members = np.arange(hyd.shape[2])
    for q, cols in (("depth", (0, 2)), ("flow", (1, 3))):
        for node, col in zip((np.zeros_like(last), last), cols):
            x = hyd[:, col, :]
            e = {s: env[q][s][members, node] for s in A.ENV_STATS}
            assert np.array_equal(e["max"], np.max(x, axis=0)) and np.array_equal(e["min"], np.min(x, axis=0)), (q, col)
            assert np.array_equal(e["max_level"], np.argmax(x, axis=0)) and np.array_equal(e["min_level"], np.argmin(x, axis=0)), (q, col)


def test_the_geometry_ensemble_runner_returns_the_envelopes_of_a_direct_batch():
    from flowsim_amd.ensemble import run_geometry_ensemble
    from flowsim_amd.hydromodel.preissmann import boundary_to_spec
    _, fx, m = next(c for c in O.sweep_cases(os.path.join(GOLDEN, "random_sweep.npz")) if c[0] == MC.SWEEP_CASE)
    base = MC.mirror_solver(m["recipe"])
    ch, N, nt = base.channel, base.number_of_nodes, base.number_of_time_levels
    B = 4
    dzl, dzm, dzr, ns = MC.transforms(B, N, 57, amp=0.1)
    dzm[3], dzl[3], dzr[3] = 0.05, 0.0, -0.05
    with PreissmannBatch(B, N, nt, section_mode="irregular", history=True) as b:          # what the runner does, step by step
        b.set_scheme(base.theta, base.time_step, base.spatial_step, m["tolerance"], m["max_iter"])
        b.set_geometry_irregular_members(ch.node_geometry, dzl, dzm, dzr, ns)
        beds = b.bed_levels()
        for side, boundary, bed in ((A.UPSTREAM, ch.upstream_boundary, beds[:, 0]), (A.DOWNSTREAM, ch.downstream_boundary, beds[:, -1])):
            spec = boundary_to_spec(boundary, nt, base.time_step)
            if "bed_level" in spec.params:
                spec = BoundarySpec(spec.kind, dict(spec.params, bed_level=bed.copy()), spec.target)
            b.set_boundary(side, spec)
        assert ch.interpolation_method == "linear"
        b.init_state("linear", ch.initial_flow_rate, depth_ds=ch.downstream_boundary.initial_depth, depth_us=ch.upstream_boundary.initial_depth)
        b.step(nt - 1)
        assert np.all(b.status() == 0)
        stage = fields_of(b, 0, nt)["stage"]
        thr = 0.5 * (stage.min(axis=0) + stage.max(axis=0))            # [B, N]
        env = b.envelope(("stage", "velocity"), threshold=thr)
        bands = {q: b.profile_bands(q, "max", (0.05, 0.5, 0.95)) for q in ("stage", "velocity")}
        hyd, its = b.hydrographs(), b.iterations()
    kw = dict(tolerance=m["tolerance"], max_iter=m["max_iter"])
    res = run_geometry_ensemble(base, dzl, dzm, dzr, ns, envelope=dict(quantities=("stage", "velocity"), threshold=thr), **kw)
    assert sorted(res) == ["envelope", "hydrographs", "iterations", "profile_bands", "status"]
    assert np.array_equal(res["hydrographs"], hyd) and np.array_equal(res["iterations"], its) and np.all(res["status"] == 0)
    assert sorted(res["envelope"]) == ["crossing", "levels", "stage", "velocity"] and sorted(res["profile_bands"]) == ["stage", "velocity"]
    for q in ("stage", "velocity"):
        assert all(np.array_equal(res["envelope"][q][s], env[q][s]) for s in A.ENV_STATS), q
        assert all(np.array_equal(res["profile_bands"][q][k], bands[q][k]) for k in bands[q]), q
    assert all(np.array_equal(res["envelope"]["crossing"][k], env["crossing"][k]) for k in A.ENV_CROSS_ROWS)
    assert res["envelope"]["levels"].tolist() == [nt] * B and np.any(env["crossing"]["count"] > 0)
    ends = run_geometry_ensemble(base, dzl, dzm, dzr, ns, envelope=dict(quantities=("depth", "flow")), **kw)
    assert np.array_equal(ends["hydrographs"], hyd) and ends["envelope"]["crossing"] is None
    assert_end_nodes_are_numpy_on_the_hydrographs(ends["envelope"], hyd, np.full(B, N - 1))
    plain = run_geometry_ensemble(base, dzl, dzm, dzr, ns, **kw)
    assert list(plain) == ["hydrographs", "iterations", "status"]
    assert np.array_equal(plain["hydrographs"], hyd) and np.array_equal(plain["iterations"], its) and np.all(plain["status"] == 0)
    with pytest.raises(ValueError, match="unknown keys"):
        run_geometry_ensemble(base, dzl, dzm, dzr, ns, envelope=dict(quantity="stage"), **kw)


def test_the_scenario_ensemble_runner_returns_envelopes_that_agree_with_its_hydrographs():
    """the six members of tests/test_gpu_forcing.py::test_scenario_sweep_is_its_members_run_one_at_a_time"""
    from cases.gerd_roseires import settings as S
    from cases.gerd_roseires.gerd_discharge import GerdHydrograph
    from cases.gerd_roseires.inputs import import_hydrograph
    from cases.gerd_roseires.model import build as build_model
    from flowsim_amd.ensemble import run_scenario_ensemble
    solver, _ = build_model(inflow_hyd_func=None)
    table, spec = import_hydrograph(S.inflow_hyd_path), GerdHydrograph.pool_spec()
    kw = dict(inflow_scale=np.array([0.5, 1.0, 1.5, 2.0, 2.5, 1.25]), inflow_shift=np.array([0.0, 5400.0, -5400.0, 0.0, 5400.0, 0.0]),
              pool_level=np.array([640.0, 637.0, 634.125, 641.0, 632.0, 642.0]), n_main=np.array([0.030, 0.025, 0.035, 0.030, 0.040, 0.028]),
              tolerance=S.tolerance)
    B, N, nt = 6, solver.number_of_nodes, solver.number_of_time_levels
    old = run_scenario_ensemble(solver, spec, table, **kw)
    assert list(old) == ["hydrographs", "iterations", "status", "initial_flow", "pool"] and np.all(old["status"] == 0)
    res = run_scenario_ensemble(solver, spec, table, envelope=dict(quantities=("depth", "flow")), **kw)
    assert list(res) == list(old) + ["envelope", "profile_bands"] and sorted(res["profile_bands"]) == ["depth", "flow"]
    for k in ("hydrographs", "iterations", "status", "initial_flow"):                  # the keyword changes none of the old bits
        assert np.array_equal(res[k], old[k]), k
    assert all(np.array_equal(res["pool"][k], old["pool"][k]) for k in old["pool"])
    env = res["envelope"]
    assert sorted(env) == ["crossing", "depth", "flow", "levels"] and env["crossing"] is None and env["levels"].tolist() == [nt] * B
    assert env["depth"]["max"].shape == (B, N)
    assert_end_nodes_are_numpy_on_the_hydrographs(env, res["hydrographs"], np.full(B, N - 1))
    for q in ("depth", "flow"):
        assert np.array_equal(res["profile_bands"][q]["max"], env[q]["max"].max(axis=0)) and np.all(res["profile_bands"][q]["n_members"] == B)
