"""Geometry ensembles built on the device (fs_batch_set_geometry_irregular_members: flow-sim_amd/csrc/fs_member_geo.hpp) against the
path they replace: flowsim_amd._pack.member_sections (numpy, the definition of the member transform) handed to the per-reach
setter, whose stage tables the host builds (fs::build_stage_table).

1. tables and bed levels bit for bit, 2. the same steps to the bits (with tables and walking the edges), 3. three members of two
channels against the CPU oracle at the suite's bar, 4. run_geometry_ensemble against single-member runs of the mirror package,
5. the refusals.  Shapes: the smallest that cross each boundary of the two kernels - one member and two nodes; a node count that
is no multiple of the 64 node-lanes of a wave; node 65, which starts a second wave of node-lanes; 65 and 130 members; stations250 (245 stations,
256 breakpoint slots, a different vertex count per node); 15 and 16 stations (16 and 32 breakpoint slots)."""
import numpy as np
import pytest

from flowsim_amd import _abi as A
from flowsim_amd import _pack
from flowsim_amd.batch import PreissmannBatch
from flowsim_amd.ensemble import run_geometry_ensemble
from oracle import preissmann_oracle as O

from kernel_harness import TOL, assert_same_bits, rel_err, snapshot
import member_cases as MC
import poly_edges as PE

pytestmark = pytest.mark.gpu

# (B, N, kind, seed of the channel, stations per row (None: the channel's own))
SHAPES = [(1, 2, "overtopped_shallow", 5, None), (3, 24, "on_vertex", 1, None), (65, 20, "multi_run", 4, None),
          (130, 65, "overtopped_shallow", 5, None), (2, 6, "stations250", 8, None), (4, 20, "multi_run", 4, 16)]
IDS = [f"B{B}-N{N}-{kind}{'' if P is None else '-P%d' % P}" for B, N, kind, _, P in SHAPES]
SAMPLE = 200
_cases = {}


def case(shape):
    """(Problem, transforms, member_sections' output) of a shape; computed once, never changed"""
    if shape not in _cases:
        B, N, kind, seed, P = shape
        p = PE.BUILDERS[kind](N, np.random.default_rng(seed))
        if P is not None:            # rows padded to P stations by repeating the last one: the counts stay
            pad = P - p.geo["irr_x"].shape[1]
            assert pad > 0
            p.geo = dict(p.geo, **{k: np.concatenate([p.geo[k], np.repeat(p.geo[k][:, -1:], pad, axis=1)], axis=1) for k in ("irr_x", "irr_z")})
        tr = MC.transforms(B, N, 1000 + B + N)
        _cases[shape] = (p, tr, _pack.member_sections(p.geo, B, *tr))
    return _cases[shape]


def test_the_shapes_cross_the_boundaries_they_claim():
    kp = lambda s: (case(s)[0].geo["irr_x"].shape[1] + 16) & ~15
    assert [kp(s) for s in SHAPES] == [16, 16, 16, 16, 256, 32] and case(SHAPES[2])[0].geo["irr_x"].shape[1] == 15
    assert len(set(case(SHAPES[4])[0].geo["irr_npts"])) > 1 and case(SHAPES[4])[0].geo["irr_x"].shape[1] == 245


def batch(p, B, history=True):
    b = PreissmannBatch(B, p.N, p.nt, section_mode="irregular", history=history)
    b.set_scheme(p.theta, p.dt, p.dx, p.tol, p.max_iter)
    return b


def pair(shape):
    """(the member batch, the batch given member_sections' output through the per-reach setter)"""
    p, tr, sections = case(shape)
    dev, host = batch(p, shape[0]), batch(p, shape[0])
    dev.set_geometry_irregular_members(p.geo, *tr)
    host.set_geometry_irregular(sections)
    return p, dev, host


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


# ---- 1. tables -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_tables_and_bed_levels_are_the_host_builders_bit_for_bit(shape):
    B, N = shape[:2]
    p, dev, host = pair(shape)
    with dev, host:
        assert dev.poly_tables() == 1 and host.poly_tables() == 1
        sections = case(shape)[2]
        assert same_bits(dev.bed_levels(), host.bed_levels()) and same_bits(dev.bed_levels(), sections["z_bed"])
        every = [(r, i) for r in range(B) for i in range(N)]
        if len(every) > SAMPLE:
            pick = np.random.default_rng(B * N).choice(len(every), SAMPLE, replace=False)
            every = [every[q] for q in sorted(pick)] + [(B - 1, N - 1)]
        for r, i in every:
            got, want = dev.stage_table(r, i), host.stage_table(r, i)
            assert got.shape == want.shape and same_bits(got, want), (r, i, np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))[:8])


def test_stage_table_reads_a_shared_channel_too():
    """host-built tables of ONE channel: the reach is ignored; the member batch without a transform holds the same table per member"""
    p, _, _ = case(SHAPES[1])
    with batch(p, 3) as shared, batch(p, 3) as dev:
        shared.set_geometry_irregular(p.geo)
        dev.set_geometry_irregular_members(p.geo)
        for i in (0, 7, p.N - 1):
            assert same_bits(shared.stage_table(0, i), shared.stage_table(2, i)) and same_bits(shared.stage_table(0, i), dev.stage_table(1, i))
        assert same_bits(shared.bed_levels(), np.tile(p.geo["z_bed"], (3, 1))) and same_bits(dev.bed_levels(), shared.bed_levels())


# ---- 2. stepping -----------------------------------------------------------------------------------------------------------------
def step_both(shape, tables):
    B = shape[0]
    p, dev, host = pair(shape)
    with dev, host:
        assert dev.poly_tables() == host.poly_tables() == tables
        snaps = []
        for b in (dev, host):
            MC.with_member_beds(b, p)
            b.set_state(np.tile(p.h0, (B, 1)), np.tile(p.Q0, (B, 1)))
            b.step(p.nt - 1)
            snap = snapshot(b, p.nt, fields=("status", "iters", "hyd", "state", "guess"))
            # the history of the members that finished (a member that stopped early never wrote its later rows: they hold no promise)
            snap["hist"] = tuple(a[:, snap["status"] == 0] for a in b.history_arrays(0, p.nt))
            snaps.append(snap)
        assert dev.kernel_index() == host.kernel_index()
        assert_same_bits(snaps[0], snaps[1], what=shape)
        return snaps[0]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_member_batches_step_to_the_bits_of_host_built_batches(shape):
    snap = step_both(shape, 1)
    assert np.all(snap["iters"][1] > 0), "every member took Newton iterations"
    print(f"{shape}: {int(np.sum(snap['status'] == 0))} of {shape[0]} members finished all levels")


def test_member_batches_step_to_the_same_bits_walking_the_edges(monkeypatch):
    monkeypatch.setenv("FS_POLY_WALK", "1")
    step_both(SHAPES[1], 0)


# ---- 3. against the oracle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,N,seed", MC.ORACLE_CASES, ids=[c[0] for c in MC.ORACLE_CASES])
def test_members_against_the_oracle(kind, N, seed):
    p, dzl, dzm, dzr, ns, probs, refs = MC.oracle_members(kind, N, seed)
    assert all(MC.usable(q, ref) for q, ref in zip(probs, refs))
    with batch(p, 3) as b:
        b.set_geometry_irregular_members(p.geo, dzl, dzm, dzr, ns)
        MC.with_member_beds(b, p)
        b.set_state(np.tile(p.h0, (3, 1)), np.tile(p.Q0, (3, 1)))
        b.step(p.nt - 1)
        assert np.all(b.status() == 0), b.status()
        h, Q = b.history_arrays(0, p.nt)
        its = b.iterations(0, p.nt)
    for r, ref in enumerate(refs):
        eh, eq = rel_err(h[:, r], ref["depth"], 1e-3), rel_err(Q[:, r], ref["flow"], 1.0)
        print(f"{kind} member {r}: depth {eh:.2e} flow {eq:.2e} iterations {its[:, r].tolist()} oracle {ref['iters'].tolist()}")
        assert eh <= TOL and eq <= TOL, (r, eh, eq)
        assert np.array_equal(its[:, r], ref["iters"]), (r, its[:, r], ref["iters"])


# ---- 4. run_geometry_ensemble ----------------------------------------------------------------------------------------------------
SWEEP_CASE = MC.SWEEP_CASE


def test_run_geometry_ensemble_against_single_member_runs_of_the_mirror():
    import os
    from conftest import GOLDEN
    _, fx, m = next(c for c in O.sweep_cases(os.path.join(GOLDEN, "random_sweep.npz")) if c[0] == SWEEP_CASE)
    base = MC.mirror_solver(m["recipe"])
    geo = base.channel.node_geometry
    N = base.number_of_nodes
    assert np.all(geo["irr_npts"] > 0) and base.channel.downstream_boundary.bed_level == geo["z_bed"][-1]
    B = 4
    dzl, dzm, dzr, ns = MC.transforms(B, N, 57, amp=0.1)
    dzm[3], dzl[3], dzr[3] = 0.05, 0.0, -0.05                # a member whose shifts are the same at every node ...
    sections = _pack.member_sections(geo, B, dzl, dzm, dzr, ns)
    out = run_geometry_ensemble(base, dzl, dzm, dzr, ns, tolerance=m["tolerance"], max_iter=m["max_iter"])
    flat = run_geometry_ensemble(base, dz_main=np.array([0.0, 0.0, 0.0, 0.05]), dz_right=np.array([0.0, 0.0, 0.0, -0.05]),
                                 tolerance=m["tolerance"], max_iter=m["max_iter"])         # ... given as [B]
    assert np.all(out["status"] == 0) and out["hydrographs"].shape == (base.number_of_time_levels, 4, B)
    assert np.array_equal(flat["hydrographs"][:, :, 3], out["hydrographs"][:, :, 3]) and np.array_equal(flat["hydrographs"][:, :, 0], out["hydrographs"][:, :, 0])
    for r in range(B):
        one = MC.mirror_solver(m["recipe"], None if r == 0 else MC.member_geo(sections, r))      # member 0 has no transform: the untransformed run
        one.run(tolerance=m["tolerance"], verbose=0, max_iter=m["max_iter"])
        want = np.stack([one.depth[:, 0], one.flow[:, 0], one.depth[:, -1], one.flow[:, -1]], axis=1)
        got = out["hydrographs"][:, :, r]
        eh = max(rel_err(got[:, 0], want[:, 0], 1e-3 * m["h_n"]), rel_err(got[:, 2], want[:, 2], 1e-3 * m["h_n"]))
        eq = max(rel_err(got[:, 1], want[:, 1], 1e-3 * m["Qb"]), rel_err(got[:, 3], want[:, 3], 1e-3 * m["Qb"]))
        print(f"member {r}: depth {eh:.2e} flow {eq:.2e} iterations {out['iterations'][:, r].tolist()} single {np.asarray(one.iterations).tolist()}")
        assert eh <= TOL and eq <= TOL, (r, eh, eq)
        assert np.array_equal(out["iterations"][:, r], one.iterations), (r, out["iterations"][:, r], one.iterations)
    assert not np.array_equal(out["hydrographs"][:, :, 1], out["hydrographs"][:, :, 0])


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_batch_usable():
    shape = SHAPES[1]
    B, N = shape[:2]
    p, tr, sections = case(shape)
    dzl, dzm, dzr, ns = tr
    with batch(p, B) as b:
        b.set_geometry_irregular_members(p.geo, *tr)
        before = [b.stage_table(r, 5) for r in range(B)]
        trap = dict(p.geo, irr_npts=np.where(np.arange(N) == 3, 0, p.geo["irr_npts"]).astype(np.int32))
        with pytest.raises(A.FlowsimError, match="every node must be a polyline"):
            b.set_geometry_irregular_members(trap, *tr)
        for bad in (np.nan, np.inf):
            dz = dzm.copy()
            dz[1, 2] = bad
            with pytest.raises(A.FlowsimError, match="dz_left, dz_main and dz_right must be finite"):
                b.set_geometry_irregular_members(p.geo, dzl, dz, dzr, ns)
        for bad in (0.0, -0.5, np.nan):
            s = ns.copy()
            s[0, 2] = bad
            with pytest.raises(A.FlowsimError, match="n_scale must be finite and > 0"):
                b.set_geometry_irregular_members(p.geo, dzl, dzm, dzr, s)
        tilted = dict(p.geo, z_bed=p.geo["z_bed"] + 1.0)
        with pytest.raises(A.FlowsimError, match="Z_BED must hold min"):         # the shared channel goes through today's validation
            b.set_geometry_irregular_members(tilted, *tr)
        # the geometry of the last good call is still there, and the batch steps
        assert all(same_bits(b.stage_table(r, 5), before[r]) for r in range(B)) and same_bits(b.bed_levels(), sections["z_bed"])
        MC.with_member_beds(b, p)
        b.set_state(np.tile(p.h0, (B, 1)), np.tile(p.Q0, (B, 1)))
        b.step(1)
        assert b.level == 1 and b.status()[0] == 0
    with PreissmannBatch(2, N, p.nt, section_mode="table") as t:
        with pytest.raises(A.FlowsimError, match="another section_mode"):
            t.set_geometry_irregular_members(p.geo)
        t.set_scheme(p.theta, p.dt, p.dx, p.tol, p.max_iter)
        t.set_geometry_table({k: p.geo[k] for k in A.GEO_ROWS})
        assert same_bits(t.bed_levels(), np.tile(p.geo["z_bed"], (2, 1))), "bed_levels serves TABLE batches"
        with pytest.raises(A.FlowsimError, match="no polylines"):
            t.stage_table(0, 0)


def test_stage_table_refuses_a_walking_batch(monkeypatch):
    shape = SHAPES[1]
    p, tr, sections = case(shape)
    monkeypatch.setenv("FS_POLY_WALK", "1")
    with batch(p, shape[0]) as b:
        b.set_geometry_irregular_members(p.geo, *tr)
        assert b.poly_tables() == 0
        with pytest.raises(A.FlowsimError, match="walks its polylines' edges"):
            b.stage_table(0, 0)
        assert same_bits(b.bed_levels(), sections["z_bed"])
        monkeypatch.delenv("FS_POLY_WALK")
        b.set_geometry_irregular_members(p.geo, *tr)
        assert b.poly_tables() == 1 and b.stage_table(0, 0).size == 16 + 32 * 10
