"""Geometry-ensemble cases shared by tests/test_member_geometry.py (CPU), tests/test_gpu_member_geometry.py and
tests/test_gpu_postprocess_geometry.py: seeded member
transforms of the polyline channels of tests/poly_edges.py, the members as oracle Problems, and the members the oracle comparison
uses.  flowsim_amd._pack.member_sections is the definition of the transform and the reference throughout."""
import dataclasses
import json
import logging
import os

import numpy as np

from conftest import GOLDEN
from flowsim_amd import _abi as A
from flowsim_amd import _pack
from flowsim_amd.batch import BoundarySpec
from oracle import preissmann_oracle as O

from fixture_batch import boundary_spec
import poly_edges as PE

log = logging.getLogger("member_cases")
CHOICES = os.path.join(GOLDEN, "member_geometry", "oracle_members.json")


def transforms(B, N, seed, amp=0.3):
    """dz_left, dz_main, dz_right [B, N] and n_scale [3, B], seeded, |dz| <= amp: member r % 3 == 0 has no transform, r % 3 == 1 a
    main-channel shift only, r % 3 == 2 all three shifts and the roughness factors"""
    rng = np.random.default_rng(seed)
    dzl, dzm, dzr = (rng.uniform(-amp, amp, (B, N)) for _ in range(3))
    ns = rng.uniform(0.8, 1.25, (3, B))
    kind = np.arange(B) % 3
    dzm[kind == 0] = 0.0
    dzl[kind != 2] = 0.0
    dzr[kind != 2] = 0.0
    ns[:, kind != 2] = 1.0
    return dzl, dzm, dzr, ns


def member_geo(sections, r):
    """member r of _pack.member_sections' output as the geo dict of one channel"""
    return {k: np.ascontiguousarray(v[r]) for k, v in sections.items()}


def member_problem(p, sections, r):
    """the oracle Problem of member r: the transformed sections, the same depths and flows, each boundary on the member's own bed"""
    geo = dict(p.geo, **member_geo(sections, r))
    return dataclasses.replace(p, geo=geo, us=dataclasses.replace(p.us, bed_level=float(geo["z_bed"][0])),
                               ds=dataclasses.replace(p.ds, bed_level=float(geo["z_bed"][-1])))


# ---- the members that run against the oracle -------------------------------------------------------------------------------------
# Three members of a channel of poly_edges.make: member r takes row r of transforms(3, N, s_r, 0.1) - none, a main-channel shift, all
# three shifts and the roughness factors -, s_r being the first seed from 100 * seed + 10 * r on whose member converges in the oracle
# with no Newton norm within poly_edges.FRAGILE of the tolerance (the way poly_edges.make takes the first usable draw).  The search
# costs minutes of numpy oracle: search_oracle_members runs it, tests/golden/member_geometry/oracle_members.json records what it
# found (the channel's own seed and tolerance included), the CPU test holds the record to the search, and the GPU test builds its
# members from the record and runs the oracle on those alone.
ORACLE_CASES = [("multi_run", 20, 4), ("on_vertex", 24, 1)]
AMP, TRIES = 0.1, 10


def member_draw(p, r, s):
    """(dz_left, dz_main, dz_right [N], n_scale [3]) of member r under seed s, and its Problem"""
    dzl, dzm, dzr, ns = transforms(3, p.N, s, AMP)
    one = tuple(v[r:r + 1] for v in (dzl, dzm, dzr)) + (ns[:, r:r + 1],)
    return one, member_problem(p, _pack.member_sections(p.geo, 1, *one), 0)


def usable(q, run):
    return run["status"] == 0 and not PE.fragile(run, q.tol)


def search_oracle_members(kind, N, seed):
    """the record entry of a case: dict(channel_seed, tol, member_seeds [3]); rejections logged"""
    p, _ = PE.make(kind, N, seed)
    chan = next(s for s in range(seed, seed + 6) if np.array_equal(PE.BUILDERS[kind](N, np.random.default_rng(s)).geo["irr_z"], p.geo["irr_z"]))
    seeds = []
    for r in range(3):
        for s in range(100 * seed + 10 * r, 100 * seed + 10 * r + TRIES):
            _, q = member_draw(p, r, s)
            if usable(q, O.newton_run(q, trace=True, iterates=True)):
                seeds.append(s)
                break
            log.warning("member_cases: %s N=%d member %d seed %d rejected (no convergence or a Newton norm within %.2fx of tol)", kind, N, r, s, PE.FRAGILE)
        else:
            raise RuntimeError(f"member_cases: no usable transform for member {r} of {kind} N={N}")
    return dict(channel_seed=chan, tol=p.tol, member_seeds=seeds)


_built = {}


def oracle_members(kind, N, seed):
    """(Problem, dz_left, dz_main, dz_right [3, N], n_scale [3, 3], [member Problems], [oracle runs]) from the record; once per process"""
    key = f"{kind}-{N}-{seed}"
    if key not in _built:
        rec = json.load(open(CHOICES))[key]
        p = PE.BUILDERS[kind](N, np.random.default_rng(rec["channel_seed"]))
        p.tol = rec["tol"]
        draws = [member_draw(p, r, s) for r, s in enumerate(rec["member_seeds"])]
        dzl, dzm, dzr = (np.concatenate([d[0][q] for d in draws]) for q in range(3))
        ns = np.concatenate([d[0][3] for d in draws], axis=1)
        probs = [d[1] for d in draws]
        _built[key] = (p, dzl, dzm, dzr, ns, probs, [O.newton_run(q, trace=True, iterates=True) for q in probs])
    return _built[key]


# ---- shared by the GPU tests of the member batches ---------------------------------------------------------------------------------
def with_member_beds(b, p):
    """both boundaries of p with bed_level per member, from the batch's own bed levels"""
    beds = b.bed_levels()
    for side, bc, bed in ((A.UPSTREAM, p.us, beds[:, 0]), (A.DOWNSTREAM, p.ds, beds[:, -1])):
        spec = boundary_spec(bc, p.nt)
        if "bed_level" in spec.params:
            spec = BoundarySpec(spec.kind, dict(spec.params, bed_level=bed.copy()), spec.target)
        b.set_boundary(side, spec)


SWEEP_CASE = 57        # tests/golden/random_sweep.npz: 9 nodes of 8 .. 15 stations, flow hydrograph in, normal depth out, linear start


def mirror_solver(recipe, geo=None):
    """the mirror's solver of a sweep recipe; with geo (one member of member_sections) on that member's sections: every node an
    IrregularSection of the transformed polyline, the boundaries on the member's bed, the initial conditions set up again"""
    from oracle.gen_random_sweep import build_from_recipe
    from flowsim_amd.hydromodel.cross_section import IrregularSection, section_table
    solver, _, _ = build_from_recipe(recipe)
    if geo is None:
        return solver
    ch = solver.channel
    nodes = []
    for i, xs in enumerate(ch.xs_at_node):
        c = int(geo["irr_npts"][i])
        s = IrregularSection(geo["irr_x"][i, :c], geo["irr_z"][i, :c], bed_slope=xs.bed_slope, curvature=xs.curvature)
        s.n_left, s.n_main, s.n_right = float(geo["n_left"][i]), float(geo["n_main"][i]), float(geo["n_right"][i])
        s.left_fp_limit, s.right_fp_limit = geo["irr_limits"][i]
        nodes.append(s)
    ch.xs_at_node, ch.node_geometry = nodes, section_table(nodes)
    for bnd, s in ((ch.upstream_boundary, nodes[0]), (ch.downstream_boundary, nodes[-1])):
        bnd.cross_section, bnd.bed_level = s, s.z_min
    ch.initial_conditions = np.zeros((len(nodes), 2))
    {"linear": ch._linear_conditions, "GVF_equation": ch._gvf_conditions, "steady-state": ch._steady_conditions}[ch.interpolation_method](len(nodes), ch.initial_flow_rate)
    solver.initialize_t0()
    return solver
