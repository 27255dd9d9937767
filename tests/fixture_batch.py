"""Builds a PreissmannBatch (the HIP product path, through the C ABI) from a golden fixture."""
import numpy as np

from flowsim_amd import BoundarySpec, PreissmannBatch
from flowsim_amd import _abi as A
from oracle import preissmann_oracle as O


def boundary_spec(bc: O.BC, nt):
    k = bc.kind
    if k == "flow_hydrograph":
        return BoundarySpec(A.BC_FLOW_HYDROGRAPH, {}, bc.target)
    if k == "stage_hydrograph":
        return BoundarySpec(A.BC_STAGE_HYDROGRAPH, dict(bed_level=bc.bed_level), bc.target)
    if k == "fixed_depth" and bc.storage is None:
        return BoundarySpec(A.BC_FIXED_DEPTH, dict(initial_depth=bc.initial_depth))
    if k == "fixed_depth" and any(bc.storage.get(x) is not None for x in ("curve", "rc", "losses")):
        s = bc.storage
        p = dict(min_stage=s["min_stage"], Y_min=s["Y_min"], Y_max=s["Y_max"], bed_level=bc.bed_level,
                 surface_area=s.get("area") or 0.0)
        if s.get("curve") is not None:
            p.update(curve=s["curve"], alpha=s["alpha"], beta=s["beta"])
        if s.get("rc") is not None:
            rc = s["rc"]
            p.update(rc_type=1.0 if rc["type"] == "power" else 2.0, rc_a=rc["a"], rc_b=rc["b"], rc_c=rc.get("c", 0.0),
                     rc_shift=rc.get("shift", 0.0))
        if s.get("losses") is not None:
            p.update(capture_losses=1.0, reservoir_length=s["losses"]["reservoir_length"], K_q=s["losses"]["K_q"])
        return BoundarySpec(A.BC_STORAGE_CURVE, p)
    if k == "fixed_depth":
        s = bc.storage
        return BoundarySpec(A.BC_STORAGE, dict(surface_area=s["area"], min_stage=s["min_stage"], Y_min=s["Y_min"],
                                               Y_max=s["Y_max"], bed_level=bc.bed_level))
    if k == "normal_depth":
        return BoundarySpec(A.BC_NORMAL_DEPTH, dict(bed_slope=bc.bed_slope, bed_level=bc.bed_level))
    if k == "rating_curve":
        rc = bc.rc
        if bc.rc_type == "power":
            return BoundarySpec(A.BC_RATING_POWER, dict(a=rc["a"], b=rc["b"], stage_shift=rc.get("shift", 0.0),
                                                        bed_level=bc.bed_level))
        if bc.rc_type == "polynomial":
            return BoundarySpec(A.BC_RATING_POLY, dict(a=rc["a"], b=rc["b"], c=rc["c"],
                                                       stage_shift=rc.get("shift", 0.0), bed_level=bc.bed_level))
        return BoundarySpec(A.BC_RATING_BLEND, dict(stage0=rc["initial_stage"], buffer=rc["buffer"],
                                                    lo0=rc["low"][0], lo1=rc["low"][1], lo2=rc["low"][2],
                                                    hi0=rc["high"][0], hi1=rc["high"][1], hi2=rc["high"][2],
                                                    dY=rc.get("dY", 1e-3), bed_level=bc.bed_level))
    raise ValueError(k)


def merge_specs(specs, B):
    """Per-reach parameter arrays from a list of B single-reach specs of the same kind."""
    kind = specs[0].kind
    assert all(s.kind == kind for s in specs)
    if kind == A.BC_STORAGE_CURVE:
        if B == 1:
            return specs[0]
        # one reservoir per reach (round 4): scalars [B], area curves [B, n_curve, 2] with the same number of points
        keys = sorted({k for s in specs for k in s.params if k != "curve"})
        params = {k: np.array([float(s.params.get(k) or (1.0 if k == "alpha" else 0.0)) for s in specs]) for k in keys}
        curves = [np.asarray(s.params.get("curve", np.empty((0, 2))), dtype=np.float64).reshape(-1, 2) for s in specs]
        assert len({len(c) for c in curves}) == 1, "the area curves of one batch need the same number of points"
        params["curve"] = np.stack(curves)
        return BoundarySpec(kind, params)
    params = {k: np.array([s.params[k] for s in specs], dtype=np.float64) for k in specs[0].params}
    tgt = None
    if specs[0].target is not None:
        tgt = np.stack([np.asarray(s.target, dtype=np.float64) for s in specs], axis=1)
    return BoundarySpec(kind, params, tgt)


def is_rect_uniform(p: O.Problem):
    g = p.geo
    # interpolated n / b of a prismatic channel can differ by an ulp from node to node (n*w1 + n*w2)
    flat = lambda a: np.ptp(a) <= 1e-13 * np.max(np.abs(a))
    return (np.all(g["is_compound"] < 0.5) and np.all(g["m_main"] == 0) and np.all(g["curvature"] == 0)
            and flat(g["b_main"]) and flat(g["n_main"]))


def batch_from_problems(problems, mode="auto", dtype="f64", history=True, n_main_override=None, monitor=None, trace=False):
    """One batch from a list of oracle Problems that share N, nt and the scheme parameters.  monitor=None: as the history flag (a
    test that leaves the history out wants the step kernels compiled without diagnostics, the bench shapes)."""
    monitor = history if monitor is None else monitor
    p0 = problems[0]
    B = len(problems)
    if mode == "auto":
        general_storage = any(boundary_spec(bc, p0.nt).kind == A.BC_STORAGE_CURVE for bc in (p0.us, p0.ds))
        mode = "rect_uniform" if all(is_rect_uniform(p) for p in problems) and not general_storage else "table"
        if "irr_npts" in p0.geo and np.any(p0.geo["irr_npts"] > 0):
            mode = "irregular"
        if mode != "rect_uniform" and B > 1:
            assert all(all(np.array_equal(p.geo[k], p0.geo[k]) for k in O.GEO_KEYS) for p in problems), \
                "TABLE geometry is shared by the batch: reaches with their own channel need their own batch"
    b = PreissmannBatch(B, p0.N, p0.nt, dtype=dtype, section_mode=mode, history=history, monitor=monitor, trace=trace)
    b.set_scheme(p0.theta, p0.dt, p0.dx, p0.tol, p0.max_iter)
    if mode == "rect_uniform":
        b.set_geometry_uniform([p.geo["b_main"][0] for p in problems], [p.geo["n_main"][0] for p in problems],
                               [p.geo["z_bed"][0] for p in problems], [p.geo["z_bed"][-1] for p in problems])
    elif mode == "trap_uniform":
        b.set_geometry_uniform([p.geo["b_main"][0] for p in problems], [p.geo["n_main"][0] for p in problems],
                               [p.geo["z_bed"][0] for p in problems], [p.geo["z_bed"][-1] for p in problems],
                               side_slope=[p.geo["m_main"][0] for p in problems])
    elif mode == "irregular":
        b.set_geometry_irregular(p0.geo, n_main_override)
    else:
        b.set_geometry_table(p0.geo, n_main_override)
    b.set_boundary(A.UPSTREAM, merge_specs([boundary_spec(p.us, p.nt) for p in problems], B))
    b.set_boundary(A.DOWNSTREAM, merge_specs([boundary_spec(p.ds, p.nt) for p in problems], B))
    b.set_state(np.stack([p.h0 for p in problems]), np.stack([p.Q0 for p in problems]))
    return b


def hetero_batch_from_problems(problems, mode="table", history=True, monitor=None, dtype="f64"):
    """ONE batch from oracle Problems that share nothing: every reach its own channel (node table), node
    count, theta / dt / dx, tolerance / iteration cap, boundary kinds and number of levels (fs_batch_set_geometry_table_per_reach, fs_batch_set_reach_nodes,
    fs_batch_set_reach_scheme, fs_batch_set_bc_per_reach).  Rows of shorter reaches are padded with their last node.  dtype: the
    per-reach table setter serves fp32 batches too (the per-reach polyline setters do not: per_reach_polyline_batch has no dtype)."""
    B, N, L = len(problems), max(p.N for p in problems), max(p.nt for p in problems)
    p0 = problems[0]

    def pad(a):
        a = np.asarray(a, dtype=np.float64)
        return np.concatenate([a, np.full(N - len(a), a[-1])])
    b = PreissmannBatch(B, N, L, dtype=dtype, section_mode=mode, history=history, monitor=history if monitor is None else monitor)
    b.set_scheme(p0.theta, p0.dt, p0.dx, p0.tol, p0.max_iter)
    b.set_geometry_table({k: np.stack([pad(p.geo[k]) for p in problems]) for k in A.GEO_ROWS})
    b.set_reach_nodes([p.N for p in problems])
    b.set_reach_scheme([p.theta for p in problems], [p.dt for p in problems], [p.dx for p in problems])
    if any(p.tol != p0.tol or p.max_iter != p0.max_iter for p in problems):
        b.set_reach_tolerance([p.tol for p in problems], [p.max_iter for p in problems])
    b.set_boundary_per_reach(A.UPSTREAM, [boundary_spec(p.us, p.nt) for p in problems])
    b.set_boundary_per_reach(A.DOWNSTREAM, [boundary_spec(p.ds, p.nt) for p in problems])
    b.set_state(np.stack([pad(p.h0) for p in problems]), np.stack([pad(p.Q0) for p in problems]))
    return b


def per_reach_polyline_batch(probs, history=True, monitor=True):
    """ONE batch, every reach its own polylines (and stage tables), node count and boundary parameters; rows of a shorter reach
    are padded by repeating its last node (include/flowsim_abi.h: fs_batch_set_geometry_irregular_per_reach).  history=False,
    monitor=False: the shapes of the no-diagnostics kernels."""
    B, N, L = len(probs), max(p.N for p in probs), max(p.nt for p in probs)
    P = max(p.geo["irr_x"].shape[1] for p in probs)
    p0 = probs[0]

    def pad_nodes(a):
        a = np.asarray(a)
        return np.concatenate([a, np.repeat(a[-1:], N - len(a), axis=0)], axis=0)

    def pad_pts(a, n_pts):          # [n, p] -> [n, P]: columns beyond a node's own count repeat its last station
        a = np.asarray(a, dtype=np.float64)
        return np.concatenate([a, np.repeat(a[:, -1:], P - a.shape[1], axis=1)], axis=1) if a.shape[1] < P else a
    geo = {k: np.stack([pad_nodes(p.geo[k]) for p in probs]) for k in A.GEO_ROWS}
    geo["irr_npts"] = np.stack([pad_nodes(p.geo["irr_npts"]) for p in probs]).astype(np.int32)
    geo["irr_x"] = np.stack([pad_nodes(pad_pts(p.geo["irr_x"], None)) for p in probs])
    geo["irr_z"] = np.stack([pad_nodes(pad_pts(p.geo["irr_z"], None)) for p in probs])
    geo["irr_limits"] = np.stack([pad_nodes(p.geo["irr_limits"]) for p in probs])
    b = PreissmannBatch(B, N, L, section_mode="irregular", history=history, monitor=monitor)
    b.set_scheme(p0.theta, p0.dt, p0.dx, p0.tol, p0.max_iter)
    b.set_geometry_irregular(geo)
    b.set_reach_nodes([p.N for p in probs])
    b.set_boundary_per_reach(A.UPSTREAM, [boundary_spec(p.us, p.nt) for p in probs])
    b.set_boundary_per_reach(A.DOWNSTREAM, [boundary_spec(p.ds, p.nt) for p in probs])
    b.set_state(np.stack([pad_nodes(p.h0) for p in probs]), np.stack([pad_nodes(p.Q0) for p in probs]))
    return b
