"""Ensembles: many copies of one channel stepped together on the device.  Manning-n ensembles differ only in the main-channel
roughness; scenario ensembles (run_scenario_ensemble) in what the reach is forced with - inflow, pool level, outlets in service (BASELINE.json configs[3]; the reference does this one member at a
time, cases/gerd_roseires/n_calibrate.py:55-67 -> model.run(n_main=...))."""
import numpy as np

from . import _abi as A
from . import _pack as P
from .batch import BoundarySpec, PreissmannBatch
from .hydromodel.preissmann import boundary_to_spec


def _add_envelope(out, b, envelope, nt):
    """out['envelope'] and out['profile_bands'] of the runners' envelope= keyword"""
    unknown = set(envelope) - {"quantities", "threshold", "threshold_quantity", "quantiles"}
    if unknown:
        raise ValueError(f"envelope: unknown keys {sorted(unknown)}")
    env = b.envelope(envelope.get("quantities", ("stage",)), envelope.get("threshold"), envelope.get("threshold_quantity", "stage"), 0, nt)
    out["envelope"] = env
    out["profile_bands"] = {name: b.profile_bands(name, "max", envelope.get("quantiles", (0.05, 0.5, 0.95)))
                            for name in env if name not in ("levels", "crossing")}


def _step(b, n_steps, balance, history, gauges=None, dx=None):
    """the runners' time loop: one launch; with balance= or gauges= on a batch WITHOUT history, chunks of `every` levels with the state
    marked (PreissmannBatch.reach_integrals(current=True), PreissmannBatch.gauges(current=True)) before the first and after each -
    stream-ordered, the host does not wait.  One chunk loop serves both keywords.  gauges=: the gauges are set here, at the chainages
    given, dx apart the nodes."""
    every = threshold = None
    if balance is not None:
        every, threshold, _ = P.balance_options(balance)
    if gauges is not None:
        chainage, g_every = P.gauge_options(gauges)[:2]
        if every is not None and g_every != every:
            raise ValueError(f"balance= and gauges= mark the state at the same chunk boundaries: every={every} and every={g_every} differ")
        every = g_every
        b.set_gauges(chainage=chainage, dx=dx)
    if every is None or history:
        b.step(n_steps)
        return

    def mark():
        if balance is not None:
            b.reach_integrals(threshold=threshold, current=True)
        if gauges is not None:
            b.gauges(current=True)
    mark()
    for chunk in P.balance_chunks(n_steps, every):
        b.step(chunk, sync=False)
        mark()
    b.sync()


def _add_balance(out, b, balance, nt, history):
    """out['balance'] of the runners' balance= keyword: dict(rows, totals, bands)"""
    _, threshold, quantiles = P.balance_options(balance)
    if history:
        b.reach_integrals(0, nt, threshold=threshold)
    rows, totals = b.water_balance(0, nt)
    out["balance"] = dict(rows=rows, totals=totals, bands=b.integral_bands(quantiles, 0, nt))


def _add_gauges(out, b, gauges, nt, history):
    """out['gauges'] of the runners' gauges= keyword: dict(node, weight, rows [G, nt, 4, B] when asked for, bands: one
    PreissmannBatch.gauge_bands per gauge, score: one gauge_score per gauge when observed [G, nt] is given)"""
    chainage, _, quantiles, observed, signal, rows = P.gauge_options(gauges)
    G = len(chainage)
    if observed is not None and observed.shape != (G, nt):
        raise ValueError(f"gauges: observed must be [G, nt] = [{G}, {nt}], not {list(observed.shape)}")
    if history:
        b.gauges(0, nt)
    node, weight = b.gauge_positions
    res = dict(node=node, weight=weight)
    if rows:
        res["rows"] = np.stack([b.gauge_rows(g, 0, nt) for g in range(G)])
    res["bands"] = [b.gauge_bands(g, quantiles, 0, nt) for g in range(G)]
    if observed is not None:
        res["score"] = [b.gauge_score(g, signal, observed[g], 0, nt) for g in range(G)]
    out["gauges"] = res


def run_manning_ensemble(solver, n_main_values, tolerance=1e-4, max_iter=100, dtype="f64", device=0, monitor=True, initial="host",
                         summaries=False, score=None, bands=None, hydrographs=True, envelope=None, balance=None, gauges=None):
    """`solver`: a set-up (not yet run) PreissmannSolver whose channel provides geometry, boundaries
    and initial conditions; the initial conditions are shared by all members (the reference's
    members start from the same downstream level and the same flow; their GVF profiles differ
    with n - pass `initial_conditions[B, N, 2]` through `solver.channel.member_ics` to override).

    initial="gvf": every member starts from its own backwater profile instead, marched on the device from the channel's
    downstream depth with the member's n (PreissmannBatch.init_state; channel.py:307-378) - no per-member set-up on the host.

    Post-processing on the device, on the hydrograph block where it is (PreissmannBatch.summaries / lookup / bands):
    summaries=True adds 'summaries' (dict of [B]: the numbers of the reference's result summary, see summary_text);
    score=dict(xq, target=None, y_offset=None) adds 'score' (dict(values[n_q, B], rmse[B],
    monotone[B]): the members' upstream level at the flows xq and its RMSE against the target, n_calibrate.py:55-67);
    bands=(q, ...) adds 'bands' (min, max, mean, std [nt, 4], quantiles [nt, 4, n_q], n_members [nt] across the members);
    hydrographs=False leaves the block on the device - at 32 768 members and 385 levels it is 400 MB.

    Along the reach: envelope=dict(quantities=("stage",), threshold=None, threshold_quantity="stage", quantiles=(0.05, 0.5, 0.95))
    adds 'envelope' (PreissmannBatch.envelope over all levels: per member and node the extremes, their levels, the crossings of the
    threshold) and 'profile_bands' (dict name -> PreissmannBatch.profile_bands of that quantity's maxima across the members).  Its
    cost: the batch is created with history=True, which selects the step kernels compiled with diagnostics and holds the whole
    history, 2 * levels * B * N values, on the device.  With envelope=None nothing changes.

    Storage and mass balance: balance=dict(every=1, threshold=None, quantiles=(0.05, 0.5, 0.95)) adds 'balance' = dict(rows: per
    level and member the stored volume, the water surface, the length of reach at or above the stage `threshold` and the residual
    of the discrete water balance (PreissmannBatch.reach_integrals / water_balance), totals: per member, bands: integral_bands
    across the members).  With a history (envelope=) the whole range is reduced after the run; without one the run is stepped in
    chunks of `every` levels and the state is marked after each, so that the balance closes over each chunk and the rows between
    two marks are NaN.  With balance=None nothing changes.

    Stations inside the reach: gauges=dict(chainage=, every=1, quantiles=(0.05, 0.5, 0.95), observed=None, signal="stage", rows=True)
    adds 'gauges' = dict(node, weight: where the chainages [G] fall between the nodes; rows [G, nt, 4, B]: depth, flow, stage and
    velocity at every gauge (rows=False leaves them on the device); bands: per gauge, gauge_bands across the members; score: per
    gauge, gauge_score of `signal` against observed [G, nt], NaN where there is no observation).  With a history (envelope=) the
    whole range is evaluated after the run; without one the state is marked at the chunk boundaries balance= marks it at (the two
    must agree on `every`) and the rows between two marks are NaN.  With gauges=None nothing changes.

    Returns dict(hydrographs[nt, 4, B], iterations[nt, B], status[B]) and what the keywords above add."""
    if initial not in ("host", "gvf"):
        raise ValueError("initial must be 'host' or 'gvf'")
    ch = solver.channel
    n_vals = np.ascontiguousarray(n_main_values, dtype=np.float64)
    B, N, nt = len(n_vals), solver.number_of_nodes, solver.number_of_time_levels
    ics = getattr(ch, "member_ics", None)
    with PreissmannBatch(B, N, max(nt, 2), dtype=dtype, section_mode="table", device=device, monitor=monitor, history=envelope is not None) as b:
        b.set_scheme(solver.theta, solver.time_step, solver.spatial_step, tolerance, max_iter)
        b.set_geometry_table(ch.node_geometry, n_main_override=n_vals)
        b.set_boundary(A.UPSTREAM, boundary_to_spec(ch.upstream_boundary, max(nt, 2), solver.time_step))
        b.set_boundary(A.DOWNSTREAM, boundary_to_spec(ch.downstream_boundary, max(nt, 2), solver.time_step))
        if initial == "gvf":
            b.init_state("GVF_equation", ch.initial_flow_rate, depth_ds=ch.downstream_boundary.initial_depth)
        elif ics is None:
            b.set_state(ch.initial_conditions[:, 0], ch.initial_conditions[:, 1])
        else:
            b.set_state(ics[:, :, 0], ics[:, :, 1])
        _step(b, nt - 1, balance, envelope is not None, gauges, solver.spatial_step)
        out = dict(iterations=b.iterations(0, nt), status=b.status())
        if hydrographs:
            out = dict(hydrographs=b.hydrographs(0, nt), **out)
        if summaries:
            out["summaries"] = b.summaries(0, nt)
        if score is not None:
            out["score"] = b.lookup(A.ROW_Q_IN, A.ROW_H_IN, score["xq"],
                                    y_offset=score.get("y_offset"), target=score.get("target"), first=0, n=nt)
        if bands is not None:
            out["bands"] = b.bands(bands, 0, nt)
        if envelope is not None:
            _add_envelope(out, b, envelope, nt)
        if balance is not None:
            _add_balance(out, b, balance, nt, envelope is not None)
        if gauges is not None:
            _add_gauges(out, b, gauges, nt, envelope is not None)
        return out


def run_scenario_ensemble(solver, pool, inflow_table, inflow_scale=None, inflow_shift=None, pool_level=None, weir_scale=None, n_main=None,
                          initial="gvf", tolerance=1e-4, max_iter=100, dtype="f64", device=0, monitor=True, summaries=False, score=None,
                          bands=None, hydrographs=True, envelope=None, balance=None, gauges=None):
    """Scenario ensembles: members that differ in what the reach is forced with - the inflow into the reservoir upstream of it
    (`inflow_table` [K, 2], time [s] and flow, per member multiplied by inflow_scale and delayed by inflow_shift [s]), the pool
    level the reservoir starts from (pool_level, required; it is also the member's hold level), the outlets in service (weir_scale
    [n_weirs] or [n_weirs, B]: multipliers of the weir coefficients of `pool`, a forcing.PoolSpec) - and, optionally, in n_main.
    Scalars are shared, arrays [B] make the ensemble.  The reference does this one member at a time: GerdHydrograph.build
    (cases/gerd_roseires/gerd_discharge.py:12-56) and then model.run (model.py:36-113).

    Order: the inflow is sampled on the device (PreissmannBatch.set_boundary_sampled), routed through every member's pool
    (route_pool), row 0 of the release is each member's initial flow, from which its backwater profile is marched (init_state;
    initial="gvf" is the only choice), then step and reduce.  Nothing per member runs on the host.  `solver` is a set-up
    PreissmannSolver that provides the geometry, the scheme and the downstream boundary; its upstream boundary must be a flow
    hydrograph, whose own table is not read.  The downstream rating curve stays the SHARED smooth gate curve of `solver`, built as
    today from the default initial flow (model.py:79-81): it is not rebuilt per member.

    A member whose pool leaves the bracket (the reference's ValueError) carries POOL_NO_BRACKET in 'pool' and ends with status NAN.
    Post-processing keywords and what they add: as run_manning_ensemble (envelope= included, at the same cost: history=True; balance=).  Returns dict(hydrographs[nt, 4, B], iterations[nt, B],
    status[B], initial_flow[B], pool=dict(flags[B], level[B])) and what the keywords add."""
    if initial != "gvf":
        raise ValueError("initial must be 'gvf': every member starts from the backwater profile of its own release")
    if pool_level is None:
        raise ValueError("pool_level is required: the level every member's reservoir starts from")
    ch = solver.channel
    if ch.upstream_boundary.condition != "flow_hydrograph":
        raise ValueError("the upstream boundary of the solver must be a flow hydrograph")
    table = np.asarray(inflow_table, dtype=np.float64)
    sizes = {np.shape(v)[-1] for v in (inflow_scale, inflow_shift, pool_level, n_main, weir_scale)
             if v is not None and np.ndim(v) > 0 and not (v is weir_scale and np.ndim(v) == 1)}
    if len(sizes) > 1:
        raise ValueError(f"per-member arguments of different lengths: {sorted(sizes)}")
    B = sizes.pop() if sizes else 1
    N, nt = solver.number_of_nodes, solver.number_of_time_levels
    L = max(nt, 2)
    n_vals = None if n_main is None else np.ascontiguousarray(np.broadcast_to(np.asarray(n_main, dtype=np.float64), (B,)))
    with PreissmannBatch(B, N, L, dtype=dtype, section_mode="table", device=device, monitor=monitor, history=envelope is not None) as b:
        b.set_scheme(solver.theta, solver.time_step, solver.spatial_step, tolerance, max_iter)
        b.set_geometry_table(ch.node_geometry, n_main_override=n_vals)
        b.set_boundary_sampled(A.UPSTREAM, BoundarySpec(A.BC_FLOW_HYDROGRAPH), table[:, 0], table[:, 1], scale=inflow_scale, shift=inflow_shift)
        routed = b.route_pool(A.UPSTREAM, pool, pool_level, weir_scale=weir_scale)
        flow0 = b.bc_target(A.UPSTREAM, 0, 1)[0]
        b.set_boundary(A.DOWNSTREAM, boundary_to_spec(ch.downstream_boundary, L, solver.time_step))
        b.init_state("GVF_equation", flow0, depth_ds=ch.downstream_boundary.initial_depth)
        _step(b, nt - 1, balance, envelope is not None, gauges, solver.spatial_step)
        out = dict(iterations=b.iterations(0, nt), status=b.status(), initial_flow=flow0, pool=routed)
        if hydrographs:
            out = dict(hydrographs=b.hydrographs(0, nt), **out)
        if summaries:
            out["summaries"] = b.summaries(0, nt)
        if score is not None:
            out["score"] = b.lookup(A.ROW_Q_IN, A.ROW_H_IN, score["xq"],
                                    y_offset=score.get("y_offset"), target=score.get("target"), first=0, n=nt)
        if bands is not None:
            out["bands"] = b.bands(bands, 0, nt)
        if envelope is not None:
            _add_envelope(out, b, envelope, nt)
        if balance is not None:
            _add_balance(out, b, balance, nt, envelope is not None)
        if gauges is not None:
            _add_gauges(out, b, gauges, nt, envelope is not None)
        return out


def run_geometry_ensemble(solver, dz_left=None, dz_main=None, dz_right=None, n_scale=None, tolerance=1e-4, max_iter=100, dtype="f64",
                          device=0, monitor=True, summaries=False, score=None, bands=None, hydrographs=True, envelope=None, balance=None, gauges=None):
    """Geometry ensembles of a surveyed river: members that differ in the bed level of the main channel, the elevation of the left
    and right floodplain (levees included) and the three roughnesses.  `solver`: a set-up (not yet run) PreissmannSolver whose
    channel has polyline sections at every node; member r is that channel with the main-channel / left / right vertices of node i
    lifted by dz_main / dz_left / dz_right [r, i] ([B]: the same at every node; None: 0) and (n_left, n_main, n_right) multiplied by
    n_scale[0..2, r] ([3, B]; None: 1) - _pack.member_sections is the definition.  The reference builds one Channel per member.

    Everything per member is made on the device: polylines, bed levels and stage tables (PreissmannBatch.
    set_geometry_irregular_members), the initial state by the channel's own interpolation method on each member's geometry
    (init_state), and each boundary's bed_level is the member's own (bed_levels() of the end nodes).

    Keywords and return value: as run_manning_ensemble (dtype: polyline batches are fp64; envelope= at the same cost: history=True; balance=)."""
    ch = solver.channel
    geo = ch.node_geometry
    if "irr_npts" not in geo or np.any(np.asarray(geo["irr_npts"]) == 0):
        raise ValueError("run_geometry_ensemble needs a channel of polyline sections at every node")
    sizes = {np.shape(v)[-1 if v is n_scale else 0] for v in (dz_left, dz_main, dz_right, n_scale) if v is not None}
    if len(sizes) > 1:
        raise ValueError(f"per-member arguments of different lengths: {sorted(sizes)}")
    B = sizes.pop() if sizes else 1
    N, nt = solver.number_of_nodes, solver.number_of_time_levels
    L = max(nt, 2)
    with PreissmannBatch(B, N, L, dtype=dtype, section_mode="irregular", device=device, monitor=monitor, history=envelope is not None) as b:
        b.set_scheme(solver.theta, solver.time_step, solver.spatial_step, tolerance, max_iter)
        b.set_geometry_irregular_members(geo, dz_left, dz_main, dz_right, n_scale)
        beds = b.bed_levels()
        for side, boundary, bed in ((A.UPSTREAM, ch.upstream_boundary, beds[:, 0]), (A.DOWNSTREAM, ch.downstream_boundary, beds[:, -1])):
            spec = boundary_to_spec(boundary, L, solver.time_step)
            if "bed_level" in spec.params:         # a member's boundary row sees its own bed
                spec = BoundarySpec(spec.kind, dict(spec.params, bed_level=bed.copy()), spec.target)
            b.set_boundary(side, spec)
        method = ch.interpolation_method
        if method == "steady-state":
            b.init_state(method, ch.initial_flow_rate, bed_slope=[xs.bed_slope for xs in ch.xs_at_node])
        else:
            b.init_state(method, ch.initial_flow_rate, depth_ds=ch.downstream_boundary.initial_depth,
                         depth_us=ch.upstream_boundary.initial_depth if method == "linear" else None)
        _step(b, nt - 1, balance, envelope is not None, gauges, solver.spatial_step)
        out = dict(iterations=b.iterations(0, nt), status=b.status())
        if hydrographs:
            out = dict(hydrographs=b.hydrographs(0, nt), **out)
        if summaries:
            out["summaries"] = b.summaries(0, nt)
        if score is not None:
            out["score"] = b.lookup(A.ROW_Q_IN, A.ROW_H_IN, score["xq"],
                                    y_offset=score.get("y_offset"), target=score.get("target"), first=0, n=nt)
        if bands is not None:
            out["bands"] = b.bands(bands, 0, nt)
        if envelope is not None:
            _add_envelope(out, b, envelope, nt)
        if balance is not None:
            _add_balance(out, b, balance, nt, envelope is not None)
        if gauges is not None:
            _add_gauges(out, b, gauges, nt, envelope is not None)
        return out


def summary_text(summaries, r, time_step, spatial_step, duration):
    """Member r's result summary in the reference's words (solver.py:188-233; Solver.summary writes the same block from a
    single-channel run) from the numbers PreissmannBatch.summaries computed on the device."""
    from .hydromodel.solver import summary_block
    s = summaries
    return summary_block(spatial_step, time_step, duration, s["q_net"][r], s["q_in"][r], s["peak_q_in"][r], s["peak_q_out"][r],
                         s["median_in_level"][r], s["median_out_level"][r])


def gvf_profiles(channel, n_main_values):
    """Initial depth profiles of every ensemble member at once: the reference's GVF backwater march
    (channel.py:307-378, Heun predictor-corrector from the downstream depth) vectorised over the
    members - they share the geometry table and differ in the main-channel Manning n.
    Returns initial_conditions[B, N, 2]."""
    from .hydromodel import cross_section as XS
    from .hydromodel import hydraulics
    geo = channel.node_geometry
    n_vals = np.asarray(n_main_values, dtype=np.float64)
    B, N = len(n_vals), len(geo["z_bed"])
    Q = channel.initial_flow_rate
    dx = channel.length / (N - 1)

    def node_geo(i):
        g = {k: np.full(B, v[i]) for k, v in geo.items()}
        g["n_main"] = n_vals          # the override is applied to every input section (custom_functions.py:147)
        return g

    def slope(h, i, S0):
        g = node_geo(i)
        hw = h + g["z_bed"]
        A, P, R, T, over = XS.props(g, hw)
        K = XS.conveyance(g, hw, (A, P, R, T, over))
        Fr = hydraulics.froude_array(T, A, Q)
        if np.any(Fr > 1.0):
            raise RuntimeError(f"GVF Error: Flow became supercritical at node {i}. "
                               "Downstream boundary control is not valid for this Q.")
        den = np.maximum(1 - Fr ** 2, 0.01)
        Se = Q * abs(Q) / K ** 2
        curv = g["curvature"]
        if np.any(curv != 0):
            neq = XS.equivalent_n(g, hw, (A, P, R, T, over), K)
            with np.errstate(divide="ignore", invalid="ignore"):
                f = hydraulics.darcy_weisbach_f(neq, R)
                Sc = (2.86 * np.sqrt(f) + 2.07 * f) * h ** 2 * Fr ** 2 / ((0.565 + np.sqrt(f)) * (1.0 / curv) ** 2)
            Se = Se + np.where(curv != 0, Sc, 0.0)
        return np.where((T < 1e-6) | (A < 1e-6), 0.0, (S0 - Se) / den)

    ic = np.empty((B, N, 2))
    ic[:, :, 1] = Q
    h = np.full(B, channel.downstream_boundary.initial_depth, dtype=np.float64)
    ic[:, N - 1, 0] = h
    z = geo["z_bed"]
    for i in reversed(range(N - 1)):
        S0 = (z[i] - z[i + 1]) / dx
        k1 = slope(h, i + 1, S0)
        h_pred = h - k1 * dx
        h_pred = np.where(h_pred <= 0, 0.01, h_pred)
        k2 = slope(h_pred, i, S0)
        h = h - 0.5 * (k1 + k2) * dx
        h = np.where(h <= 0, 0.01, h)
        ic[:, i, 0] = h
    return ic
