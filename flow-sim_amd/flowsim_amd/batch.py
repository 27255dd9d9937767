"""PreissmannBatch - B independent reaches advanced together on one MI355X through the C ABI.

Host-side mirror of the state the reference's PreissmannSolver carries (preissmann.py:23-59,
solver.py:11-51): scheme parameters, node geometry, two boundaries, initial conditions; `step(n)`
is the batched equivalent of n passes of the outer loop of PreissmannSolver.run
(preissmann.py:108-161).  All arithmetic happens in the HIP kernels.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np

from . import _abi as A
from . import _pack as P
from ._pack import _KIND_PARAMS  # noqa: F401  (the parameter names per boundary kind)


@dataclass
class BoundarySpec:
    """One boundary of every reach in the batch (Boundary, boundary.py:10-46, flattened).

    params: dict name -> scalar (shared by all reaches) or array [B] (per reach); the names per
    kind are in _KIND_PARAMS.  target: hydrograph pre-sampled at level*dt, [n_levels] (shared) or
    [n_levels, B]."""
    kind: int
    params: dict = field(default_factory=dict)
    target: Optional[np.ndarray] = None


def _dptr(a):
    return a.ctypes.data_as(A._D)


def _iptr(a):
    return a.ctypes.data_as(A._I)


def _opt(a):
    """an optional array argument: NULL where the caller gave none"""
    return None if a is None else _dptr(a)


class PreissmannBatch:
    def __init__(self, n_reaches: int, n_nodes: int, max_levels: int, dtype: str = "f64",
                 section_mode: str = "rect_uniform", device: int = 0, history: bool = False, trace: bool = False,
                 monitor: bool = True):
        """monitor: the conditioning monitor of the on-chip elimination (status ILL_CONDITIONED, the stand-in for the reference's
        `diagnos` check, preissmann.py:133-144) runs on every batch unless the caller opts out - a batch without history or
        trace then runs the step kernels compiled without diagnostics (1 - 3 % faster on the benchmark shapes; bench.py does)."""
        self.B, self.N, self.L = int(n_reaches), int(n_nodes), int(max_levels)
        self.dtype = {"f64": A.F64, "f32": A.F32}[dtype]
        self.mode = {"rect_uniform": A.SEC_RECT_UNIFORM, "trap_uniform": A.SEC_TRAP_UNIFORM,
                     "table": A.SEC_TABLE, "irregular": A.SEC_IRREGULAR}[section_mode]
        self._lib = A.lib()
        desc = A.BatchDesc(self.B, self.N, self.dtype, self.mode, device, self.L,
                           (A.FLAG_HISTORY if history else 0) | (A.FLAG_TRACE if trace else 0) | (A.FLAG_MONITOR if monitor else 0), 0)
        self._h = self._lib.fs_batch_create(C.byref(desc))
        if not self._h:
            raise A.FlowsimError(A.last_error())
        self.history = history
        self._max_pts = 0           # stations per polyline row of the geometry on the device (stage_table)
        self._envelope = ((), False)      # what the envelope on the handle holds: quantity names, crossing rows
        self.gauge_positions = None       # (node, weight) of set_gauges

    # -- lifetime -------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.fs_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- setup ----------------------------------------------------------------------------
    def set_scheme(self, theta, dt, dx, tolerance=1e-4, max_iter=100):
        A.check(self._lib.fs_batch_set_scheme(self._h, float(theta), float(dt), float(dx), float(tolerance),
                                              int(max_iter)), "set_scheme")

    def set_geometry_uniform(self, width, manning, z_us, z_ds, side_slope=None):
        p = P.uniform_params(self.mode == A.SEC_TRAP_UNIFORM, self.B, width, manning, z_us, z_ds, side_slope)
        A.check(self._lib.fs_batch_set_geometry_uniform(self._h, _dptr(p)), "set_geometry_uniform")

    def set_geometry_table(self, geo: dict, n_main_override: Optional[Sequence[float]] = None):
        """geo[k]: [N] (one channel shared by the batch) or [B, N] (one channel per reach: geometry ensembles, different
        rivers; rows of a shorter reach padded by repeating its last node, see set_reach_nodes)"""
        per_reach = any(np.ndim(geo[k]) == 2 for k in A.GEO_ROWS)
        tab, ov = P.geometry_table(geo, self.B, self.N, per_reach), P.n_override(n_main_override, self.B)
        fn = self._lib.fs_batch_set_geometry_table_per_reach if per_reach else self._lib.fs_batch_set_geometry_table
        A.check(fn(self._h, _dptr(tab), _opt(ov)), "set_geometry_table")

    def set_reach_nodes(self, n_nodes):
        """per-reach node counts (<= N of the batch): each reach its own channel length / grid (solver.py:34-38, :53-55)"""
        n = np.ascontiguousarray(n_nodes, dtype=np.int32)
        assert n.shape == (self.B,)
        A.check(self._lib.fs_batch_set_reach_nodes(self._h, _iptr(n)), "set_reach_nodes")

    def set_reach_scheme(self, theta=None, dt=None, dx=None):
        """per-reach theta / time step / spatial step (arrays [B]; None: the batch-wide value of set_scheme)"""
        arrs = [P.opt_per_reach(v, self.B) for v in (theta, dt, dx)]
        A.check(self._lib.fs_batch_set_reach_scheme(self._h, *[_opt(a) for a in arrs]), "set_reach_scheme")

    def set_reach_tolerance(self, tolerance=None, max_iter=None):
        """per-reach convergence tolerance and iteration cap (arrays [B]; None: the batch-wide value of set_scheme): what each
        run(tolerance=, max_iter=) of the reference has of its own (preissmann.py:101)"""
        tol, mit = P.opt_per_reach(tolerance, self.B), P.opt_per_reach(max_iter, self.B, np.int32)
        A.check(self._lib.fs_batch_set_reach_tolerance(self._h, _opt(tol), None if mit is None else _iptr(mit)), "set_reach_tolerance")

    def set_boundary_per_reach(self, side: int, specs):
        """one BoundarySpec per reach, kinds free to differ: the closed-form kinds BC_FLOW_HYDROGRAPH .. BC_STORAGE and, in table /
        polyline batches, BC_STORAGE_CURVE (a general reservoir behind some of the channels, each with its own scalars and an area
        curve of its own length) and BC_HOST_ROW on the reaches whose plugin has no device form (such a batch advances with
        iterate(), and set_host_rows() writes the rows of those reaches only); a spec's target is [n_levels] (sampled at that
        reach's own k * dt)"""
        kinds, p, rows = P.bc_params_per_reach(specs, self.B)
        tgt = P.bc_target_per_reach([s.target for s in specs], self.L, self.B)
        A.check(self._lib.fs_batch_set_bc_per_reach_wide(self._h, side, _iptr(kinds), _dptr(p), rows, _opt(tgt)), "set_boundary_per_reach")

    def set_geometry_irregular(self, geo: dict, n_main_override: Optional[Sequence[float]] = None):
        """geo: the TABLE rows plus irr_x / irr_z [N, P] (rows padded beyond irr_npts), irr_npts [N]
        (0 = trapezoid-family node) and irr_limits [N, 2] (IrregularSection.left/right_fp_limit); one channel per reach:
        irr_npts [B, N], irr_x / irr_z [B, N, P], irr_limits [B, N, 2]"""
        tab, cnt, x, z, lim, per_reach = P.irregular_arrays(geo, self.B, self.N)
        ov = P.n_override(n_main_override, self.B)
        fn = self._lib.fs_batch_set_geometry_irregular_per_reach if per_reach else self._lib.fs_batch_set_geometry_irregular
        A.check(fn(self._h, _dptr(tab), _iptr(cnt), x.shape[-1], _dptr(x), _dptr(z), _dptr(lim), _opt(ov)), "set_geometry_irregular")
        self._max_pts = x.shape[-1]

    def set_geometry_irregular_members(self, geo: dict, dz_left=None, dz_main=None, dz_right=None, n_scale=None):
        """A geometry ensemble of ONE polyline channel (geo as set_geometry_irregular takes a shared channel, every node a
        polyline): member r is the channel with its left-strip, main-channel and right-strip vertices of node i lifted by
        dz_left / dz_main / dz_right [r, i] ([B]: the same shift at every node; None: 0) and its (n_left, n_main, n_right) multiplied
        by n_scale[0..2, r] ([3, B]; None: 1) - _pack.member_sections is the definition.  The members' polylines, bed levels and
        stage tables are built on the device; the batch is then where set_geometry_irregular(_pack.member_sections(...)) leaves it."""
        tab, cnt, x, z, lim, dl, dm, dr, ns = P.member_arrays(geo, self.B, self.N, dz_left, dz_main, dz_right, n_scale)
        A.check(self._lib.fs_batch_set_geometry_irregular_members(self._h, _dptr(tab), _iptr(cnt), x.shape[-1], _dptr(x), _dptr(z), _dptr(lim),
                                                                  _opt(dl), _opt(dm), _opt(dr), _opt(ns)), "set_geometry_irregular_members")
        self._max_pts = x.shape[-1]

    def stage_table(self, reach: int, node: int):
        """the node's stage table as fs::build_stage_table orders it: breakpoints padded with +inf, then 32 numbers per interval
        (FlowsimError for a batch that walks its polylines' edges)"""
        out = np.empty(((self._max_pts + 16) & ~15) + 32 * self._max_pts)
        A.check(self._lib.fs_batch_get_stage_table(self._h, int(reach), int(node), _dptr(out)), "stage_table")
        return out

    def bed_levels(self):
        """[B, N]: every reach's bed levels as the kernels read them (table and polyline batches)"""
        out = np.empty((self.B, self.N))
        A.check(self._lib.fs_batch_get_bed_levels(self._h, _dptr(out)), "bed_levels")
        return out

    def set_boundary(self, side: int, spec: BoundarySpec):
        """one kind for the batch, its parameters shared or [B]; BC_HOST_ROW and BC_STORAGE_CURVE follow no hydrograph"""
        p, n_params, per_reach = P.bc_params(spec, self.B)
        tgt = None if spec.kind in (A.BC_HOST_ROW, A.BC_STORAGE_CURVE) else P.bc_target(spec.target, self.L, self.B)
        A.check(self._lib.fs_batch_set_bc(self._h, side, spec.kind, _opt(p), n_params, per_reach, _opt(tgt)), "set_boundary")

    def set_boundary_sampled(self, side: int, spec: BoundarySpec, times, values, table_of=None, scale=None, offset=None, shift=None):
        """set_boundary for a flow or stage hydrograph whose target is sampled on the device: member r follows
        offset[r] + scale[r] * np.interp(k * dt_r - shift[r], times, values[table_of[r]]) - Hydrograph.sample (hydrograph.py:26-32)
        of a table the member scales, lifts and delays.  values: [K] or [n_tables, K]; table_of, scale, offset, shift: None, a scalar
        or [B].  spec.target is not read.  Call after set_scheme (and set_reach_scheme, where used)."""
        p, n_params, per_reach = P.bc_params(spec, self.B)
        if per_reach:
            raise ValueError("set_boundary_sampled takes parameters shared by the batch")
        t, v = P.sample_tables(times, values)
        idx = P.table_index(table_of, v.shape[0], self.B)
        sc, off, sh = (P.opt_per_reach(a, self.B) for a in (scale, offset, shift))
        A.check(self._lib.fs_batch_set_bc_sampled(self._h, side, spec.kind, _opt(p), n_params, _dptr(t), _dptr(v), t.size, v.shape[0],
                                                  None if idx is None else _iptr(idx), _opt(sc), _opt(off), _opt(sh)), "set_boundary_sampled")

    def route_pool(self, side: int, pool, initial_stage, weir_scale=None):
        """Level-pool routing of the side's flow target through `pool` (forcing.PoolSpec), every member from its own initial_stage
        (scalar or [B]; it is also the member's hold level): GerdHydrograph.build (gerd_discharge.py:12-56) for the whole batch on the
        device.  The target becomes the release, pool_stages() the pool's stage.  weir_scale: None, [n_weirs] or [n_weirs, B]
        multipliers of the weir coefficients (0: out of service).  Returns dict(flags[B]: POOL_* bits, level[B]: the first level at
        which brentq had no bracket, else -1); such a member's rows are NaN from that level on."""
        z, v, w = pool.arrays()
        z0 = P.per_reach(initial_stage, self.B)
        ws = P.weir_scale(weir_scale, len(w), self.B)
        info = np.empty((2, self.B), dtype=np.int32)
        A.check(self._lib.fs_batch_route_pool(self._h, side, _dptr(z), _dptr(v), z.size, _dptr(w), len(w), float(pool.base_flow),
                                              float(pool.vol_scale), float(pool.z_lo), float(pool.z_hi), _dptr(z0), _opt(ws), _iptr(info)),
                "route_pool")
        return dict(flags=info[0].copy(), level=info[1].copy())

    def bc_target(self, side: int, first=0, n=None):
        """[n, B]: rows of the side's target as the kernels read it (n None: all max_levels)"""
        n = self.L - first if n is None else n
        out = np.empty((n, self.B))
        A.check(self._lib.fs_batch_get_bc_target(self._h, side, int(first), int(n), _dptr(out)), "get_bc_target")
        return out

    def pool_stages(self, first=0, n=None):
        """[n, B]: the pool stage per level of the last route_pool (n None: all max_levels)"""
        n = self.L - first if n is None else n
        out = np.empty((n, self.B))
        A.check(self._lib.fs_batch_get_pool_stages(self._h, int(first), int(n), _dptr(out)), "get_pool_stages")
        return out

    def set_state(self, h, Q):
        h, Q = P.per_node(h, self.B, self.N), P.per_node(Q, self.B, self.N)
        A.check(self._lib.fs_batch_set_state(self._h, _dptr(h), _dptr(Q)), "set_state")

    def set_state_uniform(self, h, Q):
        """Steady-state IC of prismatic reaches: one depth and one flow per reach (channel.py:296-305)."""
        h, Q = P.per_reach(h, self.B), P.per_reach(Q, self.B)
        A.check(self._lib.fs_batch_set_state_uniform(self._h, _dptr(h), _dptr(Q)), "set_state_uniform")

    IC_METHODS = {"linear": A.IC_LINEAR, "GVF_equation": A.IC_GVF, "steady-state": A.IC_STEADY}      # Channel's interpolation_method names

    def init_state(self, method, flow, depth_ds=None, depth_us=None, bed_slope=None, strict=True):
        """Channel.initialize_conditions (channel.py:107-138) on the device, for every reach at once, on the geometry the batch
        holds: method 'linear' (depth_us, depth_ds), 'GVF_equation' (depth_ds: the backwater march) or 'steady-state' (normal depth;
        bed_slope [N] or [B, N]: the nodes' interpolated CrossSection.bed_slope, None in the uniform modes).  flow, depth_*: scalar
        or [B].  The batch is then where set_state(*state) would leave it.

        Returns dict(flags[B], node[B]): the IC_* bits of each reach and the node of its first supercritical evaluation (-1).
        strict=True raises the reference's RuntimeError for the first reach whose march met Fr > 1 (its depth is NaN upstream
        of that node; the other reaches are complete)."""
        flow, depth_ds, depth_us = P.per_reach(flow, self.B), P.opt_per_reach(depth_ds, self.B), P.opt_per_reach(depth_us, self.B)
        bed_slope, per_reach = P.bed_slope(bed_slope, self.B, self.N)
        info = np.empty((2, self.B), dtype=np.int32)
        A.check(self._lib.fs_batch_init_state(self._h, self.IC_METHODS[method], _dptr(flow), _opt(depth_us), _opt(depth_ds), _opt(bed_slope),
                                              per_reach, _iptr(info)), "init_state")
        out = dict(flags=info[0].copy(), node=info[1].copy())
        bad = np.flatnonzero(out["flags"] & A.IC_SUPERCRITICAL)
        if strict and len(bad):
            r = int(bad[0])
            raise RuntimeError(f"GVF Error: Flow became supercritical (Fr>1) at node {int(out['node'][r])} of reach {r}. "
                               "Downstream boundary control is not valid for this Q.")
        return out

    # -- the hot path ---------------------------------------------------------------------
    def step(self, n_steps: int = 1, sync: bool = True):
        A.check(self._lib.fs_batch_step(self._h, int(n_steps)), "step")
        if sync:
            self.sync()

    def sync(self):
        A.check(self._lib.fs_batch_sync(self._h), "sync")

    def iterate(self) -> int:
        """One Newton iteration of level `level + 1` for every reach still iterating on it; returns how many
        remain open (0: the level is complete and `level` has advanced)."""
        n = C.c_int32()
        A.check(self._lib.fs_batch_iterate(self._h, C.byref(n)), "iterate")
        return n.value

    def set_host_rows(self, side: int, dh, dq, res):
        """Boundary row (d/dh, d/dQ, residual) of every reach at the current Newton vector (BC_HOST_ROW sides; with per-reach
        kinds the entries of the reaches whose boundary the device evaluates are ignored)."""
        A.check(self._lib.fs_batch_set_host_rows(self._h, side, _dptr(P.host_rows(dh, dq, res, self.B))), "set_host_rows")

    def boundary_iterate(self):
        """[4, B]: h[0], Q[0], h[N-1], Q[N-1] of the current Newton vector."""
        out = np.empty((4, self.B))
        A.check(self._lib.fs_batch_get_boundary_iterate(self._h, _dptr(out)), "get_boundary_iterate")
        return out

    def restart(self, level: int, h, Q, h_guess, Q_guess, storage_stage=None):
        """Continue bit-exactly from `level`: state, Newton start vector of level + 1 and reservoir stage."""
        arrs = [P.per_node(a, self.B, self.N) for a in (h, Q, h_guess, Q_guess)]
        st = P.opt_per_reach(storage_stage, self.B)
        A.check(self._lib.fs_batch_restart(self._h, int(level), *[_dptr(a) for a in arrs], _opt(st)), "restart")

    @property
    def level(self):
        return self._lib.fs_batch_level(self._h)

    def _span(self, first, n):
        """the level count of a [first, first + n) range: up to the current level unless given"""
        return self.level - first + 1 if n is None else n

    # -- results --------------------------------------------------------------------------
    def state(self, out=None):
        """depth[k], flow[k] of the current level, [B, N] each; out=(h, Q): filled in place (a caller that downloads every few
        levels reuses its buffers instead of paying the page faults of fresh ones each time)"""
        h, Q = out if out is not None else (np.empty((self.B, self.N)), np.empty((self.B, self.N)))
        assert h.shape == Q.shape == (self.B, self.N) and h.dtype == Q.dtype == np.float64 and h.flags.c_contiguous and Q.flags.c_contiguous
        A.check(self._lib.fs_batch_get_state(self._h, _dptr(h), _dptr(Q)), "get_state")
        return h, Q

    def guess(self):
        h = np.empty((self.B, self.N)); Q = np.empty((self.B, self.N))
        A.check(self._lib.fs_batch_get_guess(self._h, _dptr(h), _dptr(Q)), "get_guess")
        return h, Q

    def hydrographs(self, first=0, n=None):
        """[n, 4, B]: depth[k,0], flow[k,0], depth[k,-1], flow[k,-1]."""
        n = self._span(first, n)
        out = np.empty((n, 4, self.B))
        A.check(self._lib.fs_batch_get_hydrographs(self._h, first, n, _dptr(out)), "get_hydrographs")
        return out

    def iterations(self, first=0, n=None):
        n = self._span(first, n)
        out = np.empty((n, self.B), dtype=np.int32)
        A.check(self._lib.fs_batch_get_iterations(self._h, first, n, _iptr(out)), "get_iterations")
        return out

    def status(self):
        out = np.empty(self.B, dtype=np.int32)
        A.check(self._lib.fs_batch_get_status(self._h, _iptr(out)), "get_status")
        return out

    def history_arrays(self, first=0, n=None):
        """depth, flow [n, B, N] (needs history=True)."""
        n = self._span(first, n)
        h = np.empty((n, self.B, self.N)); Q = np.empty((n, self.B, self.N))
        A.check(self._lib.fs_batch_get_history(self._h, first, n, _dptr(h), _dptr(Q)), "get_history")
        return h, Q

    def storage_stage(self):
        out = np.empty(self.B)
        A.check(self._lib.fs_batch_get_storage_stage(self._h, _dptr(out)), "get_storage_stage")
        return out

    def residual_trace(self, first=0, n=None):
        """[n, TRACE_CAP, B] ||R|| per Newton iteration (needs trace=True); zeros beyond a level's count."""
        n = self._span(first, n)
        out = np.empty((n, A.TRACE_CAP, self.B))
        A.check(self._lib.fs_batch_get_residual_trace(self._h, first, n, _dptr(out)), "get_residual_trace")
        return out

    def storage_stages(self, first=0, n=None):
        """[n, B] reservoir stage per time level (storage boundary only)."""
        n = self._span(first, n)
        out = np.empty((n, self.B))
        A.check(self._lib.fs_batch_get_storage_stages(self._h, first, n, _dptr(out)), "get_storage_stages")
        return out

    DERIVED = ("level", "area", "top_width", "froude_number", "velocity", "wave_celerity", "amplitude")

    def derive(self, first=0, n=None, fields=None):
        """Solver.prepare_results on the device (needs history=True): dict name -> [n, B, N] plus
        peak_amplitude [B, N]."""
        n = self._span(first, n)
        want = set(self.DERIVED + ("peak_amplitude",)) if fields is None else set(fields)
        out = {k: np.empty((n, self.B, self.N)) for k in self.DERIVED if k in want}
        if "peak_amplitude" in want:
            out["peak_amplitude"] = np.empty((self.B, self.N))
        ptr = lambda k: _opt(out.get(k))
        A.check(self._lib.fs_batch_derive(self._h, first, n, *[ptr(k) for k in self.DERIVED], ptr("peak_amplitude")),
                "derive")
        return out

    # -- ensemble post-processing on the device (the hydrograph block is reduced where it is) ----
    def summaries(self, first=0, n=None):
        """The numbers of the reference's result summary (solver.py:203-229) for every reach over the levels [first, first + n):
        dict name -> [B] with the names of _abi.SUM_ROWS.  Level indices are relative to `first` (multiply by the reach's dt); a
        failed reach is summarised over the rows before its failing level, `levels` says how many."""
        n = self._span(first, n)
        out = np.empty((len(A.SUM_ROWS), self.B))
        A.check(self._lib.fs_batch_summarize(self._h, int(first), int(n), _dptr(out)), "summarize")
        return {k: out[i] for i, k in enumerate(A.SUM_ROWS)}

    def lookup(self, x_row, y_row, xq, y_offset=None, target=None, first=0, n=None):
        """np.interp(xq, x_series, y_series + y_offset) for every reach (rows: _abi.ROW_*), dict(values [n_q, B], rmse [B] against
        `target` or None, monotone [B]: False where x descends somewhere in the range - np.interp is not defined there, and the
        values of that reach are those of a plain bisection)."""
        n = self._span(first, n)
        xq = np.ascontiguousarray(xq, dtype=np.float64).reshape(-1)
        off = P.opt_per_reach(y_offset, self.B)
        tgt = None if target is None else np.ascontiguousarray(target, dtype=np.float64).reshape(-1)
        assert tgt is None or tgt.shape == xq.shape
        values = np.empty((len(xq), self.B))
        rmse = None if tgt is None else np.empty(self.B)
        info = np.empty(self.B, dtype=np.int32)
        A.check(self._lib.fs_batch_lookup(self._h, int(first), int(n), int(x_row), int(y_row), _opt(off), _dptr(xq), len(xq), _opt(tgt),
                                          _dptr(values), _opt(rmse), _iptr(info)), "lookup")
        return dict(values=values, rmse=rmse, monotone=(info & 1) == 0)

    def bands(self, quantiles=(0.05, 0.5, 0.95), first=0, n=None):
        """Across the members, per level and signal: dict(min, max, mean, std [n, 4], quantiles [n, 4, n_q]: exact order
        statistics, numpy's default method; n_members [n]).  Failed members are left out."""
        n = self._span(first, n)
        q = np.ascontiguousarray(quantiles, dtype=np.float64).reshape(-1)
        mom = np.empty((n, 4, 4))
        qu = np.empty((n, 4, len(q)))
        cnt = np.empty(n, dtype=np.int32)
        A.check(self._lib.fs_batch_bands(self._h, int(first), int(n), _opt(q if len(q) else None), len(q), _dptr(mom),
                                         _opt(qu if len(q) else None), _iptr(cnt)), "bands")
        return dict(min=mom[:, :, 0], max=mom[:, :, 1], mean=mom[:, :, 2], std=mom[:, :, 3], quantiles=qu, n_members=cnt)

    # -- flood envelopes along the reach (the stored history is reduced where it is) ----------------
    def envelope(self, quantities=("stage",), threshold=None, threshold_quantity="stage", first=0, n=None):
        """Per (reach, node) over the levels [first, first + n) of the stored history (needs history=True): dict name -> dict(max,
        max_level, min, min_level) of [B, N] for the names of _abi.ENV_QUANTITIES given, plus levels [B] (the rows of each reach that
        entered: a failed reach enters with the rows before its failing level) and crossing = dict(first, last, count) of [B, N] or
        None.  Levels are relative to `first` and are first indices, as np.argmax / np.argmin.  threshold: scalar, [N] or [B, N],
        held against `threshold_quantity` (typically stage against the bank or levee crest): the first and last level at or above
        it (-1: never) and their number; NaN entries are not assessed.  The envelope stays on the device for profile_bands."""
        n = self._span(first, n)
        mask, names = P.envelope_mask(quantities)
        thr, per_reach = P.envelope_threshold(threshold, self.B, self.N)
        out = np.empty((len(names), len(A.ENV_STATS), self.B, self.N))
        cross = None if thr is None else np.empty((len(A.ENV_CROSS_ROWS), self.B, self.N))
        levels = np.empty(self.B, dtype=np.int32)
        self._envelope = ((), False)
        A.check(self._lib.fs_batch_envelope(self._h, int(first), int(n), mask, _opt(thr), per_reach, P.envelope_quantity(threshold_quantity),
                                            _dptr(out), _opt(cross), _iptr(levels)), "envelope")
        self._envelope = (names, thr is not None)
        res = {name: dict(zip(A.ENV_STATS, out[i])) for i, name in enumerate(names)}
        res["levels"] = levels
        res["crossing"] = None if cross is None else dict(zip(A.ENV_CROSS_ROWS, cross))
        return res

    def envelope_device(self, quantities=("stage",), threshold=None, threshold_quantity="stage", first=0, n=None):
        """envelope() with the results left on the device; returns {(name, stat): device pointer to [B, N] float64}, the crossing rows
        under ("crossing", "first" | "last" | "count")."""
        n = self._span(first, n)
        mask, names = P.envelope_mask(quantities)
        thr, per_reach = P.envelope_threshold(threshold, self.B, self.N)
        self._envelope = ((), False)
        A.check(self._lib.fs_batch_envelope_device(self._h, int(first), int(n), mask, _opt(thr), per_reach,
                                                   P.envelope_quantity(threshold_quantity)), "envelope_device")
        self._envelope = (names, thr is not None)
        keys = [(name, stat) for name in names for stat in A.ENV_STATS] + ([("crossing", c) for c in A.ENV_CROSS_ROWS] if thr is not None else [])
        return {k: self._lib.fs_batch_envelope_device_ptr(self._h, i) for i, k in enumerate(keys)}

    def profile_bands(self, quantity, stat="max", quantiles=(0.05, 0.5, 0.95)):
        """Across the members, per node, of one row of the envelope this batch holds (envelope() comes first): dict(min, max, mean,
        std [N], quantiles [N, n_q]: exact order statistics, numpy's default method; exceed [N]: the fraction of the entering members
        that reached the threshold at the node, or None for an envelope without a threshold; n_members [N]).  quantity: a name the
        envelope was computed for with stat of _abi.ENV_STATS, or "crossing" with stat "first" | "last" | "count".  Failed members,
        members without rows and, at a node, members of a ragged batch that do not have it are left out."""
        names, crossings = self._envelope
        if not names:
            raise ValueError("this batch holds no envelope: call envelope() first")
        qbit, row = P.envelope_row(quantity, stat, names, crossings)
        q = P.quantile_levels(quantiles)
        mom = np.empty((self.N, 4))
        qu = np.empty((self.N, len(q)))
        exceed = np.empty(self.N) if crossings else None
        cnt = np.empty(self.N, dtype=np.int32)
        A.check(self._lib.fs_batch_profile_bands(self._h, qbit, row, _opt(q if len(q) else None), len(q), _dptr(mom),
                                                 _opt(qu if len(q) else None), _opt(exceed), _iptr(cnt)), "profile_bands")
        return dict(min=mom[:, 0], max=mom[:, 1], mean=mom[:, 2], std=mom[:, 3], quantiles=qu, exceed=exceed, n_members=cnt)

    # -- reach storage and the discrete water balance (reduced along the reach, where the state is) --------
    def reach_integrals(self, first=0, n=None, threshold=None, current=False):
        """Per (level, reach): the trapezoid-rule volume [m^3] and water surface [m^2] of the node areas and top widths, and the
        length [m] of reach whose stage is at or above `threshold` (scalar, [N] or [B, N]; NaN entries are not assessed; None: the
        row is NaN).  Fills the rows [first, first + n) of the batch's integral block from the stored history (needs history=True)
        and returns dict name -> [n, B] with the names of _abi.INT_ROWS ('balance' is NaN until water_balance()).  current=True
        evaluates the current state into the row of the current level instead - no history needed, no wait for the device: a batch
        without history is marked now and then between two step(..., sync=False) calls - and returns None."""
        first, n = P.integral_range(first, n, self.level, current)
        thr, per_reach = P.envelope_threshold(threshold, self.B, self.N)
        A.check(self._lib.fs_batch_reach_integrals(self._h, first, n, _opt(thr), per_reach), "reach_integrals")
        return None if current else self.integral_rows(first, n)

    def integral_rows(self, first=0, n=None):
        """the rows [first, first + n) of the integral block as they stand: dict name -> [n, B]; NaN where never evaluated"""
        n = self._span(first, n)
        out = np.empty((n, len(A.INT_ROWS), self.B))
        A.check(self._lib.fs_batch_get_reach_integrals(self._h, int(first), int(n), _dptr(out)), "get_reach_integrals")
        return {k: out[:, i] for i, k in enumerate(A.INT_ROWS)}

    def water_balance(self, first=0, n=None):
        """The discrete water balance over the levels [first, first + n), from each evaluated row of the integral block to the next
        (a span): storage change minus the net inflow volume of the Preissmann continuity row, which the scheme closes to its Newton
        tolerance.  Returns (rows, totals): rows as integral_rows() with 'balance' filled at every span's end level (0 at the first
        evaluated row), totals dict name -> [B] with the names of _abi.BAL_ROWS (levels relative to `first`)."""
        n = self._span(first, n)
        tot = np.empty((len(A.BAL_ROWS), self.B))
        A.check(self._lib.fs_batch_water_balance(self._h, int(first), int(n), _dptr(tot)), "water_balance")
        return self.integral_rows(first, n), {k: tot[i] for i, k in enumerate(A.BAL_ROWS)}

    def integral_bands(self, quantiles=(0.05, 0.5, 0.95), first=0, n=None):
        """bands() on the integral block: across the members, per level and row of _abi.INT_ROWS, dict(min, max, mean, std [n, 4],
        quantiles [n, 4, n_q], n_members [n]).  Failed members are left out; a level that a remaining member has not evaluated
        is NaN."""
        n = self._span(first, n)
        q = P.quantile_levels(quantiles)
        mom = np.empty((n, 4, 4))
        qu = np.empty((n, 4, len(q)))
        cnt = np.empty(n, dtype=np.int32)
        A.check(self._lib.fs_batch_integral_bands(self._h, int(first), int(n), _opt(q if len(q) else None), len(q), _dptr(mom),
                                                  _opt(qu if len(q) else None), _iptr(cnt)), "integral_bands")
        return dict(min=mom[:, :, 0], max=mom[:, :, 1], mean=mom[:, :, 2], std=mom[:, :, 3], quantiles=qu, n_members=cnt)

    def reach_integrals_device_ptr(self):
        """device pointer to the integral block [max_levels, 4, B] float64 (None before the first evaluation)"""
        return self._lib.fs_batch_reach_integrals_device_ptr(self._h)

    # -- interior gauges: station series, their bands across the members and fit scores ---------------------
    def set_gauges(self, chainage=None, node=None, weight=None, dx=None, nodes=None):
        """Gauges inside the reach, each between node and node + 1 at weight in [0, 1) of the way: node, weight [G] shared by the
        batch or [B, G] per reach; or chainage [G] / [B, G], distances from the upstream end, with dx (scalar or [B]: the node
        spacing) and nodes (scalar or [B]: the reaches' own node counts; None: N) through _pack.gauge_positions.  Allocates the batch's gauge block [G, L, 4, B] on the device, every row NaN; no gauges
        (empty arrays) frees it.  Returns (node, weight) as set."""
        if chainage is not None:
            if node is not None or weight is not None or dx is None:
                raise ValueError("set_gauges: chainage comes with dx, and without node and weight")
            node, weight = P.gauge_positions(chainage, dx, self.N if nodes is None else nodes)
        elif node is None or weight is None:
            raise ValueError("set_gauges: give chainage and dx, or node and weight")
        node, weight, per_reach = P.gauge_arrays(node, weight, self.B)
        A.check(self._lib.fs_batch_set_gauges(self._h, int(node.shape[-1]), _iptr(node), _dptr(weight), per_reach), "set_gauges")
        self.gauge_positions = (node, weight)
        return node, weight

    def gauges(self, first=0, n=None, current=False):
        """Fills the rows [first, first + n) of every gauge from the stored history (needs history=True): per (level, member) depth,
        flow, stage and velocity at the gauge, evaluated at its two nodes as derive() evaluates them and interpolated in float64.
        current=True fills the row of the current level from the current state instead - no history needed, no wait for the device:
        a batch without history is marked between two step(..., sync=False) calls.  Returns None; gauge_rows() downloads."""
        first, n = P.integral_range(first, n, self.level, current)
        A.check(self._lib.fs_batch_gauges(self._h, first, n), "gauges")

    def gauge_rows(self, g, first=0, n=None):
        """the rows [first, first + n) of gauge g as they stand: [n, 4, B] in the order of _abi.GAUGE_ROWS; NaN where never evaluated,
        from a failed member's failing level on, and for a member whose reach does not have the gauge"""
        n = self._span(first, n)
        out = np.empty((n, len(A.GAUGE_ROWS), self.B))
        A.check(self._lib.fs_batch_get_gauges(self._h, int(g), int(first), int(n), _dptr(out)), "get_gauges")
        return out

    def gauge_bands(self, g, quantiles=(0.05, 0.5, 0.95), first=0, n=None):
        """bands() on gauge g's block: across the members, per level and row of _abi.GAUGE_ROWS, dict(min, max, mean, std [n, 4],
        quantiles [n, 4, n_q], n_members [n]).  Failed members and members without the gauge are left out; a level that a remaining
        member has not evaluated is NaN."""
        n = self._span(first, n)
        q = P.quantile_levels(quantiles)
        mom = np.empty((n, 4, 4))
        qu = np.empty((n, 4, len(q)))
        cnt = np.empty(n, dtype=np.int32)
        A.check(self._lib.fs_batch_gauge_bands(self._h, int(g), int(first), int(n), _opt(q if len(q) else None), len(q), _dptr(mom),
                                               _opt(qu if len(q) else None), _iptr(cnt)), "gauge_bands")
        return dict(min=mom[:, :, 0], max=mom[:, :, 1], mean=mom[:, :, 2], std=mom[:, :, 3], quantiles=qu, n_members=cnt)

    def gauge_lookup(self, g, x_row, y_row, xq, y_offset=None, target=None, first=0, n=None):
        """lookup() on gauge g's block: np.interp(xq, x_series, y_series + y_offset) for every member, the rows being names or
        indices of _abi.GAUGE_ROWS (a rating at the gauge: x_row="flow", y_row="stage").  Every level of the range must have been
        evaluated.  dict(values [n_q, B], rmse [B] or None, monotone [B])."""
        n = self._span(first, n)
        xq = np.ascontiguousarray(xq, dtype=np.float64).reshape(-1)
        off = P.opt_per_reach(y_offset, self.B)
        tgt = None if target is None else np.ascontiguousarray(target, dtype=np.float64).reshape(-1)
        if tgt is not None and tgt.shape != xq.shape:
            raise ValueError("gauge_lookup: target must have the shape of xq")
        values = np.empty((len(xq), self.B))
        rmse = None if tgt is None else np.empty(self.B)
        info = np.empty(self.B, dtype=np.int32)
        A.check(self._lib.fs_batch_gauge_lookup(self._h, int(g), int(first), int(n), P.gauge_row(x_row), P.gauge_row(y_row), _opt(off),
                                                _dptr(xq), len(xq), _opt(tgt), _dptr(values), _opt(rmse), _iptr(info)), "gauge_lookup")
        return dict(values=values, rmse=rmse, monotone=(info & 1) == 0)

    def gauge_score(self, g, signal, observed, first=0, n=None):
        """The fit of every member to a record at gauge g: `signal` (a name or index of _abi.GAUGE_ROWS) over the levels
        [first, first + n) against observed [n] (shared) or [n, B]; NaN: no observation at that level.  dict name -> [B] with the
        names of _abi.GS_ROWS: count of the levels that entered (inside the member's completed rows, evaluated, observed), bias,
        rmse, nse (Nash-Sutcliffe), the simulated peak and its level (relative to `first`), peak error and peak lag in levels."""
        n = self._span(first, n)
        obs, per_reach = P.gauge_observed(observed, n, self.B)
        out = np.empty((len(A.GS_ROWS), self.B))
        A.check(self._lib.fs_batch_gauge_score(self._h, int(g), P.gauge_row(signal), int(first), int(n), _dptr(obs), per_reach, _dptr(out)),
                "gauge_score")
        return {k: out[i] for i, k in enumerate(A.GS_ROWS)}

    def gauges_device_ptr(self, g):
        """device pointer to gauge g's block [max_levels, 4, B] float64 (None: no such gauge)"""
        return self._lib.fs_batch_gauges_device_ptr(self._h, int(g))

    # -- assimilation of gauge observations: the analysis step of an ensemble Kalman filter -------------------
    def assimilate(self, observations, perturbations=None, taper=None, depth_floor=1e-3):
        """Corrects the state (and the Newton start vector) of every active member from observations of gauge signals of the
        current state, between two step() calls: observations is a sequence of assimilation.Observation or (gauge, signal, value,
        variance) tuples, perturbations [n_obs, B] what is added to each observation per member (None: zeros; the library draws no
        random numbers - assimilation.perturbations does), taper [N] or [n_obs, N] in [0, 1] the localisation along the reach
        (None: ones).  A member is active when it holds every observed gauge at the current level; failed members are not, and are
        not written.  Returns dict(n_active, prior: dict(mean_h, var_h, mean_Q, var_Q [N]) of the active members before the
        update, cross_cov [2, n_obs, N]: cov(h or Q at a node, observation), clamped [B]: nodes whose new depth was raised to
        depth_floor).  History, hydrographs, level and status stay what they were: they record the forecast."""
        m, gauge, signal, value, variance, pert, tap, floor = P.pack_observations(observations, self.B, self.N, perturbations, taper, depth_floor)
        prior, cross = np.empty((4, self.N)), np.empty((2, m, self.N))
        clamped, n_active = np.zeros(self.B, dtype=np.int32), C.c_int32(0)
        A.check(self._lib.fs_batch_assimilate(self._h, m, _iptr(gauge), _iptr(signal), _dptr(value), _dptr(variance), _opt(pert), _opt(tap), floor,
                                              _dptr(prior), _dptr(cross), _iptr(clamped), C.byref(n_active)), "assimilate")
        return dict(n_active=int(n_active.value), prior=dict(mean_h=prior[0], var_h=prior[1], mean_Q=prior[2], var_Q=prior[3]), cross_cov=cross,
                    clamped=clamped)

    def last_step_ms(self):
        return self._lib.fs_batch_last_step_ms(self._h)

    def kernel_info(self):
        v = [C.c_int32() for _ in range(4)]
        A.check(self._lib.fs_batch_kernel_info(self._h, *[C.byref(x) for x in v]), "kernel_info")
        return dict(cells_per_thread=v[0].value, waves_per_reach=v[1].value, lds_bytes=v[2].value, vgprs=v[3].value)

    def poly_tables(self):
        """polyline batches: 1 = stage tables, 0 = edge walk (tables beyond FS_POLY_TABLE_MAX_BYTES or FS_POLY_WALK=1), -1 = none set"""
        return self._lib.fs_batch_poly_tables(self._h)

    def kernel_index(self):
        """index into _abi.kernel_table() of the instantiation the last step / iterate launched"""
        return self._lib.fs_batch_kernel_index(self._h)

    def derive_device(self, first=0, n=None, fields=A.DERIVE_ALL):
        """prepare_results with the results left on the device; returns {name: device pointer}."""
        n = self._span(first, n)
        A.check(self._lib.fs_batch_derive_device(self._h, first, n, int(fields)), "derive_device")
        names = self.DERIVED + ("peak_amplitude",)
        return {k: self._lib.fs_batch_derived_device_ptr(self._h, i) for i, k in enumerate(names) if fields & (1 << i)}

    def hydrograph_device_ptr(self):
        return self._lib.fs_batch_hydrograph_device_ptr(self._h)
