"""Python values -> the flat arrays the C ABI receives (include/flowsim_abi.h), without the library: numpy and the constants of _abi
only, no arithmetic - but for member_sections, the member transform of a geometry ensemble written out in numpy (its definition, and
the host path the device kernels replace).  Every function returns C-contiguous arrays of the dtype and shape the call takes; batch.py passes them on.
tests/test_batch_pack.py holds them on the CPU to the arrays the setters built before these functions existed, and to what
fs::check_bc / fs::check_bc_per_reach accept; tests/test_envelope_pack.py holds the envelope arguments."""
import numpy as np

from . import _abi as A

_KIND_PARAMS = {
    A.BC_FLOW_HYDROGRAPH: (), A.BC_STAGE_HYDROGRAPH: ("bed_level",), A.BC_FIXED_DEPTH: ("initial_depth",),
    A.BC_NORMAL_DEPTH: ("bed_slope", "bed_level"), A.BC_RATING_POWER: ("a", "b", "stage_shift", "bed_level"),
    A.BC_RATING_POLY: ("a", "b", "c", "stage_shift", "bed_level"),
    A.BC_RATING_BLEND: ("stage0", "buffer", "lo0", "lo1", "lo2", "hi0", "hi1", "hi2", "dY", "bed_level"),
    A.BC_STORAGE: ("surface_area", "min_stage", "Y_min", "Y_max", "bed_level"),
}


# -- scalar or array -> one value per reach / per node --------------------------------------------
def per_reach(v, B, dtype=np.float64):
    """scalar or [B] -> [B]"""
    return np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dtype), (B,)))


def opt_per_reach(v, B, dtype=np.float64):
    return None if v is None else per_reach(v, B, dtype)


def per_node(v, B, N):
    """scalar, [N] or [B, N] -> [B, N]"""
    return np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (B, N)))


def bed_slope(v, B, N):
    """(None | [N] | [B, N], per_reach) of init_state; None entries are the reference's undefined slope: NaN, which the library
    refuses as the reference does"""
    if v is None:
        return None, 0
    v = np.ascontiguousarray(np.array(v, dtype=np.float64))
    assert v.shape in ((N,), (B, N))
    return v, int(v.ndim == 2)


# -- geometry -------------------------------------------------------------------------------------
def n_override(v, B):
    if v is None:
        return None
    v = np.ascontiguousarray(v, dtype=np.float64)
    assert v.shape == (B,)
    return v


def uniform_params(trap, B, width, manning, z_us, z_ds, side_slope=None):
    """[RU_NPARAM | TU_NPARAM, B]"""
    p = np.empty((A.TU_NPARAM if trap else A.RU_NPARAM, B), dtype=np.float64)
    p[A.RU_WIDTH], p[A.RU_MANNING], p[A.RU_Z_US], p[A.RU_Z_DS] = width, manning, z_us, z_ds
    if trap:
        p[A.TU_SIDE_SLOPE] = 0.0 if side_slope is None else side_slope
    return p


def geometry_table(geo, B, N, per_reach):
    """[GEO_NPARAM, N], or with per_reach [B, GEO_NPARAM, N] (rows given as [N] are shared by the reaches)"""
    tab = np.empty(((B,) if per_reach else ()) + (A.GEO_NPARAM, N), dtype=np.float64)
    for i, k in enumerate(A.GEO_ROWS):
        tab[..., i, :] = np.asarray(geo[k], dtype=np.float64)
    return tab


def irregular_arrays(geo, B, N):
    """(table, n_pts int32, x, z, limits, per_reach); one channel per reach where irr_npts is [B, N]"""
    per_reach = np.ndim(geo["irr_npts"]) == 2
    lead = (B,) if per_reach else ()
    cnt = np.ascontiguousarray(geo["irr_npts"], dtype=np.int32)
    x = np.ascontiguousarray(geo["irr_x"], dtype=np.float64)
    z = np.ascontiguousarray(geo["irr_z"], dtype=np.float64)
    lim = np.ascontiguousarray(geo["irr_limits"], dtype=np.float64)
    assert cnt.shape == lead + (N,) and x.shape == z.shape and x.shape[:-1] == lead + (N,) and lim.shape == lead + (N, 2)
    return geometry_table(geo, B, N, per_reach), cnt, x, z, lim, per_reach


def member_shift(v, B, N):
    """a dz_* of the member transform: None, or [B] (the same shift at every node) / [B, N] -> [B, N]"""
    if v is None:
        return None
    v = np.asarray(v, dtype=np.float64)
    if v.shape not in ((B,), (B, N)):
        raise ValueError("dz_left, dz_main and dz_right must be [B] or [B, N]")
    return np.ascontiguousarray(np.broadcast_to(v[:, None] if v.ndim == 1 else v, (B, N)))


def member_n_scale(v, B):
    """n_scale of the member transform: None or [3, B] (left, main, right)"""
    if v is None:
        return None
    v = np.ascontiguousarray(v, dtype=np.float64)
    if v.shape != (3, B):
        raise ValueError("n_scale must be [3, B]: the factors of n_left, n_main, n_right")
    return v


def member_arrays(geo, B, N, dz_left=None, dz_main=None, dz_right=None, n_scale=None):
    """(table, n_pts int32, x, z, limits, dz_left, dz_main, dz_right, n_scale) of fs_batch_set_geometry_irregular_members: ONE
    channel as irregular_arrays packs it, the transforms [B, N] / [3, B] or None"""
    tab, cnt, x, z, lim, per_reach = irregular_arrays(geo, B, N)
    if per_reach:
        raise ValueError("a geometry ensemble takes ONE channel: irr_npts [N], irr_x / irr_z [N, P]")
    return (tab, cnt, x, z, lim) + tuple(member_shift(v, B, N) for v in (dz_left, dz_main, dz_right)) + (member_n_scale(n_scale, B),)


def member_sections(geo, B, dz_left=None, dz_main=None, dz_right=None, n_scale=None):
    """THE DEFINITION of the member transform (include/flowsim_abi.h: fs_batch_set_geometry_irregular_members), in numpy: the
    per-reach geo dict set_geometry_irregular accepts (irr_z [B, N, P], z_bed [B, N], n_* [B, N], ...) of the B members of one
    polyline channel.  Vertex j of node i is in the left strip where x_j < left limit, in the right one where x_j > right limit, in
    the main channel otherwise; z'_j = z_j + dz_strip(j)[r, i]; n' = n * n_scale[0..2][r]; z_bed' = min_j z'_j; slots beyond a node's
    count repeat its transformed last vertex.  The device builds the same, bit for bit; this is also the host path it replaces."""
    cnt = np.asarray(geo["irr_npts"], dtype=np.int32)
    N = len(cnt)
    x, z, lim = (np.asarray(geo[k], dtype=np.float64) for k in ("irr_x", "irr_z", "irr_limits"))
    P = x.shape[1]
    dzl, dzm, dzr = (np.zeros((B, N)) if v is None else member_shift(v, B, N) for v in (dz_left, dz_main, dz_right))
    ns = np.ones((3, B)) if n_scale is None else member_n_scale(n_scale, B)
    slot = np.minimum(np.arange(P)[None, :], cnt[:, None] - 1)               # [N, P]: padding slots read the last vertex
    xs, zs = np.take_along_axis(x, slot, 1), np.take_along_axis(z, slot, 1)
    left, right = xs < lim[:, :1], xs > lim[:, 1:]
    dz = np.where(left[None], dzl[:, :, None], np.where(right[None], dzr[:, :, None], dzm[:, :, None]))
    out = {k: np.ascontiguousarray(np.broadcast_to(np.asarray(geo[k], dtype=np.float64), (B, N))) for k in A.GEO_ROWS}
    out["irr_z"] = zs[None] + dz
    out["irr_x"] = np.ascontiguousarray(np.broadcast_to(xs, (B, N, P)))
    out["irr_npts"] = np.ascontiguousarray(np.broadcast_to(cnt, (B, N)))
    out["irr_limits"] = np.ascontiguousarray(np.broadcast_to(lim, (B, N, 2)))
    out["z_bed"] = out["irr_z"].min(axis=2)
    for row, k in enumerate(("n_left", "n_main", "n_right")):
        out[k] = np.asarray(geo[k], dtype=np.float64)[None, :] * ns[row][:, None]
    return out


# -- boundaries -----------------------------------------------------------------------------------
def storage_curve_rows(out, params, stages, areas):
    """FS_BC_STORAGE_CURVE into out [rows] (one reservoir) or [rows, B]: the FS_SC_* scalars (alpha 1 when absent, the others 0 when
    absent or None, n_curve from the curve), then stages [n_curve(, B)], then areas; rows beyond those are left as they are"""
    nf, nc = len(A.SC_NAMES), len(stages)
    sc = {"alpha": 1.0, **params, "n_curve": float(nc)}
    for i, k in enumerate(A.SC_NAMES):
        v = sc.get(k)
        out[i] = 0.0 if v is None else v
    out[nf:nf + nc] = stages
    out[nf + nc:nf + 2 * nc] = areas


def _curve(params):
    return np.asarray(params.get("curve", np.empty((0, 2))), dtype=np.float64)


def bc_params(spec, B):
    """(params | None, n_params, per_reach) of fs_batch_set_bc; KeyError for a kind without a device form"""
    if spec.kind == A.BC_HOST_ROW:          # evaluated by the caller before every Newton iteration (set_host_rows / iterate)
        return None, 3, 1
    if spec.kind == A.BC_STORAGE_CURVE:
        # one reservoir per reach where a scalar is [B] or the curve [B, n_curve, 2] (the others shared), else one for the batch
        curve = _curve(spec.params)
        per = curve.ndim == 3 or any(np.ndim(v) > 0 for k, v in spec.params.items() if k != "curve")
        if per:
            curve = np.broadcast_to(curve.reshape((-1,) + curve.shape[-2:]) if curve.size else np.empty((1, 0, 2)), (B,) + curve.shape[-2:])
        else:
            curve = curve.reshape(-1, 2)
        p = np.empty((len(A.SC_NAMES) + 2 * curve.shape[-2],) + ((B,) if per else ()), dtype=np.float64)
        storage_curve_rows(p, spec.params, curve[..., 0].T, curve[..., 1].T)
        return p, p.shape[0], int(per)
    names = _KIND_PARAMS[spec.kind]
    vals = [np.asarray(spec.params[n], dtype=np.float64) for n in names]
    per = any(v.ndim > 0 for v in vals)
    p = np.empty((len(names),) + ((B,) if per else ()), dtype=np.float64)
    for i, v in enumerate(vals):
        p[i] = v
    return (p if names else None), len(names), int(per)


def bc_params_per_reach(specs, B):
    """(kinds int32 [B], params [rows, B], rows) of fs_batch_set_bc_per_reach_wide; a kind without a device form gets zeros (the
    library refuses it)"""
    assert len(specs) == B
    kinds = np.array([s.kind for s in specs], dtype=np.int32)
    curves = {r: _curve(s.params).reshape(-1, 2) for r, s in enumerate(specs) if s.kind == A.BC_STORAGE_CURVE}
    rows = max([A.BC_MAX_PARAMS] + [len(A.SC_NAMES) + 2 * len(c) for c in curves.values()])
    p = np.zeros((rows, B), dtype=np.float64)
    for r, s in enumerate(specs):
        if r in curves:
            storage_curve_rows(p[:, r], s.params, curves[r][:, 0], curves[r][:, 1])
        else:
            for i, name in enumerate(_KIND_PARAMS.get(s.kind, ())):
                p[i, r] = float(s.params[name])
    return kinds, p, rows


def _pad_levels(out, t):
    """the first min(L, n) rows of t [n, ...] into out [L, ...], the last of them repeated below"""
    n = min(len(out), len(t))
    out[:n] = t[:n]
    out[n:] = t[n - 1]


def bc_target(target, L, B):
    """[n] (shared) or [n, B] -> [L, B]; None stays None"""
    if target is None:
        return None
    t = np.asarray(target, dtype=np.float64)
    tgt = np.empty((L, B), dtype=np.float64)
    _pad_levels(tgt, t[:, None] if t.ndim == 1 else t)
    return tgt


def bc_target_per_reach(targets, L, B):
    """one optional [n_r] per reach -> [L, B] (zeros for a reach without one); None where no reach has one"""
    if all(t is None for t in targets):
        return None
    tgt = np.zeros((L, B), dtype=np.float64)
    for r, t in enumerate(targets):
        if t is not None:
            _pad_levels(tgt[:, r], np.asarray(t, dtype=np.float64).reshape(-1))
    return tgt


def host_rows(dh, dq, res, B):
    """[3, B]: d/dh, d/dQ, residual"""
    rows = np.empty((3, B), dtype=np.float64)
    rows[0], rows[1], rows[2] = dh, dq, res
    return rows


# -- forcing built on the device ------------------------------------------------------------------
def sample_tables(times, values):
    """(times [K], values [n_tables, K]) of fs_batch_set_bc_sampled; values [K] is one table.  ValueError where the library would
    refuse: no point, times not increasing, lengths that differ"""
    t = np.ascontiguousarray(times, dtype=np.float64).reshape(-1)
    v = np.ascontiguousarray(values, dtype=np.float64)
    v = v.reshape(1, -1) if v.ndim == 1 else v
    if t.size < 1 or v.ndim != 2 or v.shape[0] < 1 or v.shape[1] != t.size:
        raise ValueError("values must be [K] or [n_tables, K] for times [K], K >= 1")
    if np.any(np.isnan(t)) or np.any(np.diff(t) <= 0):
        raise ValueError("times must be increasing")
    return t, v


def table_index(table_of, n_tables, B):
    """None or int32 [B] in 0 .. n_tables - 1"""
    if table_of is None:
        return None
    idx = per_reach(table_of, B, np.int32)
    if np.any(idx < 0) or np.any(idx >= n_tables):
        raise ValueError("table_of must be 0 .. n_tables - 1")
    return idx


def pool_descriptor(curve_stage, curve_volume, weirs):
    """(curve_stage [K], curve_volume [K], weirs [n_w, 4] = C, crest, ramp_top, 0) of fs_batch_route_pool; weirs: rows of
    (C, crest) or (C, crest, ramp_top) - no ramp_top is the crest itself: no ramp"""
    z = np.ascontiguousarray(curve_stage, dtype=np.float64).reshape(-1)
    v = np.ascontiguousarray(curve_volume, dtype=np.float64).reshape(-1)
    if z.shape != v.shape:
        raise ValueError("curve_stage and curve_volume must have the same length")
    if not 2 <= z.size <= A.POOL_MAX_CURVE:
        raise ValueError(f"the volume curve takes 2 .. {A.POOL_MAX_CURVE} points")
    if np.any(np.diff(z) <= 0):
        raise ValueError("curve stages must be increasing")
    if len(weirs) > A.POOL_MAX_WEIRS:
        raise ValueError(f"at most {A.POOL_MAX_WEIRS} weirs")
    w = np.zeros((len(weirs), 4), dtype=np.float64)
    for i, row in enumerate(weirs):
        row = tuple(float(x) for x in row)
        if len(row) not in (2, 3):
            raise ValueError("a weir is (C, crest) or (C, crest, ramp_top)")
        w[i, 0], w[i, 1] = row[0], row[1]
        w[i, 2] = row[2] if len(row) == 3 else row[1]
    return z, v, w


def weir_scale(v, n_w, B):
    """None or [n_w, B] (a [n_w] column is shared by the members)"""
    if v is None:
        return None
    v = np.asarray(v, dtype=np.float64)
    if v.shape not in ((n_w,), (n_w, B)):
        raise ValueError("weir_scale must be [n_weirs] or [n_weirs, B]")
    return np.ascontiguousarray(np.broadcast_to(v[:, None] if v.ndim == 1 else v, (n_w, B)))


# -- flood envelopes ------------------------------------------------------------------------------
def envelope_quantity(name):
    """the FS_ENV_* bit of one quantity name of _abi.ENV_QUANTITIES"""
    if name not in A.ENV_QUANTITIES:
        raise ValueError(f"unknown envelope quantity {name!r}: one of {', '.join(A.ENV_QUANTITIES)}")
    return 1 << A.ENV_QUANTITIES.index(name)


def envelope_mask(quantities):
    """(FS_ENV_* mask, names in bit order - the order of the rows fs_batch_envelope writes); a single name may be given as a str"""
    names = (quantities,) if isinstance(quantities, str) else tuple(quantities)
    if not names:
        raise ValueError("no envelope quantity given")
    mask = 0
    for name in names:
        bit = envelope_quantity(name)
        if mask & bit:
            raise ValueError(f"envelope quantity {name!r} given twice")
        mask |= bit
    return mask, tuple(n for n in A.ENV_QUANTITIES if mask & envelope_quantity(n))


def envelope_threshold(threshold, B, N):
    """(None | [N] | [B, N] float64, per_reach) of fs_batch_envelope; a scalar is the same level at every node.  NaN entries stay: they
    mean "not assessed" """
    if threshold is None:
        return None, 0
    t = np.asarray(threshold, dtype=np.float64)
    if t.ndim == 0:
        t = np.full(N, float(t))
    if t.shape not in ((N,), (B, N)):
        raise ValueError(f"threshold must be a scalar, [N] = [{N}] or [B, N] = [{B}, {N}], not {list(t.shape)}")
    return np.ascontiguousarray(t), int(t.ndim == 2)


def envelope_row(quantity, stat, selected, crossings):
    """(quantity, stat) of fs_batch_profile_bands for a name pair: quantity one of `selected` (the names the envelope on the handle
    holds) with stat of _abi.ENV_STATS, or "crossing" with stat of _abi.ENV_CROSS_ROWS"""
    if quantity == "crossing":
        if not crossings:
            raise ValueError("the envelope was computed without a threshold: it has no crossing rows")
        if stat not in A.ENV_CROSS_ROWS:
            raise ValueError(f"unknown crossing row {stat!r}: one of {', '.join(A.ENV_CROSS_ROWS)}")
        return A.ENV_CROSSING, A.ENV_CROSS_ROWS.index(stat)
    bit = envelope_quantity(quantity)
    if quantity not in selected:
        raise ValueError(f"the envelope on this batch does not hold {quantity!r} (it holds: {', '.join(selected) or 'nothing'})")
    if stat not in A.ENV_STATS:
        raise ValueError(f"unknown envelope statistic {stat!r}: one of {', '.join(A.ENV_STATS)}")
    return bit, A.ENV_STATS.index(stat)


def quantile_levels(quantiles):
    """float64 [n_q], 0 <= n_q <= BANDS_MAX_Q, each in [0, 1]"""
    q = np.ascontiguousarray(quantiles, dtype=np.float64).reshape(-1)
    if len(q) > A.BANDS_MAX_Q:
        raise ValueError(f"at most {A.BANDS_MAX_Q} quantile levels")
    if np.any(~((q >= 0.0) & (q <= 1.0))):
        raise ValueError("quantile levels must be in [0, 1]")
    return q


# -- reach integrals and the water balance ---------------------------------------------------------
def integral_range(first, n, level, current):
    """(first, n) of fs_batch_reach_integrals: the levels [first, first + n) of the history (n None: up to `level`, the batch's
    current one), or (-1, 1) - the current state into the row of the current level - with current=True, which takes no range"""
    if current:
        if first != 0 or n is not None:
            raise ValueError("current=True evaluates the current state into the row of the current level: it takes no first / n")
        return -1, 1
    first = int(first)
    n = level - first + 1 if n is None else int(n)
    if first < 0 or n < 1:
        raise ValueError(f"levels [{first}, {first + n}) are no range of levels")
    return first, n


def balance_options(balance):
    """(every, threshold, quantiles) of the runners' balance= keyword: dict(every=1, threshold=None, quantiles=(0.05, 0.5, 0.95))"""
    unknown = set(balance) - {"every", "threshold", "quantiles"}
    if unknown:
        raise ValueError(f"balance: unknown keys {sorted(unknown)}")
    every = balance.get("every", 1)
    if isinstance(every, bool) or not isinstance(every, (int, np.integer)) or every < 1:
        raise ValueError(f"balance: every must be an integer >= 1, not {every!r}")
    return int(every), balance.get("threshold"), quantile_levels(balance.get("quantiles", (0.05, 0.5, 0.95)))


def balance_chunks(n_steps, every):
    """the step counts between two marks of a batch without history: `every` levels each, the last chunk what is left"""
    if n_steps < 0 or every < 1:
        raise ValueError("balance_chunks: n_steps >= 0 and every >= 1 required")
    return [every] * (n_steps // every) + ([n_steps % every] if n_steps % every else [])


# -- interior gauges -------------------------------------------------------------------------------
def gauge_positions(chainage, dx, nodes):
    """(node int32, weight float64) of fs_batch_set_gauges for gauges at the distances `chainage` from the upstream end: shared [G]
    when chainage is [G] and dx, nodes are scalars; per reach [B, G] when chainage is [B, G] or dx or nodes are [B] (chainage [G] is
    then every reach's).  x / dx within 4 eps max(1, x / dx) of an integer IS that node (weight 0.0); the end of the reach is
    (nodes - 1, 0.0); x outside [0, (nodes - 1) dx] raises."""
    x = np.asarray(chainage, dtype=np.float64)
    dx = np.asarray(dx, dtype=np.float64)
    nodes = np.asarray(nodes)
    if x.ndim not in (1, 2) or dx.ndim > 1 or nodes.ndim > 1:
        raise ValueError("gauge_positions: chainage is [G] or [B, G], dx and nodes are scalars or [B]")
    if nodes.dtype.kind not in "iu":
        raise ValueError("gauge_positions: nodes must be integers")
    if np.any(nodes < 2) or np.any(~(dx > 0.0)):
        raise ValueError("gauge_positions: nodes >= 2 and dx > 0 required")
    sizes = {a.shape[0] for a in (dx, nodes) if a.ndim == 1} | ({x.shape[0]} if x.ndim == 2 else set())
    if len(sizes) > 1:
        raise ValueError(f"gauge_positions: chainage, dx and nodes disagree on the number of reaches: {sorted(sizes)}")
    if sizes:
        B = sizes.pop()
        x = np.broadcast_to(x, (B, x.shape[-1]))
        dx, nodes = np.broadcast_to(dx, (B,))[:, None], np.broadcast_to(nodes, (B,))[:, None]
    if np.any(~np.isfinite(x)):
        raise ValueError("gauge_positions: chainage must be finite")
    last = (nodes - 1).astype(np.float64)
    outside = (x < 0.0) | (x > last * dx)
    if np.any(outside):
        raise ValueError(f"gauge_positions: chainage {x[outside].ravel()[0]!r} is outside the reach, [0, (nodes - 1) dx]")
    s = x / dx
    near = np.rint(s)
    s = np.where(np.abs(s - near) <= 4.0 * np.finfo(np.float64).eps * np.maximum(1.0, np.abs(s)), near, s)
    s = np.minimum(np.abs(s), last)              # (x = (nodes - 1) dx whose quotient rounds up a little is the last node; -0.0 is node 0)
    node = np.floor(s)
    weight = s - node
    return np.ascontiguousarray(node, dtype=np.int32), np.ascontiguousarray(weight + 0.0, dtype=np.float64)


def gauge_arrays(node, weight, B):
    """(node int32, weight float64, per_reach) of fs_batch_set_gauges: [G] shared, or [B, G]"""
    node, weight = np.asarray(node, dtype=np.int32), np.asarray(weight, dtype=np.float64)
    if node.shape != weight.shape or node.ndim not in (1, 2) or (node.ndim == 2 and node.shape[0] != B):
        raise ValueError(f"gauges: node and weight are both [G] or both [B, G] = [{B}, G], not {list(node.shape)} and {list(weight.shape)}")
    return np.ascontiguousarray(node), np.ascontiguousarray(weight), int(node.ndim == 2)


def gauge_row(name):
    """FS_GAUGE_* of a name of _abi.GAUGE_ROWS (an integer 0 .. 3 passes)"""
    if isinstance(name, str):
        if name not in A.GAUGE_ROWS:
            raise ValueError(f"unknown gauge signal {name!r}: one of {', '.join(A.GAUGE_ROWS)}")
        return A.GAUGE_ROWS.index(name)
    return int(name)


def gauge_observed(observed, n, B):
    """(float64 [n] or [n, B], per_reach) of fs_batch_gauge_score; NaN entries stay: they mean "no observation" """
    o = np.ascontiguousarray(observed, dtype=np.float64)
    if o.shape not in ((n,), (n, B)):
        raise ValueError(f"observed must be [n] = [{n}] or [n, B] = [{n}, {B}], not {list(o.shape)}")
    return o, int(o.ndim == 2)


def gauge_options(gauges):
    """(chainage, every, quantiles, observed, signal, rows) of the runners' gauges= keyword: dict(chainage=, every=1,
    quantiles=(0.05, 0.5, 0.95), observed=None, signal="stage", rows=True)"""
    unknown = set(gauges) - {"chainage", "every", "quantiles", "observed", "signal", "rows"}
    if unknown:
        raise ValueError(f"gauges: unknown keys {sorted(unknown)}")
    if "chainage" not in gauges:
        raise ValueError("gauges: chainage is required")
    chainage = np.asarray(gauges["chainage"], dtype=np.float64)
    if chainage.ndim != 1 or not 1 <= len(chainage) <= A.GAUGE_MAX:
        raise ValueError(f"gauges: chainage is [G] with 1 <= G <= {A.GAUGE_MAX}")
    every = gauges.get("every", 1)
    if isinstance(every, bool) or not isinstance(every, (int, np.integer)) or every < 1:
        raise ValueError(f"gauges: every must be an integer >= 1, not {every!r}")
    signal = gauges.get("signal", "stage")
    gauge_row(signal)
    observed = gauges.get("observed")
    return (chainage, int(every), quantile_levels(gauges.get("quantiles", (0.05, 0.5, 0.95))),
            None if observed is None else np.asarray(observed, dtype=np.float64), signal, bool(gauges.get("rows", True)))


# -- assimilation of gauge observations ------------------------------------------------------------
def pack_observations(observations, B, N, perturbations=None, taper=None, depth_floor=1e-3):
    """(n_obs, gauge int32 [m], signal int32 [m], value [m], variance [m], perturb [m, B] | None, taper [m, N] | None, depth_floor)
    of fs_batch_assimilate.  observations: a sequence of (gauge, signal, value, variance) - tuples or objects with those attributes
    (assimilation.Observation) -, signal a name or index of _abi.GAUGE_ROWS.  perturbations: [m, B]; taper: [N] (every observation's)
    or [m, N].  Shapes and the observation count are checked here; what the values may be is the library's to refuse."""
    obs = [(o.gauge, o.signal, o.value, o.variance) if hasattr(o, "gauge") else tuple(o) for o in observations]
    m = len(obs)
    if not 1 <= m <= A.ASSIM_MAX_OBS:
        raise ValueError(f"assimilate: 1 .. {A.ASSIM_MAX_OBS} observations, not {m}")
    if any(len(o) != 4 for o in obs):
        raise ValueError("assimilate: an observation is (gauge, signal, value, variance)")
    gauge = np.ascontiguousarray([int(o[0]) for o in obs], dtype=np.int32)
    signal = np.ascontiguousarray([gauge_row(o[1]) for o in obs], dtype=np.int32)
    value = np.ascontiguousarray([float(o[2]) for o in obs], dtype=np.float64)
    variance = np.ascontiguousarray([float(o[3]) for o in obs], dtype=np.float64)
    if perturbations is not None:
        perturbations = np.ascontiguousarray(perturbations, dtype=np.float64)
        if perturbations.shape != (m, B):
            raise ValueError(f"assimilate: perturbations are [n_obs, B] = [{m}, {B}], not {list(perturbations.shape)}")
    if taper is not None:
        taper = np.asarray(taper, dtype=np.float64)
        if taper.shape not in ((N,), (m, N)):
            raise ValueError(f"assimilate: taper is [N] = [{N}] or [n_obs, N] = [{m}, {N}], not {list(taper.shape)}")
        taper = np.ascontiguousarray(np.broadcast_to(taper, (m, N)))
    return m, gauge, signal, value, variance, perturbations, taper, float(depth_floor)
