"""The cases of the device-helper tests: inputs, references and bars (TEST INFRASTRUCTURE, CPU only; shared by
tests/test_helper_reference.py, which checks them on the CPU, and tests/test_gpu_device_helpers.py, which runs the device on them).

Every bar is fixed here, before any device run, from one of four sources:
  stated     a bound the source states for the helper (frcp(double) 2.3e-15, fsqrt_pos(double) 2e-15, frcp(float) 1 ulp = 2^-23,
             log_pos 4e-16 as tests/test_pow_model.py);
  libm pair  pow_pos(double): 1.25 x the error of float64 exp(b log x) on the same points (the criterion of tests/test_pow_model.py);
  4 x noise  four times the worst error of a plain restatement in the working precision (numpy's correctly rounded sqrt, cbrt,
             divide, log2, exp2, exp, power of that type; helper_reference.unary_ref / pow_plain_f32 / k15_ref and, for the fp32
             composites, the whole restatement run in float32) against the same reference on the same points, per function, type
             and parameter set, not below four machine epsilons.  The fp32 pow_pos / pow_ are documented as exp2(b log2 x), so
             that expression in float32 is their restatement: the rounding of b log2 x, up to |b log2 x| 2^-24 ln 2, is part of the
             documented function and of its noise alike;
  1e-12      fp64 composites, the bar of device post-processing in tests/test_gpu_postprocess_geometry.py.
Values that are exact or shared are compared bit for bit and carry no bar.

The Brent root of the general reservoir row has no value to compare with at such a bar: two valid evaluation paths end up to 2 delta
apart.  Its criterion (sc_root_brackets) is the root's own: the reference mass balance changes sign between Y - w and Y + w, or is 0
at Y, with w = FACTOR x (max(delta_D(Y), ulp_D(Y)) + noise_f / A_min): Brent's own half-tolerance (xtol + rtol |Y|) / 2 in the device
type, not below one ulp of Y (a bracket cannot be narrower), plus the stage error that the rounding noise of f in the device type
(the set's worst relative noise of the plain restatement, times the magnitudes of f's terms at Y) makes through the smallest slope of f
in the bracket.  A root point is compared only where the trapezoid of net_vol is at least SWITCH_GAP away from changing its n (f jumps
there and two valid paths may end on different sides); a flag only where |f| at both bracket ends is FLAG_MARGIN x the noise of f or
exactly 0.  tests/test_helper_reference.py checks both conditions, and that scipy's brentq roots meet the criterion."""
import functools

import numpy as np

import helper_reference as HR

N_SCALAR = 1 << 18
N_NODE = 4096
N_BC = 512
FACTOR = 4.0
COMPOSITE_F64 = 1e-12
TYPES = {"f64": np.float64, "f32": np.float32}


def _bar_from_noise(plain, ref, scale=None):
    return FACTOR * HR.noise(plain, ref, scale)


# ------------------------------------------------------------------------------------------------------------------------------
# scalar helpers
# ------------------------------------------------------------------------------------------------------------------------------
STATED = {("frcp", "f64"): 2.3e-15, ("fsqrt_pos", "f64"): 2e-15, ("frcp", "f32"): 2.0 ** -23, ("log_pos", "f64"): 4e-16}


@functools.lru_cache(maxsize=None)
def scalar_cases(typ):
    """list of dicts: name, call ("unary", op code | "pow", 0 pow_pos / 1 pow_ | "k15"), x (tuple of device-typed inputs), ref, bar,
    source, and for pow_pos(double) `pair`: the error of the float64 libm pair on the same points"""
    D = TYPES[typ]
    T = HR.reference_type(D)
    rng = np.random.default_rng(20261020)
    out = []
    edges = HR.edge_points(1e-6, 1e6, D)
    x = np.concatenate([HR.log_uniform(rng, 1e-6, 1e6, N_SCALAR - len(edges), D), edges])
    for code, op in enumerate(HR.UNARY_OPS):
        if op in ("log_pos", "exp_short"):
            if typ != "f64":
                continue
            if op == "log_pos":
                e = HR.edge_points(1e-4, 1e4, D)
                near = (1.0 + rng.uniform(-2e-4, 2e-4, 4096)).astype(D)
                xs = np.concatenate([HR.log_uniform(rng, 1e-4, 1e4, N_SCALAR - len(e) - 4096, D), near, e])
            else:
                k = np.arange(-86, 87)
                half = ((k + 0.5) * np.log(2.0)).astype(D)              # where the reduction's k steps
                e = np.concatenate([half, np.nextafter(half, D(-100)), np.nextafter(half, D(100)), np.array([0.0, 5e-324, -5e-324, 1e-17, -1e-17, 60.0, -60.0], dtype=D)])
                e = e[np.abs(e) <= 60]
                xs = np.concatenate([rng.uniform(-60, 60, N_SCALAR - len(e)).astype(D), e])
        else:
            xs = x
        ref = HR.unary_ref(op, xs.astype(T))
        if (op, typ) in STATED:
            bar, src = STATED[(op, typ)], "stated"
        else:
            bar, src = _bar_from_noise(HR.unary_ref(op, xs), ref), "4 x noise"
        out.append(dict(name=op, call=("unary", code), x=(xs,), ref=ref, bar=bar, source=src))
    grids = [("", (1e-4, 1e4), (0.2, 5.0))] + ([("[rating]", (0.1, 100.0), (0.5, 3.0))] if typ == "f32" else [])
    for tag, (xlo, xhi), (blo, bhi) in grids:
        e = HR.edge_points(xlo, xhi, D)
        a = np.concatenate([HR.log_uniform(rng, xlo, xhi, N_SCALAR - len(e), D), e])
        b = rng.uniform(blo, bhi, N_SCALAR).astype(D)
        ref = HR.pow_ref(a.astype(T), b.astype(T))
        if typ == "f64":
            pair, _ = HR.worst(HR.pow_libm_pair(a, b), ref)
            out.append(dict(name="pow_pos", call=("pow", 0), x=(a, b), ref=ref, bar=1.25 * pair, source="libm pair", pair=pair))
        else:
            bar = _bar_from_noise(HR.pow_plain_f32(a, b), ref)
            out.append(dict(name="pow_pos" + tag, call=("pow", 0), x=(a, b), ref=ref, bar=bar, source="4 x noise"))
            out.append(dict(name="pow_" + tag, call=("pow", 1), x=(a, b), ref=ref, bar=bar, source="4 x noise"))
    # k15_(A, P, n^-1.5): areas and perimeters of sub-sections, Manning's n 0.01 .. 0.2
    A = HR.log_uniform(rng, 1e-6, 1e6, N_SCALAR, D)
    P = HR.log_uniform(rng, 1e-2, 1e4, N_SCALAR, D)
    n15 = HR.unary_ref("pm15_", HR.log_uniform(rng, 0.01, 0.2, N_SCALAR, D))
    ref = HR.k15_ref(A.astype(T), P.astype(T), n15.astype(T))
    out.append(dict(name="k15_", call=("k15", 0), x=(A, P, n15), ref=ref, bar=_bar_from_noise(HR.k15_ref(A, P, n15), ref), source="4 x noise"))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# node terms
# ------------------------------------------------------------------------------------------------------------------------------
COMPOUND = dict(b=30.0, m=1.5, nm=0.03, nl=0.06, nr=0.06, compound=1.0, hbf=4.0, bl=50.0, br=80.0, mfp=3.0)
# (name, parameters, the closed-form fast path that applies besides the general one)
SECTIONS = (
    ("rect_5m", dict(b=5.0, nm=0.025), "rect"),
    ("rect_2km", dict(b=2000.0, nm=0.035), "rect"),
    ("trap_5m_m0.5", dict(b=5.0, m=0.5, nm=0.03), "trap"),
    ("trap_2km_m2.5", dict(b=2000.0, m=2.5, nm=0.04), "trap"),
    ("trap_curv_1e-3", dict(b=40.0, m=2.5, nm=0.03, curv=1e-3), None),
    ("rect_curv_1e-13", dict(b=25.0, nm=0.03, curv=1e-13), None),            # residual term on, derivative terms off
    ("compound", dict(COMPOUND), None),
    ("compound_zero_width_fp", dict(COMPOUND, bl=0.0, br=0.0), None),
    ("compound_unequal_n", dict(COMPOUND, nl=0.05, nr=0.09, bl=120.0), None),
    ("compound_mfp_0", dict(COMPOUND, mfp=0.0, bl=100.0, br=60.0), None),
    ("compound_curv_1e-3", dict(COMPOUND, curv=1e-3), None),
    ("compound_empty_fp_curv_1e-13", dict(COMPOUND, bl=0.0, br=0.0, mfp=0.0, curv=1e-13), None),
)
K_EQ_SCALE = {"rect": 2, "trap": 2, "general": 1}       # Geometry<...>::kEQScale of the family (fs_kernel.hpp)
FORM_CODE = {"rect": 0, "trap": 1, "general": 2}


def node_points(sec, D, seed):
    """4 096 (h, Q): h log-uniform in 0.05 .. 60 m, Q of both signs and Q = 0; a compound section also gets d == h_bf exactly and the
    next number above it"""
    rng = np.random.default_rng(seed)
    h = HR.log_uniform(rng, 0.05, 60.0, N_NODE, D)
    Q = (HR.log_uniform(rng, 1e-2, 1e4, N_NODE, D) * rng.choice(np.array([-1, 1], dtype=D), N_NODE)).astype(D)
    Q[::16] = 0
    if sec["compound"] > 0.5:
        h[1:9:2] = sec["hbf"]
        h[2:10:2] = np.nextafter(sec["hbf"], D(np.inf))
    return h, Q


@functools.lru_cache(maxsize=None)
def node_cases(typ):
    """list of dicts: name, sec, forms, h, Q, ref / scale (field -> array), bar (field -> float), and `props`: the same for the
    thirteen GeneralProps fields"""
    D = TYPES[typ]
    T = HR.reference_type(D)
    out = []
    for i, (name, kw, fast) in enumerate(SECTIONS):
        sec = HR.section(D, **kw)
        h, Q = node_points(sec, D, 100 + i)
        ref, scale = HR.node_terms(sec, h, Q, T)
        g = HR.general_props(sec, h, T)
        gscale = HR.props_scales(g)
        if typ == "f64":
            bar = {f: COMPOSITE_F64 for f in HR.NODE_FIELDS}
            gbar = {f: COMPOSITE_F64 for f in HR.PROP_FIELDS}
        else:
            plain, _ = HR.node_terms(sec, h, Q, D)
            bar = {f: _bar_from_noise(plain[f], ref[f], scale[f]) for f in HR.NODE_FIELDS}
            gp = HR.general_props(sec, h, D)
            gbar = {f: _bar_from_noise(gp[f], g[f], gscale[f]) for f in HR.PROP_FIELDS}
        out.append(dict(name=name, sec=sec, forms=([fast] if fast else []) + ["general"], h=h, Q=Q, ref=ref, scale=scale, bar=bar,
                        props=dict(ref=g, scale=gscale, bar=gbar)))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# boundary rows
# ------------------------------------------------------------------------------------------------------------------------------
Z = 12.5                                                   # bed level of the boundary node's section
BLEND = dict(s0=14.0, lo=(5.0, 2.0, 1.5), hi=(20.0, 1.0, 2.5), dY=1e-3)
STORAGE = dict(area=2.5e5, min_stage=13.0, Y_min=10.0, Y_max=20.0, bed=Z)
DT = 60.0


def _params(D, *v):
    p = np.zeros(10, dtype=D)
    p[:len(v)] = v
    return p


def bc_sets(D):
    """(name, kind, params, bed level of the section, level, forms): one launch each"""
    K = HR.KINDS
    both, general = ("general", "rect"), ("general",)
    sets = [
        ("flow", K["flow"], _params(D), Z, 2, both),
        ("stage", K["stage"], _params(D, Z), Z, 2, both),
        ("fixed", K["fixed"], _params(D, 3.25), Z, 2, both),
        ("normal_S0+_same_bed_0", K["normal"], _params(D, 1e-3, 0.0), 0.0, 2, both),      # hd == h exactly: the shared reciprocal
        ("normal_S0-_same_bed", K["normal"], _params(D, -4e-4, Z), Z, 2, both),
        ("normal_S0+_bed_off_0.3", K["normal"], _params(D, 2e-4, Z + 0.3), Z, 2, both),   # hd != h
        ("power_shift", K["power"], _params(D, 4.5, 1.6, 0.25, Z), Z, 2, general),
        ("poly", K["poly"], _params(D, 2.0, 15.0, 5.0, 0.5, 1.5), Z, 2, both),
    ]
    for buf in (0.3, 0.5):
        sets.append((f"blend_buf_{buf}", K["blend"], _params(D, BLEND["s0"], buf, *BLEND["lo"], *BLEND["hi"], BLEND["dY"], Z), Z, 2, both))
    s = STORAGE
    for level in (1, 2):
        sets.append((f"storage_level_{level}", K["storage"], _params(D, s["area"], s["min_stage"], s["Y_min"], s["Y_max"], s["bed"]), Z, level, both))
    return sets


def bc_points(name, params, D, seed):
    """512 (h, Q, Qold, Yprev, target) for one parameter set"""
    rng = np.random.default_rng(seed)
    n = N_BC
    h = HR.log_uniform(rng, 0.2, 20.0, n, D)
    sign = lambda: rng.choice(np.array([-1, 1], dtype=D), n)
    Q = (HR.log_uniform(rng, 1.0, 5e3, n, D) * sign()).astype(D)
    Qold = (HR.log_uniform(rng, 1.0, 5e3, n, D) * sign()).astype(D)
    Yprev = rng.uniform(13.5, 19.0, n).astype(D)
    tgt = (HR.log_uniform(rng, 1.0, 5e3, n, D) * sign()).astype(D)
    if name == "stage":
        tgt = (D(Z) + HR.log_uniform(rng, 0.2, 20.0, n, D)).astype(D)
    if name.startswith("blend"):
        # stages below s0, inside the buffer and above it, and within dY of both edges, so that z - dY, z, z + dY fall on different sides
        s0, buf, dY = float(params[0]), float(params[1]), float(params[8])
        z = rng.uniform(s0 - 1.0, s0 + buf + 1.0, n)
        near = np.array([-1.5, -1.0, -0.75, -0.25, 0.0, 0.25, 0.75, 1.0, 1.5]) * dY
        z[:9], z[9:18] = s0 + near, s0 + buf + near
        h = (z.astype(D) - D(Z)).astype(D)
    if name.startswith("storage"):
        # a third as drawn; a third whose outflow puts Y below min_stage (still inside the range: the floor holds, dq loses its
        # 1 / area term); a third whose Y leaves [Y_min, Y_max] at either end (FS_STORAGE_RANGE)
        k = n // 3
        per_m = 2.0 * STORAGE["area"] / DT                            # flow sum that moves the stage by 1 m
        Q[:k] = (rng.uniform(-0.2, 0.2, k) * per_m).astype(D)
        Qold[:k] = (rng.uniform(-0.2, 0.2, k) * per_m).astype(D)
        h[:2 * k] = rng.uniform(2.0, 6.0, 2 * k).astype(D)          # Yold = h + bed = 14.5 .. 18.5 at level 1, Yprev at level 2
        Qold[k:2 * k] = 0
        Q[k:2 * k] = (-rng.uniform(6.2, 6.8, k) * per_m).astype(D)    # Y = Yold - 6.2 .. 6.8: 6.7 .. 12.8 - below 13
        h[2 * k:] = rng.uniform(2.0, 6.0, n - 2 * k).astype(D)
        Qold[2 * k:] = 0
        Q[2 * k:] = (rng.choice([-1.0, 1.0], n - 2 * k) * rng.uniform(9.5, 12.0, n - 2 * k) * per_m).astype(D)
    return h, Q, Qold, Yprev, tgt


def bc_section(form, z, D):
    return HR.section(D, z=z, **COMPOUND) if form == "general" else HR.section(D, z=z, b=25.0, nm=0.03)


@functools.lru_cache(maxsize=None)
def bc_cases(typ):
    """list of dicts: name, form, kind, params, sec, level, dt, the five input arrays, ref (helper_reference.bc_row in the reference
    type) and bar: output -> float for res, dh, Ynew where they are not exact"""
    D = TYPES[typ]
    T = HR.reference_type(D)
    out = []
    for i, (name, kind, params, z, level, forms) in enumerate(bc_sets(D)):
        pts = bc_points(name, params, D, 500 + i)
        for form in forms:
            sec = bc_section(form, z, D)
            ref = HR.bc_row(kind, params, sec, level, D(DT), *pts, T)
            fields = [f for f in ("res", "dh") if f not in ref["exact"]] + (["Ynew"] if kind == HR.KINDS["storage"] else [])
            scales = dict(res=ref["s_res"], dh=ref["s_dh"], Ynew=ref["s_Y"])
            if typ == "f64":
                bar = {f: COMPOSITE_F64 for f in fields}
            else:
                plain = HR.bc_row(kind, params, sec, level, D(DT), *pts, D)
                bar = {f: _bar_from_noise(plain[f], ref[f], scales[f]) for f in fields}
            out.append(dict(name=name, form=form, kind=kind, params=params, sec=sec, level=level, dt=D(DT), pts=pts, ref=ref, scales=scales, bar=bar))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# the general reservoir row (FS_BC_STORAGE_CURVE) and the host row
# ------------------------------------------------------------------------------------------------------------------------------
DT_SC = 900.0
Y_LO, Y_HI = 10.0, 20.0                                    # the bracket of every set
CURVE2 = [[10.0, 1.0e5], [20.0, 9.0e5]]
# gaps 1, 0.5, 1.5, 3, 4: the step is the second gap; (Y_HI - Y_LO) / step = 20 trapezoid points at the most (the probe's rule: <= 64)
CURVE6 = [[10.0, 1.0e5], [11.0, 1.5e5], [11.5, 2.2e5], [13.0, 2.4e5], [16.0, 5.0e5], [20.0, 9.0e5]]
POLY = dict(type="polynomial", a=3.0, b=2.0, c=-300.0, shift=0.0)          # dq/dY = 6 Y + 2 > 0, q > 0 on the bracket
POWER = dict(type="power", a=2.5, b=1.6, shift=-9.0)                       # x = Y - 9 in 1 .. 11 over the bracket
LOSSES = dict(reservoir_length=2.0e4, K_q=0.5)
Z1 = 8.0                                                   # bed of the level-1 sets: Yold = h + bed, so the bed lies below the bracket
SWITCH_GAP = 1e-3
MAX_DROPPED = 0.05
FLAG_MARGIN = 1000.0


def sc_sets(D):
    """(name, params, bed level of the section, level): the section is the compound one of the other rows"""
    base = dict(Y_min=Y_LO, Y_max=Y_HI, min_stage=10.75, bed=Z)
    P = lambda **kw: HR.sc_params(D, **dict(base, **kw))
    return [
        ("const_area", P(area=2.5e5), Z, 2),                                                   # root Yold + vol / area
        ("curve2", P(curve=CURVE2, bed=Z1), Z1, 1),
        ("curve6", P(curve=CURVE6), Z, 2),
        ("curve6_alpha_beta_poly", P(curve=CURVE6, alpha=0.8, beta=0.25, rc=POLY), Z, 2),
        ("curve6_power_shift", P(curve=CURVE6, rc=POWER, bed=Z1), Z1, 1),
        ("curve6_poly_losses_bed_off", P(curve=CURVE6, rc=POLY, losses=LOSSES, bed=Z + 0.3), Z, 2),    # bed_level != sec.z: two depths
        ("curve6_power_losses_same_bed", P(curve=CURVE6, alpha=1.25, rc=POWER, losses=LOSSES, bed=Z1), Z1, 1),
    ]


def _around(v, D):
    v = np.asarray(v, dtype=D)
    return np.concatenate([v, np.nextafter(v, D(-np.inf)), np.nextafter(v, D(np.inf))])


def sc_area_points(p, rng):
    """stages for area_at (and outflow): random ones from below the curve to above it, and Y + beta on every breakpoint, one ulp to
    either side, below xs(0) and above xs(nc - 1)"""
    D = p.dtype.type
    xs, _ = HR.sc_curve(p)
    beta = p[HR.SC["beta"]]
    special = np.concatenate([_around(xs, D) - beta, np.array([Y_LO - 1.0, Y_LO - 0.5, Y_HI + 0.5, Y_HI + 3.0], dtype=D)])
    return np.concatenate([special, rng.uniform(Y_LO - 1.0, Y_HI + 1.0, N_BC - len(special)).astype(D)])


def sc_vol_points(p, rng):
    """(Y1, Y2) for net_vol: |Y2 - Y1| / step at 1.9, 2, 2.99, 3, 3.01 with both signs, the largest n of the set, Y1 == Y2, random"""
    D = p.dtype.type
    step = float(HR.sc_step(p))
    q = np.array([1.9, 2.0, 2.99, 3.0, 3.01])
    y1 = np.concatenate([np.full(5, 14.0), np.full(5, 14.0), [Y_LO, Y_HI, 13.0, 17.5]])
    y2 = np.concatenate([14.0 + q * step, 14.0 - q * step, [Y_HI, Y_LO, 13.0, 17.5]])
    k = N_BC - len(y1)
    y1 = np.concatenate([y1, rng.uniform(Y_LO, Y_HI, k)]).astype(D)
    y2 = np.concatenate([y2, rng.uniform(Y_LO, Y_HI, k)]).astype(D)
    return y1, y2


ROOT_SPECIAL = ("largest_n", "floor", "at_min_stage", "f_lo_zero", "f_hi_zero", "both_negative", "both_positive", "nan")


def sc_root_points(name, p, rng):
    """(Yold, vol, tags) for storage_root.  A point is made from the stage Y* it should return: vol = f(Y*) + vol in float64, rounded to
    the device type.  tags: index -> name of the special points; every other point is random with Y* 0.2 m inside the bracket."""
    D = p.dtype.type
    n = N_BC
    ymin = float(p[HR.SC["min_stage"]])
    yold = rng.uniform(Y_LO + 0.5, Y_HI - 1.0, n)
    ystar = rng.uniform(Y_LO + 0.2, Y_HI - 0.2, n)
    tags = {}
    yold[0], ystar[0] = Y_LO, Y_HI - 0.2                                  # the largest n of the set
    tags[0] = "largest_n"
    ystar[1:9] = rng.uniform(Y_LO + 0.1, ymin - 0.05, 8)                  # a root below min_stage: the row floors it
    tags.update({i: "floor" for i in range(1, 9)})
    yold[9], ystar[9] = 12.0, ymin                                        # a root at min_stage
    tags[9] = "at_min_stage"
    yold[10:12], ystar[10], ystar[11] = 12.0, Y_LO, Y_HI                  # f(Y_min) == 0, f(Y_max) == 0 (exact with a constant area)
    tags.update({10: "f_lo_zero", 11: "f_hi_zero"})
    ystar[12:16] = Y_HI + np.array([1.0, 2.0, 5.0, 30.0])                 # f < 0 at both ends
    ystar[16:20] = Y_LO - np.array([1.0, 2.0, 5.0, 30.0])                 # f > 0 at both ends
    tags.update({i: "both_negative" for i in range(12, 16)})
    tags.update({i: "both_positive" for i in range(16, 20)})
    yold = yold.astype(D)
    f0, _ = HR.sc_f(p, yold, np.zeros(n), DT_SC, ystar, np.float64, n=HR.sc_trapezoid_n(p, yold.astype(np.float64), ystar))
    vol = f0.astype(D)                                                    # f(Y*) with vol = 0 is the volume that puts the root at Y*
    vol[20] = np.nan
    tags[20] = "nan"
    if name != "const_area":                                              # not constructible exactly on a curve: ordinary root points there
        tags = {i: t for i, t in tags.items() if t not in ("f_lo_zero", "f_hi_zero")}
        ystar[10], ystar[11] = Y_LO + 0.3, Y_HI - 0.3
        vol[10:12] = HR.sc_f(p, yold[10:12], np.zeros(2), DT_SC, ystar[10:12], np.float64,
                             n=HR.sc_trapezoid_n(p, yold[10:12].astype(np.float64), ystar[10:12]))[0].astype(D)
    return yold, vol, tags


def sc_row_points(p, level, yold, vol, rng):
    """(h, Q, Qold, Yprev) that hand the row the reservoir states of the root points: Yold = Yprev at level 2 and h + bed at level 1
    (where Yprev holds a stage that must be ignored), vol = (Qold + Q) dt / 2"""
    D = p.dtype.type
    n = len(yold)
    qsum = (2.0 * vol.astype(np.float64) / DT_SC)
    Qold = (rng.uniform(0.2, 0.8, n) * qsum).astype(D)
    Q = (qsum - Qold.astype(np.float64)).astype(D)
    if level == 1:
        h = (yold - p[HR.SC["bed"]]).astype(D)
        Yprev = rng.uniform(Y_LO + 1.0, Y_HI - 1.0, n).astype(D)
    else:
        h = rng.uniform(0.5, 7.0, n).astype(D)
        Yprev = yold.copy()
    return h, Q, Qold, Yprev


def _noise_of(fn, D, T, scale_of=lambda r: r[1]):
    """(reference, scale, relative noise of the plain restatement in D against it)"""
    ref = fn(T)
    plain = fn(D)
    return ref[0], scale_of(ref), HR.noise(plain[0], ref[0], scale_of(ref))


@functools.lru_cache(maxsize=None)
def sc_cases(typ):
    """list of dicts, one per parameter set: params, sec, level, the points of each op with reference, scale and bar, and for the root:
    yold, vol, tags, `root_mask` (the points whose returned stage is compared), `flag` (what storage_root must report), noise_f"""
    D = TYPES[typ]
    T = HR.reference_type(D)
    out = []
    for i, (name, p, z, level) in enumerate(sc_sets(D)):
        rng = np.random.default_rng(900 + i)
        c = dict(name=name, params=p, sec=HR.section(D, z=z, **COMPOUND), level=level, dt=D(DT_SC))
        bar = lambda nz: COMPOSITE_F64 if typ == "f64" else FACTOR * nz
        ya = sc_area_points(p, rng) if int(p[HR.SC["n_curve"]]) else rng.uniform(Y_LO - 1.0, Y_HI + 1.0, N_BC).astype(D)
        ref, _, nz = _noise_of(lambda t: (HR.sc_area_at(p, ya, t), None), D, T)
        c["area"] = dict(Y=ya, ref=ref, bar=bar(nz))
        ref, sc, nz = _noise_of(lambda t: HR.sc_outflow(p, ya, t), D, T)
        c["outflow"] = dict(Y=ya, ref=ref, scale=sc, bar=bar(nz))
        y1, y2 = sc_vol_points(p, rng)
        ref, sc, nz = _noise_of(lambda t: HR.sc_net_vol(p, y1, y2, t), D, T)
        c["net_vol"] = dict(Y1=y1, Y2=y2, ref=ref, scale=sc, bar=bar(nz))
        yold, vol, tags = sc_root_points(name, p, rng)
        c.update(yold=yold, vol=vol, tags=tags, root=sc_root_expectations(p, yold, vol, tags, D, T))
        h, Q, Qold, Yprev = c["row_pts"] = sc_row_points(p, level, yold, vol, rng)
        # the reservoir state the row forms from them, in its own arithmetic, and what its root finder must report on it
        with np.errstate(all="ignore"):
            c["row_yold"] = (h + p[HR.SC["bed"]]) if level == 1 else Yprev
            c["row_vol"] = D(0.5) * (Qold + Q) * D(DT_SC)
        c["row_root"] = sc_root_expectations(p, c["row_yold"], c["row_vol"], tags, D, T)
        out.append(c)
    return out


def sc_switch_distance(p, yold, Y):
    """how far |Y - Yold| / step is from an integer (1 without a curve: the trapezoid never changes its form)"""
    if int(p[HR.SC["n_curve"]]) == 0:
        return np.ones(len(yold))
    q = np.abs(np.asarray(Y, dtype=np.float64) - yold.astype(np.float64)) / float(HR.sc_step(p))
    return np.abs(q - np.round(q))


def sc_root_expectations(p, yold, vol, tags, D, T):
    """flag: FS_OK / FS_STORAGE_RANGE from the signs of the reference f at the bracket ends (NaN: range); `end`: +-1 where f(end) == 0
    makes storage_root return that end; noise_f: the relative rounding noise of f in D (scale: the magnitudes of its terms) over the
    bracket ends; margin: |f| / (noise_f x scale) at each end"""
    n = len(yold)
    lo, hi = np.full(n, p[HR.SC["Y_min"]]), np.full(n, p[HR.SC["Y_max"]])
    finite = np.isfinite(vol)
    v0 = np.where(finite, vol, D(0))
    ends = {}
    nz = 0.0
    for k, y in (("lo", lo), ("hi", hi)):
        ref, mag = HR.sc_f(p, yold, v0, DT_SC, y, T)
        plain, _ = HR.sc_f(p, yold, v0, DT_SC, y, D)
        nz = max(nz, HR.noise(plain, ref, mag))
        ends[k] = (ref, mag, plain)
    zero = {k: (ends[k][2] == 0) & (ends[k][0] == 0) for k in ends}               # exact by construction: zero in D and in T
    flo, fhi = ends["lo"][0], ends["hi"][0]
    ok = finite & (zero["lo"] | zero["hi"] | ((flo < 0) != (fhi < 0)))
    margin = np.minimum(np.abs(flo) / (nz * ends["lo"][1]), np.abs(fhi) / (nz * ends["hi"][1])).astype(np.float64)
    margin = np.where(zero["lo"] | zero["hi"] | ~finite, np.inf, margin)
    return dict(flag=np.where(ok, HR.FS_OK, HR.FS_STORAGE_RANGE).astype(np.int32), end=np.where(zero["lo"], -1, np.where(zero["hi"], 1, 0)),
                noise_f=nz, margin=margin, is_root=ok & ~zero["lo"] & ~zero["hi"])


def sc_root_width(c, Y, typ):
    """w of the root criterion at the returned stages Y: FACTOR x (max(delta_D(Y), ulp_D(Y)) + noise_f / A_min), with noise_f the set's
    relative noise of f in D times the magnitudes of f's terms at Y"""
    D = TYPES[typ]
    p = c["params"]
    Y = np.asarray(Y, dtype=D)
    _, mag = HR.sc_f(p, c["yold"], np.where(np.isfinite(c["vol"]), c["vol"], D(0)), DT_SC, Y, np.float64 if typ == "f32" else HR.LD)
    half = np.maximum(HR.brent_delta(Y).astype(np.float64), np.spacing(np.abs(Y)).astype(np.float64))
    return FACTOR * (half + c["root"]["noise_f"] * mag.astype(np.float64) / HR.sc_min_slope(p))


def sc_root_brackets(c, Y, typ):
    """the root criterion: the reference f changes sign between Y - w and Y + w, or is 0 at Y (the trapezoid's n is the one of Y).
    Returns per point the multiple k of w / FACTOR, among 1, 2 and FACTOR, at which it holds (inf: at none): it is met where k <= FACTOR"""
    D = TYPES[typ]
    T = HR.reference_type(D)
    p = c["params"]
    Y = np.asarray(Y, dtype=D)
    v = np.where(np.isfinite(c["vol"]), c["vol"], D(0))
    n = HR.sc_trapezoid_n(p, c["yold"], Y)
    w = sc_root_width(c, Y, typ) / FACTOR
    at = HR.sc_f(p, c["yold"], v, DT_SC, Y, T, n=n)[0]
    need = np.full(len(Y), np.inf)
    for k in (FACTOR, 2.0, 1.0):
        a = HR.sc_f(p, c["yold"], v, DT_SC, Y.astype(T) - T(k) * w.astype(T), T, n=n)[0]
        b = HR.sc_f(p, c["yold"], v, DT_SC, Y.astype(T) + T(k) * w.astype(T), T, n=n)[0]
        need = np.where((at == 0) | ((a <= 0) != (b <= 0)), k, need)
    return need


def sc_brentq_roots(c):
    """scipy's brentq on the oracle's float64 mass balance (lumped_storage.py:24-31) at every root point; NaN elsewhere"""
    from scipy.optimize import brentq
    from oracle import preissmann_oracle as O
    st = HR.sc_oracle_st(c["params"])
    out = np.full(len(c["yold"]), np.nan)
    for i in np.nonzero(c["root"]["is_root"])[0]:
        yo, vol = float(c["yold"][i]), float(c["vol"][i])

        def f(Y):
            q = 0.5 * (O.storage_outflow(st, yo) + O.storage_outflow(st, Y)) if st.get("rc") is not None else 0.0
            return O.storage_net_vol(st, yo, Y) - (vol - q * DT_SC)
        out[i] = brentq(f, st["Y_min"], st["Y_max"])
    return out


@functools.lru_cache(maxsize=None)
def sc_reference_roots(typ):
    """set name -> sc_brentq_roots of the set, computed once"""
    return {c["name"]: sc_brentq_roots(c) for c in sc_cases(typ)}


def sc_compared(c, Y):
    """the root points whose returned stage Y stays in the comparison: away from a switch of the trapezoid's n"""
    return c["root"]["is_root"] & (sc_switch_distance(c["params"], c["yold"], Y) >= SWITCH_GAP)


HOST_ROW_B = 65


def host_rows(D):
    """params[3][65]: dh, dq, res of 65 reaches as a caller would leave them, a NaN and an inf among them"""
    rng = np.random.default_rng(77)
    rows = (HR.log_uniform(rng, 1e-6, 1e6, 3 * HOST_ROW_B, np.float64) * rng.choice([-1.0, 1.0], 3 * HOST_ROW_B)).astype(D).reshape(3, HOST_ROW_B)
    rows[0, 3], rows[1, 17], rows[2, 40], rows[2, 64], rows[0, 64] = np.nan, np.inf, -np.inf, np.nan, 0.0
    return rows


def all_bars(typ):
    """(label, bar) of every bar of the type"""
    out = [(c["name"], c["bar"]) for c in scalar_cases(typ)]
    for c in node_cases(typ):
        out += [(f"{c['name']}.{f}", b) for f, b in c["bar"].items()] + [(f"{c['name']}.props.{f}", b) for f, b in c["props"]["bar"].items()]
    for c in bc_cases(typ):
        out += [(f"{c['name']}.{c['form']}.{f}", b) for f, b in c["bar"].items()]
    for c in sc_cases(typ):
        out += [(f"storage_curve.{c['name']}.{f}", c[f]["bar"]) for f in ("area", "outflow", "net_vol")]
    return out
