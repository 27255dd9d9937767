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
Values that are exact or shared are compared bit for bit and carry no bar."""
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


def all_bars(typ):
    """(label, bar) of every bar of the type"""
    out = [(c["name"], c["bar"]) for c in scalar_cases(typ)]
    for c in node_cases(typ):
        out += [(f"{c['name']}.{f}", b) for f, b in c["bar"].items()] + [(f"{c['name']}.props.{f}", b) for f, b in c["props"]["bar"].items()]
    for c in bc_cases(typ):
        out += [(f"{c['name']}.{c['form']}.{f}", b) for f, b in c["bar"].items()]
    return out
