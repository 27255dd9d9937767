"""High-precision restatement of the device helpers, node terms and boundary rows of flow-sim_amd/csrc/fs_device.hpp, generic over the
number type (TEST INFRASTRUCTURE: tests/test_helper_reference.py holds it to the oracle and to mpmath on the CPU,
tests/test_gpu_device_helpers.py holds the device functions to it).

The formulas are the reference's, as oracle/preissmann_oracle.py states them (section_props, conveyance, equivalent_n, dR_dA, dK_dA,
the curvature terms of node_terms, the boundary rows with their two evaluation depths and the rating derivatives), not the device's
rearrangements.  `T` is the type the arithmetic runs in: np.longdouble for the fp64 device functions, np.float64 for the fp32 ones,
and the device's own type for the "plain restatement" whose rounding noise sets the bars.  `D` is the device's type: inputs are
exactly representable in it, and every branch (d > h_bf, z <= s0, z >= s0 + buf, Y < min_stage, the storage range; of the general
reservoir row the interpolation interval and the clamping of the area curve, the trapezoid's n, level == 1, the floor at min_stage and
capture_losses) is decided in it, from the inputs, as the device decides - the two sides of a comparison never sit on different branches.

Nothing here imports the package or needs a GPU."""
import numpy as np

LD = np.longdouble
G = "9.80665"            # scipy.constants.g (hydraulics.py:2), as text: exact in every type
SEC_KEYS = ("z", "b", "m", "nm", "nl", "nr", "compound", "hbf", "bl", "br", "mfp", "curv")      # the FS_GEO_* rows, in order
NODE_FIELDS = ("A", "T", "Se", "eAT", "eQ", "v", "rT")                                       # NodeTerms (eQ = eQh * kEQScale)
PROP_FIELDS = ("A", "rA", "P", "Rh", "T", "rT", "K", "rK", "neq", "dRdA", "dKdA", "dKdA_K", "y13")   # GeneralProps
DERIVE_FIELDS = ("sm", "sfp", "Tb", "Am", "Pm", "rnm", "km15", "kl15", "kr15")
KINDS = dict(flow=0, stage=1, fixed=2, normal=3, power=4, poly=5, blend=6, storage=7)          # FS_BC_*
FS_OK, FS_STORAGE_RANGE = 0, 3


def reference_type(D):
    """the type a device type is checked in"""
    if D == np.float64:
        assert np.finfo(LD).eps < 1e-18, "np.longdouble is no wider than double here: no reference for the fp64 functions"
        return LD
    return np.float64


def section(D, **kw):
    """the twelve caller-side parameters of a trapezoid-family section, rounded to the device type"""
    s = dict(z=0.0, b=10.0, m=0.0, nm=0.03, nl=0.03, nr=0.03, compound=0.0, hbf=0.0, bl=0.0, br=0.0, mfp=0.0, curv=0.0)
    s.update(kw)
    return {k: D(s[k]) for k in SEC_KEYS}


def sec_array(sec, D):
    return np.array([sec[k] for k in SEC_KEYS], dtype=D)


def oracle_geo(sec):
    """the section as a one-node geo dict of oracle/preissmann_oracle.py (GEO_KEYS is SEC_KEYS under the reference's names)"""
    from oracle import preissmann_oracle as O
    return {g: np.array([float(sec[k])]) for g, k in zip(O.GEO_KEYS, SEC_KEYS)}


# ------------------------------------------------------------------------------------------------------------------------------
# scalar helpers
# ------------------------------------------------------------------------------------------------------------------------------
UNARY_OPS = ("frcp", "frsq", "rcbrt_pos", "rcbrt2_pos", "fsqrt_pos", "p23_", "p32_", "pm15_", "log_pos", "exp_short")   # op codes


def unary_ref(op, x):
    """the function a unary helper stands for, in the type of x, from numpy's sqrt / cbrt / divide / log / exp of that type: the
    reference when x is wide, the plain restatement when x has the device's type"""
    T = x.dtype.type
    with np.errstate(all="ignore"):
        if op == "frcp":
            return T(1) / x
        if op == "frsq":
            return T(1) / np.sqrt(x)
        if op == "rcbrt_pos":
            return T(1) / np.cbrt(x)
        if op == "rcbrt2_pos":
            c = np.cbrt(x)
            return T(1) / (c * c)
        if op == "fsqrt_pos":
            return np.sqrt(x)
        if op == "p23_":
            c = np.cbrt(x)
            return c * c
        if op == "p32_":
            return x * np.sqrt(x)
        if op == "pm15_":
            return T(1) / (x * np.sqrt(x))
        if op == "log_pos":
            return np.log(x)
        if op == "exp_short":
            return np.exp(x)
    raise KeyError(op)


def unary_mp(op, x):
    """the same function of one mpmath number"""
    import mpmath as mp
    return {"frcp": lambda: 1 / x, "frsq": lambda: 1 / mp.sqrt(x), "rcbrt_pos": lambda: 1 / mp.cbrt(x), "rcbrt2_pos": lambda: 1 / mp.cbrt(x) ** 2,
            "fsqrt_pos": lambda: mp.sqrt(x), "p23_": lambda: mp.cbrt(x) ** 2, "p32_": lambda: x * mp.sqrt(x), "pm15_": lambda: 1 / (x * mp.sqrt(x)),
            "log_pos": lambda: mp.log(x), "exp_short": lambda: mp.exp(x)}[op]()


def pow_ref(a, b):
    with np.errstate(all="ignore"):
        return np.power(a, b)


def pow_plain_f32(a, b):
    """what the fp32 pow_pos / pow_ are documented to be, exp2(b log2 a), from numpy's float32 log2, multiply and exp2"""
    with np.errstate(all="ignore"):
        return np.exp2(b * np.log2(a))


def pow_libm_pair(a, b):
    """float64 exp(b log x): what pow_pos(double) replaced and is measured against (tests/test_pow_model.py)"""
    return np.exp(b * np.log(a))


def k15_ref(A, P, n15):
    """K_i^1.5 of a sub-section with K_i = A R^(2/3) / n: A^2.5 / P * n^-1.5; 0 when A or P is 0"""
    T = A.dtype.type
    with np.errstate(all="ignore"):
        return np.where((A > 0) & (P > 0), np.power(A, T(5) / T(2)) / P * n15, T(0))


def log_uniform(rng, lo, hi, n, D):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n)).astype(D)


def edge_points(lo, hi, D, k_ulp=8):
    """every power of two in [lo, hi] with its two neighbours (the neighbours of the powers of 8, where the cube root's exponent
    steps, are among them) and 1 +- k ulp"""
    e = np.arange(int(np.ceil(np.log2(lo))), int(np.floor(np.log2(hi))) + 1)
    p = np.ldexp(D(1), e).astype(D)
    pts = [p, np.nextafter(p, D(0)), np.nextafter(p, D(np.inf))]
    one = [D(1)]
    up = dn = D(1)
    for _ in range(k_ulp):
        up, dn = np.nextafter(up, D(2)), np.nextafter(dn, D(0))
        one += [up, dn]
    x = np.concatenate(pts + [np.array(one, dtype=D)])
    return x[(x >= D(lo)) & (x <= D(hi))]


# ------------------------------------------------------------------------------------------------------------------------------
# the comparison
# ------------------------------------------------------------------------------------------------------------------------------
def worst(got, ref, scale=None):
    """(max over ALL points of |got - ref| / scale, its index).  scale None: |ref|.  Where the scale is 0 the value must be the
    reference's exactly; a value that is not finite where the reference is, or the other way round, is an infinite error.  No
    mean, no mask: one bad point decides."""
    T = np.asarray(ref).dtype.type
    got = np.asarray(got).astype(T).ravel()
    ref = np.asarray(ref).ravel()
    scale = np.abs(ref) if scale is None else np.broadcast_to(np.asarray(scale, dtype=T), np.asarray(ref).shape).ravel()
    assert got.shape == ref.shape == scale.shape
    with np.errstate(all="ignore"):
        err = np.abs(got - ref) / scale
    err = np.where(scale == 0, np.where(got == ref, T(0), T(np.inf)), err)
    same_special = (np.isnan(got) & np.isnan(ref)) | (np.isinf(ref) & (got == ref))
    err = np.where(same_special, T(0), err)
    err = np.where(np.isnan(err), T(np.inf), err)
    i = int(np.argmax(err))
    return float(err[i]), i


def check(name, typ, got, ref, bar, scale=None, at=None):
    """prints the HELPER line and asserts the worst point is within the bar"""
    w, i = worst(got, ref, scale)
    where = "" if at is None else " | at " + ", ".join(f"{k} = {float(np.asarray(v).ravel()[i % np.asarray(v).size]):.17g}" for k, v in at.items())
    print(f"HELPER {name} | {typ} | worst {w:.3e} | bar {bar:.3e}{where}")
    assert w <= bar, (name, typ, w, bar, i)
    return w


def noise(plain, ref, scale=None, floor=None):
    """the worst error of a plain restatement in the working precision against the reference, not below one machine epsilon of
    that precision"""
    w, _ = worst(plain, ref, scale)
    eps = float(np.finfo(np.asarray(plain).dtype).eps) if floor is None else floor
    assert np.isfinite(w), "the plain restatement is not finite where the reference is"
    return max(w, eps)


# ------------------------------------------------------------------------------------------------------------------------------
# trapezoid / compound section (oracle: section_props, conveyance, equivalent_n, dR_dA, dK_dA)
# ------------------------------------------------------------------------------------------------------------------------------
def _p(x, num, den):
    T = x.dtype.type
    with np.errstate(all="ignore"):
        return np.power(x, T(num) / T(den))


def _cast(sec, T):
    return {k: T(v) for k, v in sec.items()}


def general_props(sec, h, T):
    """GeneralProps of the section at depths h (device-typed array), computed in T.  cross_section.py:623-793 through the oracle's
    statement of it, including the over-bank area inconsistency and the frozen n_eq."""
    s = _cast(sec, T)
    h = np.asarray(h).astype(T)
    one, two = T(1), T(2)
    comp = bool(s["compound"] > T(0.5))
    b, m, hb = s["b"], s["m"], s["hbf"]
    d = np.maximum(T(0), h)
    sm = np.sqrt(one + m * m)
    Tw = b + two * m * d
    A = (b + Tw) / two * d
    P = b + two * d * sm
    over = (d > hb) if comp else np.zeros(h.shape, dtype=bool)          # exact inputs: the decision the device takes
    dPdh = np.where(over, two * np.sqrt(one + s["mfp"] ** 2), two * sm)
    with np.errstate(all="ignore"):
        if over.any():
            dfp = d - hb
            Tb = b + two * m * hb
            A_main = (b + Tb) / two * hb
            P_main = b + two * hb * sm
            sfp = np.sqrt(one + s["mfp"] ** 2)
            A_l = (s["bl"] + T(0.5) * s["mfp"] * dfp) * dfp
            P_l = s["bl"] + dfp * sfp
            A_r = (s["br"] + T(0.5) * s["mfp"] * dfp) * dfp
            P_r = s["br"] + dfp * sfp
            A = np.where(over, A_main + A_l + A_r, A)
            P = np.where(over, P_main + P_l + P_r, P)
            Tw = np.where(over, (s["bl"] + Tb + s["br"]) + two * s["mfp"] * dfp, Tw)
        R = np.where(P > 0, A / P, T(0))
        K = A * _p(R, 2, 3) / s["nm"]                                     # hydraulics.py:15-26
        if comp:
            Km = K
            K_l = K_r = np.zeros_like(K)
            if over.any():
                A_m = A_main + Tb * dfp                                    # :694 (column included)
                R_m = np.where(P_main > 0, A_m / P_main, T(0))
                R_l = np.where(P_l > 0, A_l / P_l, T(0))
                R_r = np.where(P_r > 0, A_r / P_r, T(0))
                K_l = np.where(over, A_l * _p(R_l, 2, 3) / s["nl"], T(0))
                K_r = np.where(over, A_r * _p(R_r, 2, 3) / s["nr"], T(0))
                Km = np.where(over, A_m * _p(R_m, 2, 3) / s["nm"], K)
            K = _p(_p(K_l, 3, 2) + _p(Km, 3, 2) + _p(K_r, 3, 2), 2, 3)     # :741-754
        neq = np.full_like(A, s["nm"])
        if comp:
            neq = np.where((A > 0) & (R > 0) & (K > 0), A * _p(R, 2, 3) / K, neq)       # :710-739
        dRdA = np.where((P <= 0) | (Tw <= 0), T(0), (P - A * (dPdh * (one / Tw))) / (P * P))      # :766-790
        dKdA = np.where(A <= 0, T(0), (_p(R, 2, 3) + A * two / T(3) * _p(R, -1, 3) * dRdA) / neq)   # :756-764
        wet = A > 0
        g = dict(A=A, rA=np.where(wet, one / A, T(0)), P=P, Rh=R, T=Tw, rT=one / Tw, K=K, rK=np.where(K > 0, one / K, T(0)), neq=neq,
                 dRdA=dRdA, dKdA=dKdA, dKdA_K=np.where(K > 0, dKdA / K, T(0)), y13=np.where(R > 0, _p(R, -1, 3), T(0)), over=over)
    return g


def props_scales(g):
    """per field: |ref|, and 1 / P for dR/dA (P - A dP/dh / T cancels)"""
    T = g["A"].dtype.type
    return {f: (T(1) / g["P"] if f == "dRdA" else None) for f in PROP_FIELDS}


def sec_derive(sec, T):
    s = _cast(sec, T)
    one, two = T(1), T(2)
    sm = np.sqrt(one + s["m"] ** 2)
    Tb = s["b"] + two * s["m"] * s["hbf"]
    pm15 = lambda n: one / (n * np.sqrt(n)) if n > 0 else T(0)
    return dict(sm=sm, sfp=np.sqrt(one + s["mfp"] ** 2), Tb=Tb, Am=(s["b"] + Tb) / two * s["hbf"], Pm=s["b"] + two * s["hbf"] * sm,
                rnm=one / s["nm"], km15=pm15(s["nm"]), kl15=pm15(s["nl"]), kr15=pm15(s["nr"]))


def node_terms(sec, h, Q, T):
    """NodeTerms of the general path (oracle node_terms), eAT in the reference's mixed convention (friction part per unit area,
    curvature part times dA/dh), eQ = dSe/dQ itself.  Returns (fields, scales): a scale of None is |ref|; Se, eAT and eQ take the sum
    of the magnitudes of their addends (friction and curvature parts can cancel for Q < 0), which without curvature is |Se|, |Se / A|
    times the factor of dK/dA, and |dSe/dQ|."""
    g = general_props(sec, h, T)
    s = _cast(sec, T)
    h = np.asarray(h).astype(T)
    Q = np.asarray(Q).astype(T)
    gr = T(G)
    A, Tw, R, K, neq, dRdA = g["A"], g["T"], g["Rh"], g["K"], g["neq"], g["dRdA"]
    with np.errstate(all="ignore"):
        Sf = Q * np.abs(Q) / K ** 2                                        # hydraulics.py:57
        dSfA = T(-2) * Sf * (g["dKdA"] / K)                                # :75
        dSfQ = T(2) * np.abs(Q) / K ** 2                                   # :92
        Se, eAT, eQ = Sf, dSfA, dSfQ
        mSe, mAT, mQ = np.abs(Sf), np.abs(Sf / A), np.abs(dSfQ)           # the scales
        curv = s["curv"]
        if curv != 0:
            rc = T(1) / curv
            V = Q / np.maximum(A, T(1e-6))
            Dh = A / np.maximum(Tw, T(1e-6))
            Fr = V / np.sqrt(gr * np.maximum(Dh, T(1e-6)))                  # hydraulics.py:155-168
            C = _p(R, 1, 6) / neq
            f = T(8) * gr / C ** 2                                          # :227-229
            sq = np.sqrt(f)
            poly = T(2.86) * sq + T(2.07) * f
            num = poly * h ** 2 * Fr ** 2
            den = (T(0.565) + sq) * rc ** 2
            Sc = num / den                                                  # :94-117
            Se = Sf + Sc
            mSe = np.abs(Sf) + np.abs(Sc)
            mAT = mSe / A
            if abs(curv) > T(1e-12):
                Vr = Q / A
                Dr = A / Tw
                gD = gr * Dr
                a1 = T(-0.5) * Vr * gD ** T(-1.5) * gr * (T(1) / Tw)
                a2 = (-Q / A ** 2) * gD ** T(-0.5)
                dFrA = a1 + a2
                dfA = -(T(8) / T(3)) * gr * neq ** 2 * _p(R, -4, 3) * dRdA
                t1 = (T(2.86) / (T(2) * sq) * dfA + T(2.07) * dfA) * h ** 2 * Fr ** 2
                t2 = poly * (T(2) * h * (T(1) / Tw) * Fr ** 2)
                t3 = poly * (h ** 2 * T(2) * Fr * dFrA)
                dnum = t1 + t2 + t3
                dden = (T(1) / (T(2) * sq) * dfA) * rc ** 2
                eAT = dSfA + (dnum * den - num * dden) / den ** 2 * Tw      # :119-137, x dA_dh (cross_section.py:164)
                mAT = mAT + ((np.abs(t1) + np.abs(t2) + np.abs(t3)) * den + np.abs(num * dden)) / den ** 2 * Tw
                dFrQ = (T(1) / A) * gD ** T(-0.5)
                dScQ = (poly * h ** 2 * T(2) * Fr * dFrQ * den) / den ** 2   # :139-153
                eQ = dSfQ + dScQ
                mQ = np.abs(dSfQ) + np.abs(dScQ)
        out = dict(A=A, T=Tw, Se=Se, eAT=eAT, eQ=eQ, v=Q / A, rT=T(1) / Tw)
    scales = dict(A=None, T=None, Se=mSe, eAT=mAT, eQ=mQ, v=None, rT=None)
    return out, scales


# ------------------------------------------------------------------------------------------------------------------------------
# boundary rows (oracle: boundary_eval, rating_discharge, rating_dQ_dz - restated: boundary_eval forces float())
# ------------------------------------------------------------------------------------------------------------------------------
def blend_alpha_branch(z, s0, buf):
    """0 below the buffer, 1 above, 2 inside: decided in the type of z (the device's), as the device decides"""
    return np.where(z >= s0 + buf, 1, np.where(z <= s0, 0, 2))


def rating_blend(z, p, T, branch=None):
    """(q, al) of the blended curve at the device-typed stages z; p: s0, buf, l0, l1, l2, h0, h1, h2 (device-typed)"""
    D = np.asarray(z).dtype.type
    br = blend_alpha_branch(np.asarray(z), D(p[0]), D(p[1])) if branch is None else branch
    zz = np.asarray(z).astype(T)
    q = [T(v) for v in p]
    s = (zz - q[0]) / q[1]
    al = np.where(br == 1, T(1), np.where(br == 0, T(0), T(3) * s ** 2 - T(2) * s ** 3))
    lo = q[2] + q[3] * zz + q[4] * zz * zz
    hi = q[5] + q[6] * zz + q[7] * zz * zz
    return (T(1) - al) * lo + al * hi, al


def bc_row(kind, params, sec, level, dt, h, Q, Qold, Yprev, tgt, T):
    """One boundary row at device-typed inputs, computed in T.  Returns a dict: res, dh, dq, Ynew (T arrays), flag (int), the scales
    s_res / s_dh / s_Y of section 4 of the test's docstring, and `exact`: the names whose value the device must hit bit for bit
    (then res / dh / dq hold the device-typed value)."""
    D = np.asarray(h).dtype.type
    n = len(h)
    p = [T(v) for v in params]
    hh, QQ = np.asarray(h).astype(T), np.asarray(Q).astype(T)
    one, zero = np.full(n, T(1)), np.full(n, T(0))
    out = dict(Ynew=zero, flag=np.zeros(n, dtype=np.int32), s_Y=None, s_dh=None, exact=["dq", "flag"])
    if kind == KINDS["flow"]:
        t = np.asarray(tgt).astype(T)
        out.update(res=QQ - t, dh=zero, dq=one, s_res=np.maximum(np.abs(QQ), np.abs(t)))
        out["exact"] += ["dh"]
    elif kind in (KINDS["stage"], KINDS["fixed"]):
        depth = (np.asarray(tgt).astype(T) - p[0]) if kind == KINDS["stage"] else np.full(n, p[0])
        out.update(res=hh - depth, dh=one, dq=zero, s_res=np.maximum(np.abs(hh), np.abs(depth)))
        out["exact"] += ["dh"]
    elif kind == KINDS["normal"]:
        S0, bed = p[0], p[1]
        sg = T(-1) if S0 < 0 else T(1)
        rt = np.sqrt(abs(S0))
        gr_ = general_props(sec, h, T)                                     # residual: hw = z_min + h
        hd = (np.asarray(h) + D(params[1])) - D(sec["z"])                  # df_dh: hw = h + bed_level, at the depth the device forms
        gd = general_props(sec, hd, T)
        q = sg * gr_["K"] * rt                                             # hydraulics.py:4-13
        out.update(res=QQ - q, dh=T(0) - sg * gd["dKdA"] * rt * gd["T"], dq=one, s_res=np.maximum(np.abs(QQ), np.abs(q)))
    elif kind == KINDS["power"]:
        # (run in float32 this is the plain restatement of the fp32 row, whose x^b is documented as exp2(b log2 x): pow_plain_f32,
        # the same restatement the scalar pow_pos(float) is held to)
        pw = pow_plain_f32 if T is np.float32 else pow_ref
        x = p[3] + hh + p[2]
        q = p[0] * pw(x, p[1])                                             # rating_curve.py:59
        out.update(res=QQ - q, dh=T(0) - p[0] * p[1] * pw(x, p[1] - T(1)), dq=one, s_res=np.maximum(np.abs(QQ), np.abs(q)))
    elif kind == KINDS["poly"]:
        x = p[4] + hh + p[3]
        q = p[0] * x ** 2 + p[1] * x + p[2]
        out.update(res=QQ - q, dh=T(0) - (p[0] * T(2) * x + p[1]), dq=one, s_res=np.maximum(np.abs(QQ), np.abs(q)))
    elif kind == KINDS["blend"]:
        # the stage and its two neighbours as the device forms them (z = bed + h, z +- dY in its type), each on its own side of the
        # buffer edges; the curve at those stages in T
        z = D(params[9]) + np.asarray(h)
        dY = D(params[8])
        q0, _ = rating_blend(z, params[:8], T)
        qp, _ = rating_blend(z + dY, params[:8], T)
        qm, _ = rating_blend(z - dY, params[:8], T)
        # dh is a central difference: its two addends q(z + dY) / (2 dY) and q(z - dY) / (2 dY) cancel, their magnitudes are the scale
        out.update(res=QQ - q0, dh=T(0) - (qp - qm) / (T(2) * T(dY)), dq=one, s_res=np.maximum(np.abs(QQ), np.abs(q0)),
                   s_dh=(np.abs(qp) + np.abs(qm)) / (T(2) * T(dY)))
    elif kind == KINDS["storage"]:
        # the stage in the device's arithmetic decides the range flag, the floor and dq; the value is computed in T
        hD, QD, QoD, YpD = (np.asarray(v) for v in (h, Q, Qold, Yprev))
        area, ymin, lo, hi, bed = (D(v) for v in params[:5])
        with np.errstate(all="ignore"):
            Yd = (hD + bed if level == 1 else YpD) + D(0.5) * (QoD + QD) * D(dt) / area       # boundary.py:104-108 (k == 1 quirk)
            flag = np.where((Yd >= lo) & (Yd <= hi), FS_OK, FS_STORAGE_RANGE).astype(np.int32)
            floored = Yd < ymin
            dq_dev = D(0) - np.where(np.where(floored, ymin, Yd) <= ymin, D(0), D(1) / area) * D(0.5) * D(dt)
        Yold = (hh + p[4]) if level == 1 else np.asarray(Yprev).astype(T)
        add = T(0.5) * (np.asarray(Qold).astype(T) + QQ) * T(dt) / p[0]
        Y = np.where(floored, p[1], Yold + add)
        out.update(res=hh - (Y - p[4]), dh=one, dq=dq_dev.astype(T), Ynew=Y, flag=flag,
                   s_res=np.maximum(np.abs(hh), np.abs(Y - p[4])),
                   s_Y=np.where(floored, np.abs(p[1]), np.abs(Yold) + np.abs(add)))
        out["exact"] += ["dh"]
    else:
        raise KeyError(kind)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# the general reservoir row (oracle: storage_area_at, storage_net_vol, storage_outflow, the f of storage_mass_balance and the
# general-storage branch of boundary_eval) on one FS_BC_STORAGE_CURVE parameter block: the FS_SC_* scalars, stage[n_curve],
# area[n_curve]
# ------------------------------------------------------------------------------------------------------------------------------
KINDS.update(storage_curve=8, host_row=9)
SC_KEYS = ("min_stage", "Y_min", "Y_max", "bed", "area", "alpha", "beta", "n_curve", "rc_type", "rc_a", "rc_b", "rc_c", "rc_shift",
           "losses", "length", "K_q")                                                            # the FS_SC_* slots, in order
SC = {k: i for i, k in enumerate(SC_KEYS)}
SC_NFIXED = len(SC_KEYS)
BRENT_XTOL, BRENT_RTOL = 2e-12, 8.881784197001252e-16        # scipy.optimize.brentq's defaults, as storage_root states them


def sc_params(D, curve=None, rc=None, losses=None, **kw):
    """the parameter block in the device type.  curve: [[stage, area], ...]; rc: dict(type="power" | "polynomial", a, b, c, shift);
    losses: dict(reservoir_length, K_q)"""
    s = dict.fromkeys(SC_KEYS, 0.0)
    s.update(alpha=1.0)
    s.update(kw)
    curve = np.zeros((0, 2)) if curve is None else np.asarray(curve, dtype=np.float64)
    s["n_curve"] = len(curve)
    if rc is not None:
        s.update(rc_type={"power": 1, "polynomial": 2}[rc["type"]], rc_a=rc["a"], rc_b=rc["b"], rc_c=rc.get("c", 0.0), rc_shift=rc.get("shift", 0.0))
    if losses is not None:
        s.update(losses=1.0, length=losses["reservoir_length"], K_q=losses["K_q"])
    return np.concatenate([[s[k] for k in SC_KEYS], curve[:, 0], curve[:, 1]]).astype(D)


def sc_curve(p):
    nc = int(p[SC["n_curve"]])
    return p[SC_NFIXED:SC_NFIXED + nc], p[SC_NFIXED + nc:SC_NFIXED + 2 * nc]


def sc_oracle_st(p):
    """the block as the `storage` dict of oracle/preissmann_oracle.py (every value the float of the device-typed parameter)"""
    f = lambda k: float(p[SC[k]])
    xs, ys = sc_curve(p)
    st = dict(area=f("area"), min_stage=f("min_stage"), Y_min=f("Y_min"), Y_max=f("Y_max"), alpha=f("alpha"), beta=f("beta"))
    if len(xs):
        st["curve"] = np.stack([xs.astype(np.float64), ys.astype(np.float64)], axis=1)
    t = int(p[SC["rc_type"]])
    if t:
        st["rc"] = dict(type="polynomial" if t == 2 else "power", a=f("rc_a"), b=f("rc_b"), c=f("rc_c"), shift=f("rc_shift"))
    if f("losses") > 0.5:
        st["losses"] = dict(reservoir_length=f("length"), K_q=f("K_q"))
    return st


def sc_step(p):
    """the smallest gap of the curve's stages in the device type, as bc_storage_curve forms it (1 without two breakpoints)"""
    xs, _ = sc_curve(p)
    return np.min(np.abs(xs[1:] - xs[:-1])) if len(xs) > 1 else p.dtype.type(1)


def sc_area_branch(p, Y):
    """-1 clamped below, -2 clamped above, else the interpolation interval: decided in the type of Y (the device's for a
    device-typed stage) from Y + beta as that type rounds it"""
    xs, _ = sc_curve(p)
    B = np.asarray(Y).dtype.type
    x = np.asarray(Y) + B(p[SC["beta"]])
    xb = xs.astype(B)
    j = np.clip(np.searchsorted(xb, x, side="right") - 1, 0, max(len(xs) - 2, 0))
    return np.where(x <= xb[0], -1, np.where(x >= xb[-1], -2, j))


def sc_area_at(p, Y, T):
    """alpha * interp(Y + beta) in T; without a curve the constant area.  Y: stages of the device type, or of T (then the interval is
    the one the T value lies in)"""
    Y = np.asarray(Y)
    xs, ys = sc_curve(p)
    if len(xs) == 0:
        return np.full(Y.shape, T(p[SC["area"]]))
    br = sc_area_branch(p, Y)
    xs, ys = xs.astype(T), ys.astype(T)
    x = Y.astype(T) + T(p[SC["beta"]])
    j = np.maximum(br, 0)
    if len(xs) > 1:
        a = (ys[j + 1] - ys[j]) / (xs[j + 1] - xs[j]) * (x - xs[j]) + ys[j]
    else:
        a = np.full(Y.shape, ys[0])
    a = np.where(br == -1, ys[0], np.where(br == -2, ys[-1], a))
    return T(p[SC["alpha"]]) * a


def sc_trapezoid_n(p, Y1, Y2):
    """(int)(|Y2 - Y1| / step) in the device type (0 where the quotient is no number, as the device's conversion gives)"""
    with np.errstate(all="ignore"):
        q = np.abs(np.asarray(Y2) - np.asarray(Y1)) / sc_step(p)
    return np.where(np.isfinite(q), q, 0).astype(np.int64)


def sc_net_vol(p, Y1, Y2, T, n=None):
    """(volume between Y1 and Y2, sum of the magnitudes of its terms).  n: the trapezoid's point count per element, by default
    decided in the device type from the device-typed Y1, Y2"""
    Y1, Y2 = np.asarray(Y1), np.asarray(Y2)
    if int(p[SC["n_curve"]]) == 0:
        v = (Y2.astype(T) - Y1.astype(T)) * T(p[SC["area"]])
        return v, np.abs(v)
    n = sc_trapezoid_n(p, Y1, Y2) if n is None else np.asarray(n)
    y1, y2 = Y1.astype(T), Y2.astype(T)
    a1 = sc_area_at(p, Y1, T)
    v = T(0.5) * (sc_area_at(p, Y2, T) + a1) * (y2 - y1)
    mag = np.abs(v)
    for k in np.unique(n[n > 2]):
        m = n == k
        lo, hi = y1[m], y2[m]
        d = (hi - lo) / T(k - 1)
        s, sm, y0, a0 = np.zeros_like(lo), np.zeros_like(lo), lo, a1[m]
        for i in range(1, int(k)):
            yy = hi if i == k - 1 else lo + T(i) * d
            aa = sc_area_at(p, yy, T)
            t = (yy - y0) * (aa + a0) / T(2)
            s, sm, y0, a0 = s + t, sm + np.abs(t), yy, aa
        v[m], mag[m] = s, sm
    return v, mag


def sc_outflow(p, Y, T):
    """(reservoir release at stage Y, sum of the magnitudes of its terms)"""
    Y = np.asarray(Y)
    t = int(p[SC["rc_type"]])
    if t == 0:
        return np.zeros(Y.shape, dtype=T), np.zeros(Y.shape, dtype=T)
    a, b, c = (T(p[SC[k]]) for k in ("rc_a", "rc_b", "rc_c"))
    x = Y.astype(T) + T(p[SC["rc_shift"]])
    if t == 2:
        return a * x * x + b * x + c, np.abs(a * x * x) + np.abs(b * x) + abs(c)
    q = a * (pow_plain_f32 if T is np.float32 else pow_ref)(x, np.full(Y.shape, b))     # (fp32: exp2(b log2 x), as the power row)
    return q, np.abs(q)


def sc_f(p, Yold, vol, dt, Y, T, n=None):
    """(the mass balance whose root storage_root finds, sum of the magnitudes of its terms).  lumped_storage.py:24-31"""
    v, mag = sc_net_vol(p, Yold, Y, T, n)
    vol = np.asarray(vol).astype(T)
    if int(p[SC["rc_type"]]) != 0:
        (q0, m0), (q1, m1) = sc_outflow(p, Yold, T), sc_outflow(p, Y, T)
        qout, mq = T(0.5) * (q0 + q1), T(0.5) * (m0 + m1)
    else:
        qout = mq = np.zeros(v.shape, dtype=T)
    return v - (vol - qout * T(dt)), mag + np.abs(vol) + mq * T(dt)


def brent_delta(Y):
    """Brent's (xtol + rtol |x|) / 2 in the type of Y"""
    D = np.asarray(Y).dtype.type
    return (D(BRENT_XTOL) + D(BRENT_RTOL) * np.abs(Y)) / D(2)


def sc_min_slope(p):
    """the smallest dV/dY in the bracket: alpha times the smallest area of the curve (the rating term only adds to it)"""
    _, ys = sc_curve(p)
    return float(p[SC["alpha"]]) * float(ys.min()) if len(ys) else float(p[SC["area"]])


def sc_row(params, sec, level, dt, h, Q, Qold, Y, T):
    """The general reservoir row AT the stage Y (device-typed: the stage the root finder returned, after the floor), computed in T.
    boundary.py:97-133, :152-164, :213-237.  Returns res, dh, dq, their scales, and `exact`: name -> (mask, device-typed values) of what
    the device must hit bit for bit."""
    D = np.asarray(h).dtype.type
    p = params
    n = len(h)
    hh, QQ, YY = np.asarray(h).astype(T), np.asarray(Q).astype(T), np.asarray(Y).astype(T)
    bed, ymin = T(p[SC["bed"]]), D(p[SC["min_stage"]])
    floored = np.asarray(Y) <= ymin                                         # lumped_storage.py:37-45, decided on the device's own stage
    with np.errstate(all="ignore"):
        dY = np.where(floored, T(0), T(1) / sc_area_at(p, Y, T))
    hl = t1 = t2 = u1 = u2 = dAdh = np.zeros(n, dtype=T)
    losses = bool(p[SC["losses"]] > D(0.5))
    if losses:
        Lr, Kq, gr = T(p[SC["length"]]), T(p[SC["K_q"]]), T(G)
        aQ = np.abs(QQ)
        gr_ = general_props(sec, h, T)                                      # residual: hw = z_min + depth
        hd = (np.asarray(h) + D(p[SC["bed"]])) - D(sec["z"])                # derivatives: hw = depth + bed_level, as the device forms it
        gd = general_props(sec, hd, T)
        with np.errstate(all="ignore"):
            K = gr_["A"] * _p(gr_["Rh"], 2, 3) / gr_["neq"]
            hl = QQ * aQ / K ** 2 * Lr + Kq * (QQ / gr_["A"]) ** 2 / (T(2) * gr)
            A, R, ne = gd["A"], gd["Rh"], gd["neq"]
            K = A * _p(R, 2, 3) / ne
            dK = (_p(R, 2, 3) + A * T(2) / T(3) * _p(R, -1, 3) * gd["dRdA"]) / ne           # hydraulics.py:28-40
            V = QQ / A
            t1 = T(-2) * (QQ * aQ / K ** 2) * (dK / K) * Lr
            t2 = Kq * T(2) * V * (-QQ / A ** 2) / (T(2) * gr)
            u1 = T(2) * aQ / K ** 2 * Lr
            u2 = Kq * T(2) * V * (T(1) / A) / (T(2) * gr)
            dAdh = gd["T"]
    half_dt = T(0.5) * T(dt)
    out = dict(res=hh - (YY + hl - bed), dh=T(1) - (t1 + t2) * dAdh, dq=T(0) - (dY * half_dt + (u1 + u2)),
               s_res=np.maximum(np.abs(hh), np.abs(YY) + np.abs(hl)), s_dh=T(1) + (np.abs(t1) + np.abs(t2)) * dAdh,
               s_dq=dY * half_dt + np.abs(u1) + np.abs(u2), floored=floored, exact={})
    if not losses:
        out["exact"]["dh"] = (np.ones(n, dtype=bool), np.ones(n, dtype=D))
        out["exact"]["dq"] = (floored, np.zeros(n, dtype=D))               # dY = 0 at or below min_stage
    return out
