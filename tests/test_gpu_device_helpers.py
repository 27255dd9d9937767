"""The device math helpers, node terms and boundary rows of flow-sim_amd/csrc/fs_device.hpp on the GPU, one by one, through the probe
library (tests/device_probe/probe.hip -> libfs_probe.so, compiled with the library's flags) against the high-precision restatement of
tests/helper_reference.py on the cases and bars of tests/helper_recipes.py (both checked on the CPU by tests/test_helper_reference.py).

Errors are relative, |got - ref| / scale, the worst over ALL points; scale = |ref| unless the output can cancel (helper_reference:
node_terms, bc_row, props_scales).  Where each bar comes from: the docstring of tests/helper_recipes.py; none was taken from a device
run.  One line per function and type is printed (run with -s):  HELPER name | type | worst | bar | at x = ...

Measured on an MI355X (worst | bar); the composites as the worst of all their parameter sets and fields, relative to its bar:

  helper        fp64 worst   bar                    fp32 worst   bar
  frcp          2.11e-15     2.3e-15  stated        8.98e-08     1.19e-07 stated (1 ulp = 2^-23)
  frsq          1.67e-16     8.88e-16 4 x noise     7.35e-08     4.77e-07 4 x noise
  rcbrt_pos     1.28e-16     8.88e-16 4 x noise     8.55e-08     7.34e-07 4 x noise
  rcbrt2_pos    1.60e-16     1.51e-15 4 x noise     1.02e-07     1.52e-06 4 x noise
  fsqrt_pos     2.13e-16     2e-15    stated        1.04e-07     4.77e-07 4 x noise
  p23_          2.06e-16     1.32e-15 4 x noise     1.19e-07     1.40e-06 4 x noise
  p32_          3.00e-16     8.88e-16 4 x noise     1.43e-07     4.77e-07 4 x noise
  pm15_         5.85e-16     1.06e-15 4 x noise     3.09e-07     5.70e-07 4 x noise
  k15_          5.00e-16     1.19e-15 4 x noise     2.35e-07     8.08e-07 4 x noise
  log_pos       2.95e-16     4e-16    stated        -
  exp_short     3.48e-16     8.88e-16 4 x noise     -
  pow_pos       4.04e-15     5.05e-15 = 1.25 x 4.04e-15 of float64 exp(b log x) on the same points
  pow_pos, pow_ (fp32), x 1e-4 .. 1e4, b 0.2 .. 5   5.25e-06     1.58e-05 4 x noise
  pow_pos, pow_ (fp32), x 0.1 .. 100, b 0.5 .. 3    1.58e-06     4.52e-06 4 x noise

  composite            fp64 worst (bar 1e-12)               fp32 worst | its bar (4 x noise of that output and set)
  node_terms_rect      1.43e-14  eAT, rect_2km              2.16e-07 | 4.77e-07  v, rect_2km
  node_terms_trap      9.89e-15  eAT, trap_5m_m0.5          2.99e-07 | 6.36e-07  v, trap_2km_m2.5
  node_terms_general   1.93e-14  eAT, trap_5m_m0.5          2.30e-07 | 4.77e-07  rT, compound_curv_1e-3
  general_props        5.09e-15  dKdA, rect_2km             4.77e-07 | 5.54e-07  dRdA, rect_2km
  sec_derive           3.29e-16  kr15                       1.44e-07 | 4.77e-07  kr15
  rating_blend<true>   3.44e-16  al, buffer 0.3             2.09e-07 | 1.07e-06  al, buffer 0.3
  rating_blend<false>  3.44e-16  al, buffer 0.3             1.64e-07 | 6.14e-07  q, buffer 0.3
  bc_eval<false>       3.40e-15  dh, normal depth 0.3 off   6.58e-07 | 9.95e-07  dh, power rating
  bc_eval_rect         3.69e-15  dh, normal depth same bed  3.47e-07 | 7.76e-07  dh, normal depth S0 < 0

The general reservoir row (FS_BC_STORAGE_CURVE: seven parameter sets, helper_recipes.sc_sets) and the host row:

  area_at              4.08e-16  curve6_alpha_beta_poly     2.38e-07 | 9.51e-07  curve6_alpha_beta_poly
  outflow              6.04e-16  curve6_power_shift         1.38e-06 | 1.47e-06  curve6_power_shift (exp2(b log2 x), as the power row)
  net_vol              3.55e-16  curve6_alpha_beta_poly     1.64e-07 | 6.43e-07  curve6
  bc_eval<true>.res    2.94e-15  curve6_poly_losses_bed_off 6.91e-07 | 4.30e-06  curve6_poly_losses_bed_off
  bc_eval<true>.dh     1.58e-15  curve6_poly_losses_bed_off 7.13e-07 | 4.81e-06  curve6_poly_losses_bed_off
  bc_eval<true>.dq     1.98e-15  curve6_poly_losses_bed_off 1.21e-07 | 4.77e-07  curve6
  storage_root         the wide f changes sign within w = 4 x (max(delta, ulp) + noise_f / A_min) of the returned stage, or is 0 there, at
                       every root point away from a switch of the trapezoid's n (3 512 of 3 519 points per type; bc_eval<true>'s Ynew: 3 257 / 3 256).
                       Worst multiple of w / 4 needed on the device, of 1, 2, 4: fp64 1, fp32 1 (bar 4).
  storage_root, fp64   |Y - brentq's root| <= 0.004 x 2 delta on every set (bar 10 x 2 delta: two valid evaluation paths end at most
                       2 delta apart, tests/test_gpu_forcing.py)

The row is compared AT the stage the device returned (res, dh, dq do not inherit the root's tolerance).  Bit for bit the same: flag
(FS_STORAGE_RANGE for f of one sign at both ends and for a NaN volume), the bracket end where f(end) == 0, Ynew == min_stage on the
floor, dq == 0 there and dh == 1 without entrance losses, area_at on the clamped ends and with a constant area, outflow without a
rating curve, net_vol(Y, Y) == 0, the shared and the per-reach parameter layout, and dh, dq, res of the host row (NaN, inf included).
The rows' numbers on flagged points are not promised and not compared.

dq, dh of the stage-type rows, flag, and al outside the blend buffer (both forms, the edge stages included): bit for bit the same.
Every stated bound held: no comment had to be corrected.  pow_pos: the source's 4.1e-15 stands (4.04e-15 here, the float64 libm
pair 4.04e-15 on the same points); the 8.0e-15 of profiles/round4/rsq_pow_prec.txt is that benchmark's own grid, where host libm gives 7.95e-15.
"""
import numpy as np
import pytest

import helper_recipes as RC
import helper_reference as HR

pytestmark = pytest.mark.gpu
TYPS = ["f64", "f32"]


@pytest.fixture(scope="module")
def P():
    import device_probe
    device_probe.lib()            # RuntimeError "probe library not built" fails the tests: no skip
    return device_probe


class Tally:
    """every line is printed before the first failure is raised"""
    def __init__(self):
        self.failed = []

    def check(self, *a, **kw):
        try:
            HR.check(*a, **kw)
        except AssertionError as e:
            self.failed.append(str(e))

    def same_bits(self, name, typ, got, want):
        D = got.dtype
        ok = np.asarray(want).astype(D).tobytes() == np.ascontiguousarray(got).tobytes()
        print(f"HELPER {name} | {typ} | bit for bit | {'same' if ok else 'DIFFERENT'}")
        if not ok:
            bad = np.nonzero(np.asarray(want).astype(D) != got)[0]
            self.failed.append(f"{name} {typ}: {len(bad)} values differ, first at {bad[:4].tolist()}")

    def done(self):
        assert not self.failed, self.failed


# ------------------------------------------------------------------------------------------------------------------------------
# scalar helpers
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("typ", TYPS)
def test_scalar_helpers(P, typ):
    t = Tally()
    for c in RC.scalar_cases(typ):
        kind, code = c["call"]
        got = P.unary(code, *c["x"]) if kind == "unary" else (P.power(code, *c["x"]) if kind == "pow" else P.k15(*c["x"]))
        at = dict(zip(("x", "b", "n15") if kind != "k15" else ("A", "P", "n15"), c["x"]))
        if "pair" in c:
            print(f"HELPER pow_pos | {typ} | float64 exp(b log x) on the same points: {c['pair']:.3e}")
        t.check(c["name"], typ, got, c["ref"], c["bar"], at=at)
    t.done()


@pytest.mark.parametrize("typ", TYPS)
def test_documented_special_values(P, typ):
    D = RC.TYPES[typ]
    b = np.array([0.2, 0.5, 1.0, 1.6, 3.0, 5.0], dtype=D)
    for which in ((0,) if typ == "f64" else (0, 1)):                      # pow_(double) is libm's: not a helper of this file
        assert np.all(P.power(which, np.zeros_like(b), b) == 0), "x = 0"
        assert np.all(np.isnan(P.power(which, np.array([-1e-4, -0.5, -1.0, -2.0, -64.0, -1e4], dtype=D), b))), "x < 0"
    zero = np.zeros(1, dtype=D)
    assert P.unary(HR.UNARY_OPS.index("p23_"), zero)[0] == 0 and P.unary(HR.UNARY_OPS.index("p32_"), zero)[0] == 0
    A = np.array([0.0, 3.0, 0.0, 3.0], dtype=D)
    Pw = np.array([2.0, 0.0, 0.0, 2.0], dtype=D)
    k = P.k15(A, Pw, np.full(4, 100.0, dtype=D))
    assert np.all(k[:3] == 0) and k[3] > 0


# ------------------------------------------------------------------------------------------------------------------------------
# node terms
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("typ", TYPS)
def test_node_terms(P, typ):
    """node_terms_rect / _trap / _general against the general path's reference on the same section; eQh times the family's kEQScale"""
    t = Tally()
    for c in RC.node_cases(typ):
        at = dict(h=c["h"], Q=c["Q"])
        for form in c["forms"]:
            got = P.node_terms(RC.FORM_CODE[form], c["sec"], c["h"], c["Q"])
            got["eQ"] = got.pop("eQh") * got["A"].dtype.type(RC.K_EQ_SCALE[form])
            for f in HR.NODE_FIELDS:
                t.check(f"node_terms_{form}.{f} [{c['name']}]", typ, got[f], c["ref"][f], c["bar"][f], scale=c["scale"][f], at=at)
    t.done()


@pytest.mark.parametrize("typ", TYPS)
def test_general_props(P, typ):
    t = Tally()
    for c in RC.node_cases(typ):
        got = P.general_props(c["sec"], c["h"])
        pr = c["props"]
        for f in HR.PROP_FIELDS:
            t.check(f"general_props.{f} [{c['name']}]", typ, got[f], pr["ref"][f], pr["bar"][f], scale=pr["scale"][f], at=dict(h=c["h"]))
    t.done()


@pytest.mark.parametrize("typ", TYPS)
def test_sec_derive(P, typ):
    D = RC.TYPES[typ]
    T = HR.reference_type(D)
    secs = [c["sec"] for c in RC.node_cases(typ)]
    got = P.sec_derive(secs, D)
    t = Tally()
    for f in HR.DERIVE_FIELDS:
        ref = np.array([HR.sec_derive(s, T)[f] for s in secs], dtype=T)
        bar = RC.COMPOSITE_F64 if typ == "f64" else RC.FACTOR * HR.noise(np.array([HR.sec_derive(s, D)[f] for s in secs], dtype=D), ref)
        t.check(f"sec_derive.{f}", typ, got[f], ref, bar)
    t.done()


@pytest.mark.parametrize("typ", TYPS)
def test_a_dry_node_keeps_what_the_source_promises(P, typ):
    """h <= 0 (the oracle divides by zero there): general_props gives a dry node rA = 0 and finite fields, and the friction slope
    of node_terms_general is 0 (sections without curvature: the curvature slope of a dry node is no number in the reference either)"""
    D = RC.TYPES[typ]
    h = np.array([0.0, -0.0, -1e-3, -0.5, -60.0], dtype=D)
    Q = np.array([25.0, -25.0, 0.0, 1e4, -1e-2], dtype=D)
    for name, kw, _ in RC.SECTIONS:
        if kw.get("curv", 0.0) != 0.0:
            continue
        sec = HR.section(D, **kw)
        g = P.general_props(sec, h)
        assert all(np.all(np.isfinite(g[f])) for f in HR.PROP_FIELDS), name
        assert np.all(g["rA"] == 0) and np.all(g["A"] == 0) and np.all(g["K"] == 0), name
        nt = P.node_terms(RC.FORM_CODE["general"], sec, h, Q)
        assert all(np.all(np.isfinite(v)) for v in nt.values()), name
        assert np.all(nt["Se"] == 0) and np.all(nt["v"] == 0), name


# ------------------------------------------------------------------------------------------------------------------------------
# boundary rows
# ------------------------------------------------------------------------------------------------------------------------------
def blend_stages(case):
    D = case["params"].dtype.type
    return (D(case["params"][9]) + case["pts"][0]).astype(D)


@pytest.mark.parametrize("typ", TYPS)
def test_rating_blend_both_forms(P, typ):
    """rating_blend<true> (reciprocal, clamped) and <false> (branching) at the stages of the blended boundary rows: the curve, and -
    through a curve whose low branch is 0 and whose high branch is 1, which makes the result the weight itself - al == 0 and al == 1
    bit for bit outside the buffer"""
    D = RC.TYPES[typ]
    T = HR.reference_type(D)
    t = Tally()
    for c in RC.bc_cases(typ):
        if c["kind"] != HR.KINDS["blend"] or c["form"] != "general":
            continue
        z = blend_stages(c)
        z = np.concatenate([z, z + D(c["params"][8]), z - D(c["params"][8])]).astype(D)
        p = c["params"][:8]
        weight = np.array([p[0], p[1], 0, 0, 0, 1, 0, 0], dtype=D)
        ref, _ = HR.rating_blend(z, p, T)
        _, al = HR.rating_blend(z, weight, T)
        br = HR.blend_alpha_branch(z, D(p[0]), D(p[1]))
        assert (br == 0).sum() > 9 and (br == 1).sum() > 9 and (br == 2).sum() > 9
        if typ == "f64":
            bar = bar_al = RC.COMPOSITE_F64
        else:
            bar = RC.FACTOR * HR.noise(HR.rating_blend(z, p, D)[0], ref)
            bar_al = RC.FACTOR * HR.noise(HR.rating_blend(z, weight, D)[1], al)
        for rcp in (1, 0):
            name = f"rating_blend<{'true' if rcp else 'false'}>"
            t.check(f"{name} [{c['name']}]", typ, P.rating_blend(rcp, p, z), ref, bar, at=dict(z=z))
            got_al = P.rating_blend(rcp, weight, z)
            t.check(f"{name}.al [{c['name']}]", typ, got_al, al, bar_al, at=dict(z=z))
            t.same_bits(f"{name}.al outside the buffer [{c['name']}]", typ, got_al[br != 2], al[br != 2])
    t.done()


@pytest.mark.parametrize("typ", TYPS)
def test_boundary_rows(P, typ):
    """bc_eval<false> on a compound section and bc_eval_rect, one launch per parameter set"""
    t = Tally()
    for c in RC.bc_cases(typ):
        form = 0 if c["form"] == "general" else 1
        got = P.bc(form, c["kind"], c["params"], c["sec"], c["level"], c["dt"], *c["pts"])
        ref = c["ref"]
        name = f"bc_eval{'<false>' if form == 0 else '_rect'} [{c['name']}]"
        at = dict(h=c["pts"][0], Q=c["pts"][1])
        for f, bar in c["bar"].items():
            t.check(f"{name}.{f}", typ, got[f], ref[f], bar, scale=c["scales"][f], at=at)
        for f in ref["exact"]:
            t.same_bits(f"{name}.{f}", typ, got[f], ref[f])
    t.done()


# ------------------------------------------------------------------------------------------------------------------------------
# the general reservoir row (FS_BC_STORAGE_CURVE): its parts, its Brent root, the row at the device's own stage; the host row
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("typ", TYPS)
def test_storage_curve_parts(P, typ):
    """StorageCurve::area_at, outflow and net_vol on every parameter set; bit for bit: the clamped ends, a constant area, no rating
    curve, net_vol(Y, Y) == 0"""
    D = RC.TYPES[typ]
    t = Tally()
    for c in RC.sc_cases(typ):
        p, name = c["params"], c["name"]
        nc = int(p[HR.SC["n_curve"]])
        a, o, v = c["area"], c["outflow"], c["net_vol"]
        got, _ = P.storage_parts("area_at", p, c["dt"], a["Y"])
        t.check(f"area_at [{name}]", typ, got, a["ref"], a["bar"], at=dict(Y=a["Y"]))
        if nc:
            _, ys = HR.sc_curve(p)
            br = HR.sc_area_branch(p, a["Y"])
            t.same_bits(f"area_at, clamped ends [{name}]", typ, got[br < 0], (p[HR.SC["alpha"]] * np.where(br == -1, ys[0], ys[-1]))[br < 0])
        else:
            t.same_bits(f"area_at, n_curve = 0 [{name}]", typ, got, np.full(len(got), p[HR.SC["area"]]))
        got, _ = P.storage_parts("outflow", p, c["dt"], o["Y"])
        t.check(f"outflow [{name}]", typ, got, o["ref"], o["bar"], scale=o["scale"], at=dict(Y=o["Y"]))
        if int(p[HR.SC["rc_type"]]) == 0:
            t.same_bits(f"outflow, rc_type = 0 [{name}]", typ, got, np.zeros(len(got), dtype=D))
        got, _ = P.storage_parts("net_vol", p, c["dt"], v["Y1"], v["Y2"])
        t.check(f"net_vol [{name}]", typ, got, v["ref"], v["bar"], scale=v["scale"], at=dict(Y1=v["Y1"], Y2=v["Y2"]))
        same = v["Y1"] == v["Y2"]
        assert same.sum() >= 2
        t.same_bits(f"net_vol(Y, Y) == 0 [{name}]", typ, got[same], np.zeros(int(same.sum()), dtype=D))
        if nc == 0:
            t.same_bits(f"net_vol, n_curve = 0 [{name}]", typ, got, (v["Y2"] - v["Y1"]) * p[HR.SC["area"]])
    t.done()


def _root_checks(t, label, typ, c, Y, keep):
    """the root criterion on the points `keep`: prints the worst multiple of w / FACTOR that was needed"""
    D = RC.TYPES[typ]
    p = c["params"]
    inside = np.isfinite(Y) & (Y >= p[HR.SC["Y_min"]]) & (Y <= p[HR.SC["Y_max"]])
    need = RC.sc_root_brackets(c, np.where(keep & inside, Y, D(RC.Y_LO + 1.0)), typ)
    need = np.where(inside, need, np.inf)[keep]
    w = float(need.max()) if len(need) else 0.0
    print(f"HELPER {label} | {typ} | {int(keep.sum())} root points | worst multiple of w / {RC.FACTOR:.0f}: {w:.0f} | bar {RC.FACTOR:.0f}")
    if not w <= RC.FACTOR:
        bad = np.nonzero(keep)[0][~(need <= RC.FACTOR)]
        t.failed.append(f"{label} {typ}: no sign change of f within w at {len(bad)} points, first {bad[:4].tolist()}")
    return w


@pytest.mark.parametrize("typ", TYPS)
def test_storage_root(P, typ):
    """storage_root on every parameter set: the flag bit for bit, f(end) == 0 returns that end, and at every root point away from a
    switch of the trapezoid the wide f changes sign within w of the returned stage; fp64: within 10 x 2 delta of scipy's brentq"""
    D = RC.TYPES[typ]
    t = Tally()
    for c in RC.sc_cases(typ):
        p, name, r = c["params"], c["name"], c["root"]
        Y, flag = P.storage_parts("storage_root", p, c["dt"], c["yold"], c["vol"])
        t.same_bits(f"storage_root.flag [{name}]", typ, flag.astype(D), r["flag"])
        ends = r["end"] != 0
        if ends.any():
            t.same_bits(f"storage_root, f(end) == 0 [{name}]", typ, Y[ends], np.where(r["end"] == -1, p[HR.SC["Y_min"]], p[HR.SC["Y_max"]])[ends])
        br = RC.sc_reference_roots(typ)[c["name"]]
        keep = RC.sc_compared(c, br)
        _root_checks(t, f"storage_root [{name}]", typ, c, Y, keep)
        if typ == "f64":
            d = np.abs(Y[keep] - br[keep]) / (2.0 * HR.brent_delta(br[keep]))
            print(f"HELPER storage_root - brentq [{name}] | {typ} | worst {float(d.max()):.3f} x 2 delta | bar 10")
            if not d.max() <= 10.0:
                t.failed.append(f"storage_root [{name}]: {float(d.max())} x 2 delta from brentq's root at {int(np.nonzero(keep)[0][np.argmax(d)])}")
    t.done()


@pytest.mark.parametrize("typ", TYPS)
def test_general_reservoir_row(P, typ):
    """bc_eval<true> for FS_BC_STORAGE_CURVE: the flag, the stage it returns (the root of ITS reservoir state: at level 1 Yold is
    h + bed and Yprev is ignored), and res, dh, dq against the restatement at that stage; shared and per-reach layouts bit for bit"""
    D = RC.TYPES[typ]
    T = HR.reference_type(D)
    t = Tally()
    for c in RC.sc_cases(typ):
        p, name, sec, level, rr = c["params"], c["name"], c["sec"], c["level"], c["row_root"]
        h, Q, Qold, Yprev = c["row_pts"]
        got = P.bc_general(HR.KINDS["storage_curve"], p, sec, level, c["dt"], h, Q, Qold, Yprev)
        wide = P.bc_general(HR.KINDS["storage_curve"], np.ascontiguousarray(np.repeat(p[:, None], len(h), axis=1)), sec, level, c["dt"], h, Q, Qold, Yprev)
        for f in ("res", "dh", "dq", "Ynew"):
            t.same_bits(f"bc_eval<true>.{f}, per-reach layout [{name}]", typ, wide[f], got[f])
        t.same_bits(f"bc_eval<true>.flag, per-reach layout [{name}]", typ, wide["flag"].astype(D), got["flag"])
        sure = rr["margin"] >= RC.FLAG_MARGIN                       # (all but the f(end) == 0 points, exact in the parts' states only)
        t.same_bits(f"bc_eval<true>.flag [{name}]", typ, got["flag"][sure].astype(D), rr["flag"][sure])
        ok = sure & (rr["flag"] == HR.FS_OK) & (got["flag"] == HR.FS_OK)
        ymin = p[HR.SC["min_stage"]]
        floor = np.array([c["tags"].get(i) == "floor" for i in range(len(h))])
        t.same_bits(f"bc_eval<true>.Ynew on the floor [{name}]", typ, got["Ynew"][floor], np.full(int(floor.sum()), ymin))
        # the returned stage is the root of the row's own reservoir state
        state = dict(c, yold=c["row_yold"], vol=c["row_vol"], root=rr)
        raw = ok & (got["Ynew"] > ymin)
        keep = raw & (RC.sc_switch_distance(p, c["row_yold"], got["Ynew"]) >= RC.SWITCH_GAP)
        assert (raw & ~keep).sum() <= RC.MAX_DROPPED * raw.sum(), name
        _root_checks(t, f"bc_eval<true>.Ynew [{name}]", typ, state, got["Ynew"], keep)
        # the row at the device's own stage
        Y = got["Ynew"][ok]
        args = (p, sec, level, c["dt"], h[ok], Q[ok], Qold[ok], Y)
        ref = HR.sc_row(*args, T)
        plain = HR.sc_row(*args, D)
        at = dict(h=h[ok], Q=Q[ok], Y=Y)
        for f in ("res", "dh", "dq"):
            bar = RC.COMPOSITE_F64 if typ == "f64" else RC.FACTOR * HR.noise(plain[f], ref[f], ref["s_" + f])
            t.check(f"bc_eval<true>.{f} [{name}]", typ, got[f][ok], ref[f], bar, scale=ref["s_" + f], at=at)
        for f, (mask, val) in ref["exact"].items():
            t.same_bits(f"bc_eval<true>.{f} where exact [{name}]", typ, got[f][ok][mask], val[mask])
        assert ref["floored"].sum() >= 8
    t.done()


@pytest.mark.parametrize("typ", TYPS)
def test_host_row(P, typ):
    """FS_BC_HOST_ROW hands back columns 0, 1, 2 of each reach's own rows: dh, dq, res, NaN and inf included"""
    D = RC.TYPES[typ]
    rows = RC.host_rows(D)
    z = np.zeros(rows.shape[1], dtype=D)
    got = P.bc_general(HR.KINDS["host_row"], rows, RC.bc_section("general", RC.Z, D), 2, RC.DT, z + D(3), z, z, z)
    t = Tally()
    for k, f in enumerate(("dh", "dq", "res")):
        t.same_bits(f"bc_eval<true>.{f} [host row]", typ, got[f], rows[k])
    assert np.all(got["flag"] == HR.FS_OK)
    t.done()
