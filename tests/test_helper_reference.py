"""tests/helper_reference.py and tests/helper_recipes.py on the CPU: what the device-helper tests (tests/test_gpu_device_helpers.py) rest on.

  * the restatement, run in float64, is the oracle's section_props / conveyance / equivalent_n / dR_dA / dK_dA / node_terms /
    boundary_eval on the recipes' own sections, points and boundary parameter sets, at the bar of tests/test_derived_reference.py;
  * the long double scalar functions agree with mpmath at 50 digits within 4e-19 on 4 096 points each;
  * the bars: every "4 x noise" bar is printed with the restatement noise it comes from (run with -s);
  * the restatement of the general reservoir row, run in float64, is the oracle's storage_area_at / storage_net_vol / storage_outflow, the mass
    balance of storage_mass_balance and the general-storage branch of boundary_eval (at the stage brentq found) on every parameter set;
  * the root criterion accepts scipy's brentq root of the float64 balance on every compared root point; at most 5 % of a set's root points
    lie within 1e-3 of a switch of the trapezoid's n and no special point does; |f| at the bracket ends of every flag point is 1000 x the noise of
    f or exactly 0; the part points visit every interval, breakpoint, clamp and form of the trapezoid;
  * the comparison routine fails when ONE point of 2^18 is moved by twice its bar, and passes when it is moved by half, for every bar."""
import numpy as np
import pytest

import helper_recipes as RC
import helper_reference as HR
from oracle import preissmann_oracle as O

BAR = 1e-13               # tests/test_derived_reference.py
MP_BAR = 4e-19


def test_long_double_is_wide_enough():
    assert np.finfo(np.longdouble).eps < 1e-18
    assert HR.reference_type(np.float64) is np.longdouble and HR.reference_type(np.float32) is np.float64


def _rel(got, want, scale=None):
    return HR.worst(np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), scale)[0]


@pytest.mark.parametrize("case", RC.node_cases("f64"), ids=lambda c: c["name"])
def test_float64_restatement_is_the_oracles_node_terms(case):
    sec, h, Q = case["sec"], case["h"], case["Q"]
    geo = HR.oracle_geo(sec)
    geo = {k: np.repeat(v, len(h)) for k, v in geo.items()}
    want = O.node_terms(geo, h, Q)
    got, scale = HR.node_terms(sec, h, Q, np.float64)
    g = HR.general_props(sec, h, np.float64)
    pairs = [("A", got["A"], want["A"], None), ("T", got["T"], want["T"], None), ("Se", got["Se"], want["Se"], scale["Se"]),
             ("dSe_dA", got["eAT"], want["dSe_dA"], scale["eAT"]), ("dSe_dQ", got["eQ"], want["dSe_dQ"], scale["eQ"]),
             ("K", g["K"], want["K"], None), ("dKdA", g["dKdA"], want["dKdA"], None), ("P", g["P"], want["P"], None),
             ("R", g["Rh"], want["R"], None), ("n_eq", g["neq"], want["n_eq"], None),
             ("dR_dA", g["dRdA"], O.dR_dA(geo, h, O.section_props(geo, h)), 1.0 / g["P"])]
    assert np.array_equal(g["over"], O.section_props(geo, h)[4])
    for name, a, b, s in pairs:
        e = _rel(a, b, s)
        print(case["name"], name, e)
        assert e <= BAR, (name, e)


def _oracle_bc(case):
    p = [float(v) for v in case["params"]]
    K = HR.KINDS
    kind = case["kind"]
    if kind == K["flow"]:
        return O.BC("flow_hydrograph")
    if kind == K["stage"]:
        return O.BC("stage_hydrograph", bed_level=p[0])
    if kind == K["fixed"]:
        return O.BC("fixed_depth", initial_depth=p[0])
    if kind == K["normal"]:
        return O.BC("normal_depth", bed_slope=p[0], bed_level=p[1])
    if kind == K["power"]:
        return O.BC("rating_curve", bed_level=p[3], rc_type="power", rc=dict(a=p[0], b=p[1], shift=p[2]))
    if kind == K["poly"]:
        return O.BC("rating_curve", bed_level=p[4], rc_type="polynomial", rc=dict(a=p[0], b=p[1], c=p[2], shift=p[3]))
    if kind == K["blend"]:
        return O.BC("rating_curve", bed_level=p[9], rc_type="blend", rc=dict(initial_stage=p[0], buffer=p[1], low=p[2:5], high=p[5:8], dY=p[8]))
    return O.BC("fixed_depth", bed_level=p[4], storage=dict(area=p[0], min_stage=p[1], Y_min=p[2], Y_max=p[3]))


@pytest.mark.parametrize("case", RC.bc_cases("f64"), ids=lambda c: f"{c['name']}-{c['form']}")
def test_float64_restatement_is_the_oracles_boundary_eval(case):
    h, Q, Qold, Yprev, tgt = case["pts"]
    got = HR.bc_row(case["kind"], case["params"], case["sec"], case["level"], case["dt"], h, Q, Qold, Yprev, tgt, np.float64)
    bc = _oracle_bc(case)
    geo = HR.oracle_geo(case["sec"])
    every = 8 if case["kind"] == HR.KINDS["normal"] else 1            # (two section evaluations per point in the oracle)
    worst = dict(res=0.0, dh=0.0, dq=0.0, Y=0.0)
    for i in range(0, len(h), every):
        bc.target = np.array([0.0, 0.0, float(tgt[i])])
        store = dict(Y_prev=float(Yprev[i]))
        k = case["level"]
        try:
            res, dh, dq = O.boundary_eval(bc, geo, float(h[i]), float(Q[i]), k, float(case["dt"]), Q_old=float(Qold[i]), store=store)
        except O.StorageRange:
            assert got["flag"][i] == HR.FS_STORAGE_RANGE
            continue
        assert got["flag"][i] == HR.FS_OK
        sr = float(got["s_res"][i])
        sd = abs(dh) if got["s_dh"] is None else float(got["s_dh"][i])
        worst["res"] = max(worst["res"], abs(got["res"][i] - res) / sr)
        worst["dh"] = max(worst["dh"], abs(got["dh"][i] - dh) / sd if sd else abs(got["dh"][i] - dh))
        worst["dq"] = max(worst["dq"], abs(got["dq"][i] - dq))
        if "Y_eval" in store:
            worst["Y"] = max(worst["Y"], abs(got["Ynew"][i] - store["Y_eval"]) / abs(store["Y_eval"]))
    print(case["name"], case["form"], worst)
    assert worst["res"] <= BAR and worst["dh"] <= BAR and worst["dq"] == 0.0 and worst["Y"] <= BAR, worst
    if case["kind"] == HR.KINDS["storage"]:
        assert (got["flag"] == HR.FS_STORAGE_RANGE).sum() >= len(h) // 3 and (got["flag"] == HR.FS_OK).sum() >= len(h) // 3
        assert ((got["dq"] == 0) & (got["flag"] == HR.FS_OK)).any(), "no point on the floor inside the range"


def test_the_blend_points_straddle_both_buffer_edges():
    for case in RC.bc_cases("f64") + RC.bc_cases("f32"):
        if case["kind"] != HR.KINDS["blend"]:
            continue
        D = case["params"].dtype.type
        z = D(case["params"][9]) + case["pts"][0]
        dY = D(case["params"][8])
        br = [HR.blend_alpha_branch(v, D(case["params"][0]), D(case["params"][1])) for v in (z - dY, z, z + dY)]
        triples = set(zip(*(b.tolist() for b in br)))
        assert {(0, 0, 0), (2, 2, 2), (1, 1, 1), (0, 0, 2), (0, 2, 2), (2, 2, 1), (2, 1, 1)} <= triples, triples


def _mp_of(x):
    import mpmath as mp
    hi = float(x)
    return mp.mpf(hi) + mp.mpf(float(x - np.longdouble(hi)))


def test_long_double_scalar_functions_against_mpmath():
    import mpmath as mp
    mp.mp.dps = 50
    rng = np.random.default_rng(7)
    n = 4096
    worst = {}
    for op in HR.UNARY_OPS:
        if op == "exp_short":
            x = rng.uniform(-60, 60, n)
        elif op == "log_pos":
            x = np.concatenate([HR.log_uniform(rng, 1e-4, 1e4, n // 2, np.float64), 1.0 + rng.uniform(-2e-4, 2e-4, n // 2)])
        else:
            x = HR.log_uniform(rng, 1e-6, 1e6, n, np.float64)
        got = HR.unary_ref(op, x.astype(np.longdouble))
        worst[op] = max(float(abs(_mp_of(g) - HR.unary_mp(op, mp.mpf(float(v)))) / abs(HR.unary_mp(op, mp.mpf(float(v))))) for g, v in zip(got, x))
    a, b = HR.log_uniform(rng, 1e-4, 1e4, n, np.float64), rng.uniform(0.2, 5.0, n)
    got = HR.pow_ref(a.astype(np.longdouble), b.astype(np.longdouble))
    worst["pow"] = max(float(abs(_mp_of(g) / mp.power(mp.mpf(float(u)), mp.mpf(float(v))) - 1)) for g, u, v in zip(got, a, b))
    A, P, n15 = HR.log_uniform(rng, 1e-6, 1e6, n, np.float64), HR.log_uniform(rng, 1e-2, 1e4, n, np.float64), HR.log_uniform(rng, 10, 1e3, n, np.float64)
    got = HR.k15_ref(A.astype(np.longdouble), P.astype(np.longdouble), n15.astype(np.longdouble))
    worst["k15"] = max(float(abs(_mp_of(g) / (mp.power(mp.mpf(float(u)), mp.mpf(5) / 2) / mp.mpf(float(v)) * mp.mpf(float(w))) - 1))
                       for g, u, v, w in zip(got, A, P, n15))
    for k, v in worst.items():
        print(f"long double {k}: worst relative error against mpmath {v:.2e}")
    assert all(v <= MP_BAR for v in worst.values()), worst


@pytest.mark.parametrize("typ", ["f64", "f32"])
def test_bars_and_the_noise_they_come_from(typ):
    eps = float(np.finfo(RC.TYPES[typ]).eps)
    for c in RC.scalar_cases(typ):
        extra = f" | libm pair {c['pair']:.3e}" if "pair" in c else (f" | noise {c['bar'] / RC.FACTOR:.3e}" if c["source"] == "4 x noise" else "")
        print(f"BAR {c['name']} | {typ} | {c['bar']:.3e} | {c['source']}{extra}")
        assert np.isfinite(c["bar"]) and c["bar"] > 0 and np.all(np.isfinite(c["ref"].astype(np.float64)))
        if c["source"] == "4 x noise":
            assert c["bar"] >= RC.FACTOR * eps
    for label, bar in RC.all_bars(typ)[len(RC.scalar_cases(typ)):]:
        print(f"BAR {label} | {typ} | {bar:.3e} | " + ("1e-12" if typ == "f64" else f"4 x noise | noise {bar / RC.FACTOR:.3e}"))
        assert np.isfinite(bar) and bar >= (RC.COMPOSITE_F64 if typ == "f64" else RC.FACTOR * eps)


@pytest.mark.parametrize("typ", ["f64", "f32"])
def test_one_point_of_2_18_moved_by_twice_its_bar_fails(typ, capsys):
    D = RC.TYPES[typ]
    T = HR.reference_type(D)
    rng = np.random.default_rng(3)
    n = 1 << 18
    ref = (HR.log_uniform(rng, 1e-3, 1e3, n, np.float64) * rng.choice([-1.0, 1.0], n)).astype(T)
    scale = np.abs(ref) * T(1.5)
    bars = sorted({b for _, b in RC.all_bars(typ)})
    assert len(bars) >= 3
    for bar in bars:
        i = int(rng.integers(n))
        for sc in (None, scale):
            s = abs(ref[i]) if sc is None else sc[i]
            bad, fine = ref.copy(), ref.copy()
            bad[i] += T(2 * bar) * s
            fine[i] += T(0.5 * bar) * s
            HR.check("moved", typ, fine, ref, bar, sc)
            with pytest.raises(AssertionError):
                HR.check("moved", typ, bad, ref, bar, sc)
    bad = ref.copy()
    bad[5] = np.nan
    with pytest.raises(AssertionError):
        HR.check("nan", typ, bad, ref, 1.0)
    capsys.readouterr()


# ------------------------------------------------------------------------------------------------------------------------------
# the general reservoir row: restatement against the oracle, the root criterion against scipy, the conditions on the points
# ------------------------------------------------------------------------------------------------------------------------------
SC_IDS = [c["name"] for c in RC.sc_cases("f64")]


def _sc_bc(case):
    p = case["params"]
    return O.BC("fixed_depth", bed_level=float(p[HR.SC["bed"]]), storage=HR.sc_oracle_st(p))


@pytest.mark.parametrize("case", RC.sc_cases("f64"), ids=SC_IDS)
def test_float64_restatement_is_the_oracles_storage_functions(case):
    p, st = case["params"], HR.sc_oracle_st(case["params"])
    Y = case["area"]["Y"]
    e = _rel(HR.sc_area_at(p, Y, np.float64), [O.storage_area_at(st, float(y)) for y in Y])
    assert e <= BAR, ("area_at", e)
    q, sq = HR.sc_outflow(p, Y, np.float64)
    e = _rel(q, [O.storage_outflow(st, float(y)) for y in Y], sq)
    assert e <= BAR, ("outflow", e)
    y1, y2 = case["net_vol"]["Y1"], case["net_vol"]["Y2"]
    v, sv = HR.sc_net_vol(p, y1, y2, np.float64)
    e = _rel(v, [O.storage_net_vol(st, float(a), float(b)) for a, b in zip(y1, y2)], sv)
    assert e <= BAR, ("net_vol", e)
    # the mass balance at both bracket ends and at a stage inside, for every reservoir state with a finite volume
    yold, vol = case["yold"], case["vol"]
    ok = np.isfinite(vol)
    rng = np.random.default_rng(11)
    for Ys in (np.full(len(yold), RC.Y_LO), np.full(len(yold), RC.Y_HI), rng.uniform(RC.Y_LO, RC.Y_HI, len(yold))):
        f, sf = HR.sc_f(p, yold[ok], vol[ok], RC.DT_SC, Ys[ok], np.float64)
        want = []
        for yo, vo, y in zip(yold[ok], vol[ok], Ys[ok]):
            qo = 0.5 * (O.storage_outflow(st, float(yo)) + O.storage_outflow(st, float(y))) if st.get("rc") is not None else 0.0
            want.append(O.storage_net_vol(st, float(yo), float(y)) - (float(vo) - qo * RC.DT_SC))
        e = _rel(f, want, sf)
        assert e <= BAR, ("f", e)


@pytest.mark.parametrize("case", RC.sc_cases("f64"), ids=SC_IDS)
def test_float64_restatement_is_the_oracles_general_storage_row(case):
    """boundary_eval finds the stage with storage_mass_balance (brentq); the restatement is evaluated AT that stage"""
    p, sec, level = case["params"], case["sec"], case["level"]
    h, Q, Qold, Yprev = case["row_pts"]
    bc, geo = _sc_bc(case), HR.oracle_geo(sec)
    want, idx, Ys = [], [], []
    for i in range(len(h)):
        store = dict(Y_prev=float(Yprev[i]))
        try:
            want.append(O.boundary_eval(bc, geo, float(h[i]), float(Q[i]), level, RC.DT_SC, Q_old=float(Qold[i]), store=store))
        except O.StorageRange:
            assert case["row_root"]["flag"][i] == HR.FS_STORAGE_RANGE, i
            continue
        assert case["row_root"]["flag"][i] == HR.FS_OK, i
        idx.append(i)
        Ys.append(store["Y_eval"])
    idx, want = np.array(idx), np.array(want)
    got = HR.sc_row(p, sec, level, RC.DT_SC, h[idx], Q[idx], Qold[idx], np.array(Ys), np.float64)
    worst = {f: _rel(got[f], want[:, k], got["s_" + f]) for k, f in enumerate(("res", "dh", "dq"))}
    print(case["name"], worst)
    assert all(v <= BAR for v in worst.values()), worst
    for f, (mask, val) in got["exact"].items():
        assert np.array_equal(got[f][mask], val[mask]), f
    floored = got["floored"]
    assert floored.sum() >= 8 and (~floored).sum() >= 400, "the floor is not visited"
    if level == 1:
        assert np.all(np.abs(Yprev - case["row_yold"]) > 0), "a level-1 Yprev that equals Yold does not show that it is ignored"


@pytest.mark.parametrize("typ", ["f64", "f32"])
def test_the_root_criterion_accepts_scipys_roots_and_the_points_meet_their_conditions(typ):
    D = RC.TYPES[typ]
    n_checked = 0
    for c in RC.sc_cases(typ):
        r, tags = c["root"], c["tags"]
        br = RC.sc_reference_roots(typ)[c["name"]]
        assert np.all(np.isfinite(br[r["is_root"]]))
        # root points away from a switch: at most 5 % dropped, no special point among them
        keep = RC.sc_compared(c, br)
        dropped = r["is_root"] & ~keep
        assert dropped.sum() <= RC.MAX_DROPPED * r["is_root"].sum(), (c["name"], int(dropped.sum()))
        assert not any(dropped[i] for i in tags), (c["name"], [tags[i] for i in tags if dropped[i]])
        # the criterion holds for brentq's root (rounded to the device type: the width has one ulp in it)
        need = RC.sc_root_brackets(c, np.where(keep, br, RC.Y_LO + 1.0).astype(D), typ)
        assert np.all(need[keep] <= RC.FACTOR), (c["name"], np.nonzero(keep & ~(need <= RC.FACTOR))[0][:8])
        n_checked += int(keep.sum())
        print(f"ROOT {c['name']} | {typ} | {int(keep.sum())} of {int(r['is_root'].sum())} root points | worst multiple {need[keep].max():.0f} | noise_f {r['noise_f']:.2e}")
        # flag points away from zero, in the parts' states and in the row's; the f == 0 points are exact in the parts' states only
        assert r["margin"].min() >= RC.FLAG_MARGIN, (c["name"], r["margin"].min())
        rr = c["row_root"]
        exact_only = np.array([tags.get(i, "").endswith("_zero") for i in range(len(br))])
        assert rr["margin"][~exact_only].min() >= RC.FLAG_MARGIN, (c["name"], rr["margin"][~exact_only].min())
        assert np.array_equal(rr["flag"][~exact_only], r["flag"][~exact_only])
        # every special point is there and is what its name says
        want = set(RC.ROOT_SPECIAL) - (set() if c["name"] == "const_area" else {"f_lo_zero", "f_hi_zero"})
        assert set(tags.values()) == want
        for i, t in tags.items():
            if t in ("both_negative", "both_positive", "nan"):
                assert r["flag"][i] == HR.FS_STORAGE_RANGE, (c["name"], t)
            else:
                assert r["flag"][i] == HR.FS_OK and r["end"][i] == {"f_lo_zero": -1, "f_hi_zero": 1}.get(t, 0), (c["name"], t)
            if t == "floor":
                assert br[i] < c["params"][HR.SC["min_stage"]]
        if int(c["params"][HR.SC["n_curve"]]) > 2:
            n = HR.sc_trapezoid_n(c["params"], c["yold"], br.astype(D))[r["is_root"]]
            assert n.max() >= 19 and (n <= 2).any() and (n > 2).any()
    assert n_checked >= 3400


@pytest.mark.parametrize("typ", ["f64", "f32"])
def test_the_part_points_visit_every_branch(typ):
    for c in RC.sc_cases(typ):
        p = c["params"]
        nc = int(p[HR.SC["n_curve"]])
        y1, y2 = c["net_vol"]["Y1"], c["net_vol"]["Y2"]
        if nc:
            # |Y2 - Y1| / step at 1.9, 2, 2.99, 3, 3.01 with both signs, as the device type rounds it
            assert HR.sc_trapezoid_n(p, y1, y2)[:10].tolist() == [1, 2, 2, 3, 3] * 2, c["name"]
            xs, _ = HR.sc_curve(p)
            Y = c["area"]["Y"]
            x = Y + p[HR.SC["beta"]]
            br = HR.sc_area_branch(p, Y)
            assert set(br.tolist()) == {-1, -2} | set(range(nc - 1)), c["name"]
            for b in xs:
                assert (x == b).any() and (x == np.nextafter(b, p.dtype.type(0))).any() and (x == np.nextafter(b, p.dtype.type(99))).any(), (c["name"], b)
        assert np.all(y1[12:14] == y2[12:14])
    rows = RC.host_rows(RC.TYPES[typ])
    assert rows.shape == (3, 65) and np.isnan(rows).sum() == 2 and np.isinf(rows).sum() == 2
