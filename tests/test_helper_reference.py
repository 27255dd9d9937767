"""tests/helper_reference.py and tests/helper_recipes.py on the CPU: what the device-helper tests (tests/test_gpu_device_helpers.py) rest on.

  * the restatement, run in float64, is the oracle's section_props / conveyance / equivalent_n / dR_dA / dK_dA / node_terms /
    boundary_eval on the recipes' own sections, points and boundary parameter sets, at the bar of tests/test_derived_reference.py;
  * the long double scalar functions agree with mpmath at 50 digits within 4e-19 on 4 096 points each;
  * the bars: every "4 x noise" bar is printed with the restatement noise it comes from (run with -s);
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
