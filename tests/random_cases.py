"""The seeded draws of the random sweeps (tests/test_gpu_random_cases.py; tests/test_near_critical.py and tools/scan_supercritical.py
take the same draws): prismatic reaches far outside the benchmark's parameter boxes, non-prismatic compound channels with bends,
and mild reaches under a tide that reverses the flow."""
import numpy as np

from oracle import preissmann_oracle as O
from synth import akbari_shape, normal_depth_rect, normal_depth_trap

US_KINDS = ("flow", "flow", "flow", "stage", "fixed", "rating_us")
DS_KINDS = ("normal", "normal", "power", "poly", "fixed", "stage_ds", "flow_ds", "storage", "blend")


def wave(nt, dt, rise, fall, amp):
    return np.array([akbari_shape(1.0, amp, rise, fall, k * dt) for k in range(nt)])


def random_problem(seed, nodes=None):
    rng = np.random.default_rng(770000 + seed)
    N = int(rng.choice([2, 3, 5, 17, 63, 64, 65, 127, 128, 129, 200, 255, 256, 257, 400, 511, 512, 513, 700]))
    if nodes is not None:
        N = int(nodes)             # (the long-reach sweep below: the same draws on a reach of its own length)
    trapezoid = bool(rng.integers(0, 2))
    b = float(np.exp(rng.uniform(np.log(3.0), np.log(600.0))))
    m = float(rng.uniform(0.5, 3.0)) if trapezoid else 0.0
    n = float(rng.uniform(0.012, 0.08))
    S0 = float(np.exp(rng.uniform(np.log(5e-5), np.log(5e-3))))
    q = float(np.exp(rng.uniform(np.log(0.05), np.log(8.0))))          # base flow per metre of bed width
    Qb = q * b
    theta = float(rng.uniform(0.55, 1.0))
    dt = float(np.exp(rng.uniform(np.log(30.0), np.log(3600.0))))
    dx = float(np.exp(rng.uniform(np.log(25.0), np.log(2000.0))))
    n_steps = int(rng.integers(2, 7))
    amp = float(np.exp(rng.uniform(np.log(0.1), np.log(3.0))))
    L = (N - 1) * dx
    geo = {k: np.zeros(N) for k in O.GEO_KEYS}
    geo["b_main"][:] = b; geo["m_main"][:] = m
    geo["n_main"][:] = n; geo["n_left"][:] = n; geo["n_right"][:] = n
    geo["z_bed"] = S0 * L * (1 - np.arange(N) / (N - 1))
    hn = normal_depth_trap(b, m, n, S0, Qb) if trapezoid else normal_depth_rect(b, n, S0, Qb)
    nt = n_steps + 1
    shape = wave(nt, dt, rng.uniform(2, 6) * dt, rng.uniform(7, 14) * dt, amp)        # 1 ... 1 + amp ... 1
    us_k, ds_k = US_KINDS[rng.integers(0, len(US_KINDS))], DS_KINDS[rng.integers(0, len(DS_KINDS))]
    if ds_k == "storage" and N > 130:
        ds_k = "normal"            # the reservoir row's level-1 quirk (boundary.py:104-108): short reaches only
    if us_k != "flow" and ds_k in ("flow_ds",):
        ds_k = "normal"            # a flow imposed at the outlet needs a flow imposed at the inlet to stay well posed here
    zu = S0 * L
    if us_k == "flow":
        us = O.BC("flow_hydrograph", bed_level=zu, target=Qb * shape)
    elif us_k == "stage":
        us = O.BC("stage_hydrograph", bed_level=zu, target=zu + hn * (1.0 + 0.3 * np.minimum(amp, 1.0) * (shape - 1.0) / amp))
    elif us_k == "fixed":
        us = O.BC("fixed_depth", bed_level=zu, initial_depth=hn)
    else:
        us = O.BC("rating_curve", bed_level=zu, rc_type="polynomial", rc=dict(a=0.0, b=-0.2 * Qb, c=Qb + 0.2 * Qb * (zu + hn), shift=0.0))
    if ds_k == "normal":
        ds = O.BC("normal_depth", bed_level=0.0, bed_slope=S0)
    elif ds_k == "fixed":
        ds = O.BC("fixed_depth", bed_level=0.0, initial_depth=hn)
    elif ds_k == "poly":
        ds = O.BC("rating_curve", bed_level=0.0, rc_type="polynomial", rc=dict(a=0.15 * Qb / hn ** 2, b=0.85 * Qb / hn, c=0.0, shift=0.0))
    elif ds_k == "power":
        be = float(rng.uniform(1.2, 2.2))
        ds = O.BC("rating_curve", bed_level=0.0, rc_type="power", rc=dict(a=Qb / hn ** be, b=be, shift=0.0))
    elif ds_k == "flow_ds":
        ds = O.BC("flow_hydrograph", bed_level=0.0, target=Qb * (1.0 - 0.25 * (shape - 1.0) / amp))
    elif ds_k == "stage_ds":
        ds = O.BC("stage_hydrograph", bed_level=0.0, target=hn * (1.0 + 0.2 * (shape - 1.0) / amp))
    elif ds_k == "storage":
        ds = O.BC("fixed_depth", bed_level=0.0, initial_depth=hn,
                  storage=dict(area=max(40.0 * b * L / 50.0, 1e3), min_stage=0.5 * hn, Y_min=0.0, Y_max=50.0 * hn))
    else:
        lo = [0.0, 0.9 * Qb / hn, 0.1 * Qb / hn ** 2]
        ds = O.BC("rating_curve", bed_level=0.0, rc_type="blend",
                  rc=dict(initial_stage=hn, buffer=0.5, low=lo, high=[2 * v for v in lo], dY=1e-3))
    p = O.Problem(geo=geo, h0=np.full(N, hn), Q0=np.full(N, Qb), us=us, ds=ds, theta=theta, dt=dt, dx=dx, nt=nt, tol=1e-6)
    info = dict(N=N, trapezoid=trapezoid, b=b, m=m, n=n, S0=S0, Qb=Qb, theta=theta, dt=dt, dx=dx, amp=amp, us=us_k, ds=ds_k, hn=hn,
                courant=(Qb / (b * hn) + (9.80665 * hn) ** 0.5) * dt / dx, froude=Qb / (b * hn) / (9.80665 * hn) ** 0.5)
    return p, info


def random_table_problem(seed):
    """non-prismatic channel with compound sections (flood plains the wave reaches in some draws) and bends: width, side
    slope, bed slope, roughness, bankfull depth and curvature vary along the reach"""
    rng = np.random.default_rng(880000 + seed)
    N = int(rng.choice([3, 9, 33, 64, 65, 121, 128, 129, 200, 256, 257, 400, 513]))
    x = np.linspace(0.0, 1.0, N)
    smooth = lambda lo, hi: lo + (hi - lo) * (0.5 + 0.5 * np.sin(2 * np.pi * (rng.uniform(0.3, 1.5) * x + rng.uniform())))
    b0 = float(np.exp(rng.uniform(np.log(8.0), np.log(300.0))))
    b = b0 * smooth(0.85, 1.15)
    m = smooth(*sorted(rng.uniform(0.5, 2.5, 2)))
    nm = smooth(*sorted(rng.uniform(0.02, 0.045, 2)))
    S0 = float(np.exp(rng.uniform(np.log(1e-4), np.log(2e-3))))
    dx = float(np.exp(rng.uniform(np.log(100.0), np.log(1500.0))))
    dt = float(np.exp(rng.uniform(np.log(120.0), np.log(3600.0))))
    theta = float(rng.uniform(0.55, 1.0))
    q = float(np.exp(rng.uniform(np.log(0.3), np.log(5.0))))
    Qb = q * b0
    hn = normal_depth_trap(b0, float(m.mean()), float(nm.mean()), S0, Qb)
    geo = {k: np.zeros(N) for k in O.GEO_KEYS}
    geo["b_main"], geo["m_main"], geo["n_main"] = b, m, nm
    geo["n_left"] = nm * rng.uniform(1.2, 2.0); geo["n_right"] = nm * rng.uniform(1.2, 2.0)
    geo["z_bed"] = S0 * (N - 1) * dx * (1 - x) + 0.05 * hn * np.sin(6 * np.pi * x)
    geo["is_compound"][:] = 1.0
    geo["h_bf"] = hn * smooth(*sorted(rng.uniform(0.9, 2.2, 2)))          # some nodes over bank from the start, some never
    geo["b_fp_l"] = b * rng.uniform(0.5, 4.0); geo["b_fp_r"] = b * rng.uniform(0.5, 4.0)
    geo["m_fp"][:] = rng.uniform(2.0, 6.0)
    geo["curvature"] = rng.uniform(0.0, 2e-3) * np.sin(2 * np.pi * rng.uniform(0.5, 2.0) * x)
    n_steps = int(rng.integers(2, 6))
    nt = n_steps + 1
    amp = float(np.exp(rng.uniform(np.log(0.2), np.log(2.5))))
    shape = wave(nt, dt, rng.uniform(2, 5) * dt, rng.uniform(6, 12) * dt, amp)
    ds_k = ("normal", "power", "poly", "fixed", "stage_ds", "blend")[rng.integers(0, 6)]
    us = O.BC("flow_hydrograph", bed_level=float(geo["z_bed"][0]), target=Qb * shape)
    zb = float(geo["z_bed"][-1])
    if ds_k == "normal":
        ds = O.BC("normal_depth", bed_level=zb, bed_slope=S0)
    elif ds_k == "fixed":
        ds = O.BC("fixed_depth", bed_level=zb, initial_depth=hn)
    elif ds_k == "poly":
        ds = O.BC("rating_curve", bed_level=zb, rc_type="polynomial", rc=dict(a=0.15 * Qb / hn ** 2, b=0.85 * Qb / hn, c=0.0, shift=-zb))
    elif ds_k == "power":
        ds = O.BC("rating_curve", bed_level=zb, rc_type="power", rc=dict(a=Qb / hn ** 1.5, b=1.5, shift=-zb))
    elif ds_k == "stage_ds":
        ds = O.BC("stage_hydrograph", bed_level=zb, target=zb + hn * (1.0 + 0.2 * (shape - 1.0) / amp))
    else:
        lo = [0.0, 0.9 * Qb / hn, 0.1 * Qb / hn ** 2]
        ds = O.BC("rating_curve", bed_level=zb, rc_type="blend",
                  rc=dict(initial_stage=zb + hn, buffer=0.5, low=[lo[0] - lo[1] * zb + lo[2] * zb * zb, lo[1] - 2 * lo[2] * zb, lo[2]],
                          high=[2 * (lo[0] - lo[1] * zb + lo[2] * zb * zb), 2 * (lo[1] - 2 * lo[2] * zb), 2 * lo[2]], dY=1e-3))
    p = O.Problem(geo=geo, h0=np.full(N, hn), Q0=np.full(N, Qb), us=us, ds=ds, theta=theta, dt=dt, dx=dx, nt=nt, tol=1e-6)
    return p, dict(N=N, b0=b0, S0=S0, Qb=Qb, hn=hn, theta=theta, dt=dt, dx=dx, amp=amp, ds=ds_k, seed=seed)


def tidal_problem(seed):
    """a mild reach whose downstream stage rises fast enough to push water back up the channel: the flow changes sign
    along the reach and in time (Q|Q| in the friction slope, the sign of the advective term, negative boundary flows)"""
    rng = np.random.default_rng(990000 + seed)
    N = int(rng.choice([9, 33, 64, 65, 129, 256, 400]))
    trapezoid = bool(rng.integers(0, 2))
    b = float(rng.uniform(20.0, 200.0)); m = float(rng.uniform(1.0, 2.5)) if trapezoid else 0.0
    n = float(rng.uniform(0.02, 0.04)); S0 = float(np.exp(rng.uniform(np.log(3e-5), np.log(2e-4))))
    Qb = float(rng.uniform(0.05, 0.3)) * b
    dx = float(rng.uniform(200.0, 800.0)); dt = float(rng.uniform(120.0, 600.0)); theta = float(rng.uniform(0.6, 1.0))
    hn = normal_depth_trap(b, m, n, S0, Qb) if trapezoid else normal_depth_rect(b, n, S0, Qb)
    L = (N - 1) * dx
    geo = {k: np.zeros(N) for k in O.GEO_KEYS}
    geo["b_main"][:] = b; geo["m_main"][:] = m
    geo["n_main"][:] = n; geo["n_left"][:] = n; geo["n_right"][:] = n
    geo["z_bed"] = S0 * L * (1 - np.arange(N) / (N - 1))
    nt = 9
    rise = float(rng.uniform(0.5, 1.5))
    tide = hn * (1.0 + rise * np.sin(np.pi * np.arange(nt) / (nt - 1)) ** 2)
    us = O.BC("flow_hydrograph", bed_level=S0 * L, target=np.full(nt, Qb))
    ds = O.BC("stage_hydrograph", bed_level=0.0, target=tide)
    p = O.Problem(geo=geo, h0=np.full(N, hn), Q0=np.full(N, Qb), us=us, ds=ds, theta=theta, dt=dt, dx=dx, nt=nt, tol=1e-6)
    return p, dict(N=N, trapezoid=trapezoid, b=b, Qb=Qb, hn=hn, rise=rise, dt=dt, dx=dx, seed=seed)
