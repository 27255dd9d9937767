"""Adversarial polyline ("irregular") channels: seeded oracle.Problems that steer the device's node evaluation
(flow-sim_amd/csrc/fs_poly.hpp) onto each of its paths, on purpose rather than by chance.

  on_vertex            z_min + h0 equals a vertex elevation bit for bit (every elevation is a multiple of 2^-6 on a bed of
                       2^-4 per node), uniform flow, then a flood wave: the downstream nodes stay within 1e-6 of the vertex
                       (the edge walk of poly_eval_whole, `c1 != c2`), the upstream ones leave it; a variant holds the
                       downstream node on the vertex with a fixed depth.
  near_vertex_mixed    every node its own section; a seeded draw puts each node's initial stage exactly on a vertex, 5e-7 or
                       2e-6 from one, or mid-interval - no period, so the lanes of one wave take different paths at one row.
  many_stations        48 / 120 / 250 stations (KP 64 / 128 / 256) with a different vertex count per node, flat berms, vertical
                       walls, elevations closer than 1e-6, a roughness limit between two stations.
  multi_run            two levees (1, 2 and 3 wetted runs), an isolated wet vertex, runs that touch vertex 0 and vertex n-1, a
                       levee crest exactly at the initial stage.
  overtopped_shallow   one bank below the peak stage, nodes above every vertex, every node starting 0.3 m deep in its lowest
                       interval (a start a few cm deep runs a node dry in the oracle's Newton loop: K = 0).

Every draw whose oracle run has a Newton norm within a factor 1.25 of the tolerance is rejected (the Newton counts would hinge
on the last bits; FRAGILE below says why not a factor 2) and the next one is taken - the same channel with another tolerance, then the next seed; the rejections are
logged.  tests/test_poly_edges.py checks that the cases reach the
paths they claim, tests/test_stage_table.py builds their stage tables, tests/test_gpu_polyline_paths.py runs them on the device."""
import logging

import numpy as np

from oracle import irregular_oracle as IO
from oracle import preissmann_oracle as O

log = logging.getLogger("poly_edges")
DH = 1e-6
Q64 = 1.0 / 64.0               # grid of the on-vertex elevations: sums of them and of the bed are exact
BED_STEP = 1.0 / 16.0          # bed drop per node of the on-vertex reach (S0 = BED_STEP / DX)


def polyline_geo(xs, zs, rough, curv=None):
    """geo dict of a reach of polyline nodes: xs / zs lists of per-node arrays (any lengths), rough [N, 5] =
    (n_left, n_main, n_right, left limit, right limit).  Rows are padded by repeating the node's last station."""
    N = len(xs)
    P = max(len(x) for x in xs)
    X = np.empty((N, P)); Z = np.empty((N, P))
    for i, (x, z) in enumerate(zip(xs, zs)):
        X[i, :len(x)] = x; X[i, len(x):] = x[-1]
        Z[i, :len(z)] = z; Z[i, len(z):] = z[-1]
    rough = np.asarray(rough, dtype=np.float64)
    geo = {k: np.zeros(N) for k in O.GEO_KEYS}
    geo["z_bed"] = np.array([float(np.min(z)) for z in zs])
    geo["n_left"], geo["n_main"], geo["n_right"] = rough[:, 0].copy(), rough[:, 1].copy(), rough[:, 2].copy()
    geo["curvature"] = np.zeros(N) if curv is None else np.asarray(curv, dtype=np.float64)
    geo["irr_x"], geo["irr_z"] = X, Z
    geo["irr_npts"] = np.array([len(x) for x in xs], dtype=np.int32)
    geo["irr_limits"] = rough[:, 3:5].copy()
    return geo


def node_section(p, i):
    """(x, z, rough, curvature) of node i of a polyline Problem"""
    g = p.geo
    c = int(g["irr_npts"][i])
    return (g["irr_x"][i, :c], g["irr_z"][i, :c], (g["n_left"][i], g["n_main"][i], g["n_right"][i], *g["irr_limits"][i]),
            float(g["curvature"][i]))


def conveyance_at(p, i, h):
    x, z, rough, _ = node_section(p, i)
    return float(IO.friction(x, z, rough, h, 1.0)[3])


def wave(Q0, nt, dt, steady, peak, amp):
    """flow hydrograph: Q0 for `steady` levels, then a sin^2 wave of amplitude amp * Q0 peaking at level `peak`"""
    k = np.arange(nt, dtype=np.float64)
    s = np.clip((k - steady) / max(peak - steady, 1), 0.0, 2.0)
    return Q0 * (1.0 + amp * np.sin(0.5 * np.pi * s) ** 2)


def _problem(geo, h0, Q0, us, ds, nt, dt=300.0, dx=None, theta=0.7, tol=1e-6):
    N = len(h0)
    return O.Problem(geo=geo, h0=np.asarray(h0, dtype=np.float64), Q0=np.broadcast_to(np.asarray(Q0, dtype=np.float64), (N,)).copy(),
                     us=us, ds=ds, theta=theta, dt=dt, dx=dx, nt=nt, tol=tol)


# ---- a) on_vertex ------------------------------------------------------------------------------------------------------------
def on_vertex(N, rng, fixed=False, nt=6):
    dx = 256.0
    S0 = BED_STEP / dx
    # shape on the 2^-6 grid, thalweg at 0; the water surface sits on vertex `jv` (a bank vertex)
    xs = np.array([0.0, 6.0, 11.0, 15.0, 19.0, 26.0, 33.0, 38.0, 44.0, 52.0])
    zs = np.round(np.array([6.0, 3.1, 1.9, 0.55, 0.0, 0.25, 0.9, 1.9, 3.4, 6.2]) * 64 + rng.integers(-4, 5, 10)) * Q64
    zs[4] = 0.0
    jv = int(rng.choice([2, 6, 7]))
    h0 = float(zs[jv])
    rough = np.tile([0.05, 0.032, 0.06, xs[2], xs[7]], (N, 1))
    bed = BED_STEP * (N - 1 - np.arange(N))
    geo = polyline_geo([xs] * N, [b + zs for b in bed], rough)
    assert np.all(geo["z_bed"] + h0 == geo["irr_z"][:, jv]), "stage not on the vertex bit for bit"
    p = _problem(geo, np.full(N, h0), 1.0, None, None, nt, dx=dx)
    Q0 = conveyance_at(p, N - 1, h0) * np.sqrt(S0)
    p.Q0[:] = Q0
    p.us = O.BC("flow_hydrograph", bed_level=float(geo["z_bed"][0]), target=wave(Q0, nt, p.dt, 2, nt - 1, 0.5))
    if fixed:
        p.ds = O.BC("fixed_depth", bed_level=float(geo["z_bed"][-1]), initial_depth=h0)
    else:
        p.ds = O.BC("normal_depth", bed_level=float(geo["z_bed"][-1]), bed_slope=S0)
    return p


# ---- b) near_vertex_mixed ----------------------------------------------------------------------------------------------------
OFFSETS = (0.0, 5e-7, -5e-7, 2e-6, -2e-6, None)       # None: mid-interval


def near_vertex_mixed(N, rng, nt=4):
    dx, S0 = 300.0, 3e-4
    D = 1.3                       # depth of the vertex every section has at the target surface
    xs, zs, stage = [], [], np.empty(N)
    for i in range(N):
        x = np.cumsum(np.concatenate(([0.0], rng.uniform(3.0, 9.0, 9))))
        z = np.array([5.0, 2.8, D, 0.6, 0.0, 0.4, 0.9, D + 0.4, 3.0, 5.5]) + np.concatenate(([0, 0], [0], rng.uniform(-0.15, 0.15, 4), [0], rng.uniform(-0.2, 0.2, 2)))
        z[4] = 0.0
        z = z + S0 * dx * (N - 1 - i)
        xs.append(x); zs.append(z)
        off = OFFSETS[int(rng.integers(0, len(OFFSETS)))]
        vtx = float(z[2])           # the vertex at depth D above this node's thalweg
        stage[i] = vtx + (0.5 * (z[7] - vtx) if off is None else off)
    rough = np.array([[0.05, rng.uniform(0.028, 0.036), 0.06, x[2], x[7]] for x in xs])
    geo = polyline_geo(xs, zs, rough)
    h0 = stage - geo["z_bed"]
    p = _problem(geo, h0, 1.0, None, None, nt, dx=dx)
    Q0 = conveyance_at(p, N - 1, D) * np.sqrt(S0)
    p.Q0[:] = Q0
    p.us = O.BC("flow_hydrograph", bed_level=float(geo["z_bed"][0]), target=wave(Q0, nt, p.dt, 1, nt - 1, 0.3))
    p.ds = O.BC("normal_depth", bed_level=float(geo["z_bed"][-1]), bed_slope=S0)
    return p


# ---- c) many_stations --------------------------------------------------------------------------------------------------------
def _surveyed(n, rng):
    """a surveyed-looking section of n stations: flat berms, vertical walls, elevations closer than 1e-6, thalweg at 0"""
    t = np.linspace(-1.0, 1.0, n)
    z = 5.0 * t ** 2 + 0.08 * np.sin(7 * t + rng.uniform(0, 6)) + rng.uniform(0, 0.05, n)
    x = 60.0 * (t + 1.0) + np.concatenate(([0.0], np.cumsum(rng.uniform(0.0, 0.05, n - 1))))
    for b in rng.choice(np.arange(3, n - 6), size=max(2, n // 24), replace=False):
        k = int(rng.integers(2, 4))           # flat berm: k + 1 equal elevations
        z[b:b + k + 1] = z[b]
    for w in rng.choice(np.arange(2, n - 2), size=max(1, n // 40), replace=False):
        x[w + 1] = x[w]                       # vertical wall: repeated station
    for c in rng.choice(np.arange(1, n - 2), size=max(1, n // 30), replace=False):
        z[c + 1] = z[c] + 3e-7                # two elevations closer than 1e-6
    x = np.maximum.accumulate(x)
    z -= z.min()
    return x, z


def many_stations(n_st, N, rng, nt=3):
    dx, S0 = 300.0, 2e-4
    xs, zs, rough = [], [], []
    for i in range(N):
        n = n_st - int(rng.integers(0, max(2, n_st // 8)))      # a different vertex count per node, padded to the widest
        x, z = _surveyed(n, rng)
        z = z + S0 * dx * (N - 1 - i)
        xs.append(x); zs.append(z)
        # left limit between two stations, right limit on one
        a = int(n * 0.3)
        rough.append([0.05, 0.031, 0.06, 0.5 * (x[a] + x[a + 1]), x[int(n * 0.7)]])
    geo = polyline_geo(xs, zs, rough)
    h0 = np.full(N, 1.1) + rng.uniform(-0.05, 0.05, N)
    p = _problem(geo, h0, 1.0, None, None, nt, dx=dx)
    Q0 = conveyance_at(p, N - 1, 1.1) * np.sqrt(S0)
    p.Q0[:] = Q0
    p.us = O.BC("flow_hydrograph", bed_level=float(geo["z_bed"][0]), target=wave(Q0, nt, p.dt, 1, nt - 1, 0.4))
    p.ds = O.BC("normal_depth", bed_level=float(geo["z_bed"][-1]), bed_slope=S0)
    return p


# ---- d) multi_run ------------------------------------------------------------------------------------------------------------
def multi_run(N, rng, nt=8):
    """main channel between two levees with a secondary channel behind each; the left bank ends low (a run that touches
    vertex 0 once the stage passes it), an isolated wet vertex in the right levee's crest, the right channel reaches vertex n-1"""
    dx, S0 = 300.0, 2.5e-4
    crest = 1.8
    base_x = np.array([0.0, 6, 12, 16, 20, 24, 32, 36, 40, 44, 47, 50, 54, 60, 64.0])
    base_z = np.array([0.9, 0.6, 1.2, crest, 1.0, 0.2, 0.0, 0.3, 1.1, crest + 0.3, 1.5, crest + 0.3, 0.9, 0.4, 0.5])
    xs, zs = [], []
    for i in range(N):
        z = base_z.copy()
        z[[1, 5, 7, 12, 13]] += rng.uniform(-0.05, 0.05, 5)
        z = z + S0 * dx * (N - 1 - i)
        xs.append(base_x * (1 + 0.002 * i)); zs.append(z)
    rough = np.array([[0.05, 0.032, 0.055, x[3], x[9]] for x in xs])
    geo = polyline_geo(xs, zs, rough)
    # initial stage exactly at the left levee crest (a vertex elevation: the crest's edges are dropped), below the
    # right one: wetted runs left channel + main channel + right channel = 3 (the isolated vertex in the crest stays dry)
    stage = np.array([z[3] for z in zs])
    h0 = stage - geo["z_bed"]
    p = _problem(geo, h0, 1.0, None, None, nt, dx=dx)
    Q0 = conveyance_at(p, N - 1, float(h0[-1])) * np.sqrt(S0)
    p.Q0[:] = Q0
    # the wave lifts the stage over both crests (1 run) and the isolated vertex becomes wet in between
    p.us = O.BC("flow_hydrograph", bed_level=float(geo["z_bed"][0]), target=wave(Q0, nt, p.dt, 1, nt - 2, 2.5))
    p.ds = O.BC("normal_depth", bed_level=float(geo["z_bed"][-1]), bed_slope=S0)
    return p


# ---- e) overtopped_shallow ---------------------------------------------------------------------------------------------------
def overtopped_shallow(N, rng, nt=10):
    """every node starts in its lowest interval (a wide bottom: the first vertex above the thalweg is 0.4 m up); the wave lifts
    the stage over the low right bank (the stage passes the end vertex: a run that touches vertex n-1) and, in the upstream
    quarter, over every vertex (interval K-1, no upper bound)"""
    dx, S0 = 100.0, 3e-4
    xs, zs = [], []
    for i in range(N):
        f = i / max(N - 1, 1)
        x = np.array([0.0, 5, 9, 14, 40, 47, 53.0])
        if f < 0.25:       # low all round: the stage at the peak passes every vertex
            z = np.array([0.49, 0.45, 0.42, 0.0, 0.4, 0.44, 0.48])
        else:
            z = np.array([2.5, 1.2, 0.6, 0.0, 0.4, 0.42, 0.45])
        z = z + rng.uniform(0, 0.01, 7) * (np.arange(7) != 3)
        xs.append(x * (1 + 0.01 * f)); zs.append(z + S0 * dx * (N - 1 - i))
    rough = np.array([[0.045, 0.03, 0.05, x[1], x[5]] for x in xs])
    geo = polyline_geo(xs, zs, rough)
    h0 = np.full(N, 0.3)
    p = _problem(geo, h0, 1.0, None, None, nt, dx=dx, dt=900.0)
    Q0 = conveyance_at(p, N - 1, 0.3) * np.sqrt(S0)
    p.Q0[:] = Q0
    p.us = O.BC("flow_hydrograph", bed_level=float(geo["z_bed"][0]), target=wave(Q0, nt, p.dt, 1, nt - 1, 5.0))
    p.ds = O.BC("normal_depth", bed_level=float(geo["z_bed"][-1]), bed_slope=S0)
    return p


BUILDERS = dict(on_vertex=on_vertex, on_vertex_fixed=lambda N, rng, **k: on_vertex(N, rng, fixed=True, **k),
                near_vertex_mixed=near_vertex_mixed, multi_run=multi_run, overtopped_shallow=overtopped_shallow,
                stations48=lambda N, rng, **k: many_stations(48, N, rng, **k),
                stations120=lambda N, rng, **k: many_stations(120, N, rng, **k),
                stations250=lambda N, rng, **k: many_stations(250, N, rng, **k))


# A Newton norm this close to the tolerance makes the iteration count hinge on the last bits.  (The reference's Newton loop
# contracts the norm by only ~6x per iteration on these channels: a factor-2 margin on either side would reject ~3/4 of all
# levels and no draw of more than a few levels would pass.  Device and oracle norms agree to ~1e-9 relative.)
FRAGILE = 1.25


def fragile(run, tol):
    return any(tol / FRAGILE < e < tol * FRAGILE for _, e in run["norms"])


TOL_SCALE = (1.0, 0.6, 1.7, 0.35, 3.0, 0.2)


def make(kind, N, seed, tries=6, **kw):
    """(Problem, oracle run) of a case: the first draw from (seed, seed + 1, ...) x (tolerance 1e-6 scaled by TOL_SCALE) that
    converges with no fragile norm"""
    for s in range(seed, seed + tries):
        for f in TOL_SCALE:
            p = BUILDERS[kind](N, np.random.default_rng(s), **kw)
            p.tol *= f
            r = O.newton_run(p, trace=True, iterates=True)
            if r["status"] != 0:
                log.warning("poly_edges: %s N=%d seed %d tol %.2g rejected (status %d)", kind, N, s, p.tol, r["status"])
                break
            if fragile(r, p.tol):
                log.warning("poly_edges: %s N=%d seed %d tol %.2g rejected (a Newton norm within %.2fx of tol)", kind, N, s, p.tol, FRAGILE)
                continue
            return p, r
    raise RuntimeError(f"poly_edges: no usable draw for {kind} N={N} in seeds {seed}..{seed + tries - 1}")


# the cases of the CPU census and the stage-table test (kind, N, seed): small enough for the numpy oracle
CENSUS = [("on_vertex", 24, 1), ("on_vertex_fixed", 24, 2), ("near_vertex_mixed", 64, 3), ("multi_run", 20, 4),
          ("overtopped_shallow", 24, 5), ("stations48", 16, 6), ("stations120", 8, 7), ("stations250", 6, 8)]
