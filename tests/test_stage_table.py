"""The polyline stage tables (flow-sim_amd/csrc/fs_stage_table.hpp) built on the CPU, under AddressSanitizer and UBSan, and
checked coefficient by coefficient against the CPU oracle (oracle/irregular_oracle.py) - until now the tables were only checked
through the end-to-end GPU comparison.

tests/stage_table/stage_table_driver.cpp runs the very builder and node-minor packing that fs_host_pack.hpp (pack_polylines) runs;
the sections are those of tests/poly_edges.py (vertices exactly on a breakpoint, flat berms, vertical walls, elevations closer
than 1e-6, strip limits on and between stations, up to 245 stations) plus the three reference-generated irr_* fixtures.  For
every node, every interval and three stages inside it: A, P, T and each roughness strip's (A, P) against properties() of the
polyline and of the strip's sub-polyline, the number of wetted runs against subchannels(), the interval bounds, the node
constants, the +inf padding, and un-packing the device layout gives back each node's block."""
import os
import shutil

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from oracle import irregular_oracle as IO
from oracle import preissmann_oracle as O

import host_driver
import poly_edges as PE

DRIVER = os.path.join(ROOT, "tests", "stage_table", "stage_table_driver.cpp")
BLOCK, NSUB, ZLO, ZHI, NL, STRIP = 32, 22, 23, 24, 25, 7
REL = 1e-12


def kp(P):
    return (P + 16) & ~15


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no system C++ compiler")
    return host_driver.build(DRIVER, tmp_path_factory.mktemp("stage_table"))


def build_tables(exe, geo, tmp):
    """(blocks [N, stride], packed device layout [N * stride]) of a channel from the sanitized driver"""
    X, Z, cnt, lim = geo["irr_x"], geo["irr_z"], geo["irr_npts"], geo["irr_limits"]
    N, P = X.shape
    lines = [f"{N} {P}"]
    for i in range(N):
        c = int(cnt[i])
        consts = (lim[i, 0], lim[i, 1], geo["n_left"][i], geo["n_main"][i], geo["n_right"][i], geo["curvature"][i], Z[i, :c].min())
        lines.append(f"{c} " + " ".join(repr(float(v)) for v in consts))
        lines.append(" ".join(repr(float(v)) for v in X[i, :c]))
        lines.append(" ".join(repr(float(v)) for v in Z[i, :c]))
    fin, fout = os.path.join(tmp, "in.txt"), os.path.join(tmp, "out.bin")
    with open(fin, "w") as f:
        f.write("\n".join(lines) + "\n")
    host_driver.run(exe, [fin, fout], timeout=300)
    stride = kp(P) + P * BLOCK
    out = np.fromfile(fout, dtype=np.float64)
    assert out.size == 2 * N * stride
    return out[:N * stride].reshape(N, stride), out[N * stride:]


def unpack(packed, N, P):
    """the device layout (breakpoints [N][KP], intervals [P][BLOCK / 2][N] 16-byte pairs) back to per-node blocks"""
    K = kp(P)
    bp = packed[:N * K].reshape(N, K)
    co = packed[N * K:].reshape(P * BLOCK // 2, N, 2).transpose(1, 0, 2).reshape(N, P * BLOCK)
    return np.concatenate([bp, co], axis=1)


def close(got, want, what, scale=0.0):
    """relative to the value, or to the whole section's (scale) for a strip that holds a sliver of it"""
    assert abs(got - want) <= REL * max(abs(want), scale), (what, got, want)


def check_node(blk, x, z, rough, curv, P):
    K_ = kp(P)
    lev = np.unique(z)
    K = len(lev)
    assert np.array_equal(blk[:K], lev), "breakpoints: the distinct vertex elevations, ascending"
    assert np.all(np.isposinf(blk[K:K_])), "breakpoint padding"
    xa, xb = x[0], x[-1]
    n_l, n_m, n_r, lim_l, lim_r = rough
    strips = [(xa, lim_l), (lim_l, lim_r), (lim_r, xb)]
    for k in range(P):
        co = blk[K_ + k * BLOCK:K_ + (k + 1) * BLOCK]
        assert np.array_equal(co[NL:NL + 5], [n_l, n_m, n_r, curv, z.min()]), ("node constants", k)
        if k >= K:
            assert np.all(co[:NSUB + 1] == 0) and np.isposinf(co[ZLO]) and np.isposinf(co[ZHI]), ("unused interval", k)
            continue
        zlo, zhi = lev[k], (lev[k + 1] if k + 1 < K else np.inf)
        assert co[ZLO] == zlo and (co[ZHI] == zhi), ("bounds", k)
        span = (zhi - zlo) if np.isfinite(zhi) else 1.0
        for frac in (0.1, 0.5, 0.9):
            u = frac * span
            s = zlo + u
            if not (zlo < s < zhi):           # (elevations 3e-7 apart: keep the stage strictly inside the interval)
                continue
            u = s - zlo
            A, Pw, _, T = IO.properties(x, z, s)
            close(co[0] + co[1] * u + co[2] * u * u, A, ("A", k, frac))
            close(co[3] + co[4] * u, Pw, ("P", k, frac))
            close(co[5] + co[6] * u, T, ("T", k, frac))
            for sidx, (lo, hi) in enumerate(strips):
                m = (x >= lo) & (x <= hi)
                As, Ps = IO.properties(x[m], z[m], s)[:2] if m.sum() >= 2 else (0.0, 0.0)
                o = STRIP + 5 * sidx
                close(co[o] + co[o + 1] * u + co[o + 2] * u * u, As, ("strip A", sidx, k, frac), A)
                close(co[o + 3] + co[o + 4] * u, Ps, ("strip P", sidx, k, frac), Pw)
            assert co[NSUB] == len(IO.subchannels(x, z, s)), ("NSUB", k, frac)


def sections():
    out = []
    for kind, N, seed in PE.CENSUS:
        out.append((f"{kind}-{N}", PE.BUILDERS[kind](N, np.random.default_rng(seed)).geo))
    for name in ("irr_single", "irr_levee", "irr_mixed"):
        fx, meta = O.load_fixture(os.path.join(GOLDEN, name + ".npz"))
        p = O.problem_from_fixture(fx, meta)
        g = dict(p.geo)
        poly = g["irr_npts"] > 0
        # trapezoid-family nodes (irr_npts 0) have no table: keep the polyline nodes
        g = {k: (v[poly] if np.ndim(v) >= 1 and len(v) == len(poly) else v) for k, v in g.items()}
        out.append((name, g))
    return out


SECTIONS = sections()


@pytest.mark.parametrize("name,geo", SECTIONS, ids=[s[0] for s in SECTIONS])
def test_stage_table_against_the_oracle(driver, tmp_path, name, geo):
    blocks, packed = build_tables(driver, geo, str(tmp_path))
    N, P = geo["irr_x"].shape
    assert np.array_equal(unpack(packed, N, P), blocks), "node-minor packing does not give back the blocks"
    for i in range(N):
        c = int(geo["irr_npts"][i])
        x, z = geo["irr_x"][i, :c], geo["irr_z"][i, :c]
        rough = (geo["n_left"][i], geo["n_main"][i], geo["n_right"][i], *geo["irr_limits"][i])
        check_node(blocks[i], x, z, rough, float(geo["curvature"][i]), P)


def test_the_sections_hold_the_edges_they_claim():
    """what the mutations of the builder need to show: a strip limit exactly on a station, repeated stations and elevations,
    elevations closer than 1e-6, KP up to 256"""
    geos = dict(SECTIONS)
    on_station = sum(np.any(g["irr_x"][i] == g["irr_limits"][i, 0]) for g in geos.values() for i in range(len(g["irr_npts"])))
    assert on_station > 0
    st = geos["stations250-6"]
    assert kp(st["irr_x"].shape[1]) == 256 and len(set(st["irr_npts"])) > 1
    x, z = st["irr_x"][0, :st["irr_npts"][0]], st["irr_z"][0, :st["irr_npts"][0]]
    assert np.any(np.diff(x) == 0) and np.any(np.diff(z) == 0) and np.any((np.diff(np.unique(z)) < 1e-6))
