"""The channels of tests/poly_edges.py do what they claim: every node evaluation of their oracle runs (the old-level state and
every Newton iterate) is classified by the rules the device follows (flow-sim_amd/csrc/fs_poly.hpp), and each path must be
reached a minimum number of times - so that a later edit of the generator cannot quietly drop the coverage.

  1 hinted      node_terms_poly_hinted: the stage stays inside the interval of the node's last table evaluation
                (ZLO < hw - 1e-6, ZHI > hw + 1e-6, fewer than two wetted runs)
  2 scan        poly_eval_whole with more than one round of the breakpoint scan (KP > 16) and a table block
  3 edge walk   `c1 != c2`: a vertex elevation within 1e-6 of the stage, or on it
  4 sub-channel two or more wetted runs of >= 2 vertices: the walk over temporary sub-sections
  6 outside     the lowest interval (below every vertex but the lowest) or the top one (above every vertex, ZHI = inf)
(path 5, the table-less walk, is a mode of the whole batch: tests/test_gpu_polyline_paths.py runs every case with
FS_POLY_WALK=1.)

The census APPROXIMATES the device, it does not reproduce it: it evaluates the old-level state once per level (kernels that keep
the level's terms evaluate it once, at the start of the launch), it keeps one hint per node (the device keeps one per lane slot,
khint[M + 1]), and mixed_wave groups nodes into waves by the lane layout of one workgroup pass.  The counts are a lower bound on
what the generator produces, not a trace of a kernel."""
import numpy as np
import pytest

from oracle import irregular_oracle as IO

import poly_edges as PE

DH = 1e-6
SHAPES = [(2, 1), (8, 1), (8, 4), (4, 4)]       # (cells per lane, waves per reach) of the polyline entries


def node_info(p, i):
    x, z, _, _ = PE.node_section(p, i)
    lev = np.unique(z)
    K = len(lev)
    # wetted runs of >= 2 vertices in each interval (fixed inside it: the build_stage_table count)
    nsub = [len(IO.subchannels(x, z, lev[k] + (0.5 * (lev[k + 1] - lev[k]) if k + 1 < K else 1.0))) for k in range(K)]
    return lev, nsub, (len(x) + 16) & ~15


def census(p, run):
    """counts per path and, per iteration, the path of every node ('walk' 3 / 'table' 1, 2 / other)"""
    info = [node_info(p, i) for i in range(p.N)]
    hint = [-1] * p.N
    counts = {1: 0, 2: 0, 3: 0, 4: 0, 6: 0}
    per_iter = []

    def evaluate(i, h):
        lev, nsub, KP = info[i]
        hw = h + lev[0]
        kh = hint[i]
        if kh >= 0:
            zhi = lev[kh + 1] if kh + 1 < len(lev) else np.inf
            if lev[kh] < hw - DH and zhi > hw + DH and nsub[kh] < 2:
                counts[1] += 1
                counts[6] += kh == 0 or kh == len(lev) - 1
                return 1
        c1 = int(np.sum(lev < hw - DH)); c2 = int(np.sum(lev <= hw + DH))
        if c1 != c2:
            counts[3] += 1
            counts[4] += len(IO.subchannels(*PE.node_section(p, i)[:2], hw)) >= 2
            hint[i] = -1
            return 3
        k = c1 - 1
        counts[2] += KP > 16
        counts[6] += k == 0 or k == len(lev) - 1
        if k >= 0 and nsub[k] >= 2:
            counts[4] += 1
            hint[i] = -1
            return 4
        hint[i] = k
        return 2

    last = 0
    for k, h_old, h in run["iterates"]:
        if k != last:                 # a new level: its old-level state is evaluated once
            for i in range(p.N):
                evaluate(i, h_old[i])
            last = k
        per_iter.append(np.array([evaluate(i, h[i]) for i in range(p.N)]))
    return counts, per_iter


def mixed_wave(per_iter, M, W):
    """an iteration where one wave has a lane on the edge walk and another on a table path, at the same local row"""
    for paths in per_iter:
        N = len(paths)
        for r in range(M):
            rows = np.arange(r, N, M)                     # local row r of every lane (lane = node // M)
            waves = (rows // M) // 64
            for w in np.unique(waves):
                sel = paths[rows[waves == w]]
                if np.any(sel == 3) and np.any((sel == 1) | (sel == 2)):
                    return True
    return False


_runs = {}


def run_of(spec):
    if spec not in _runs:
        p, r = PE.make(*spec)
        _runs[spec] = (p, r, *census(p, r))
    return _runs[spec]


# per case: the paths it exists for, with a minimum count
CLAIMS = {"on_vertex": {3: 20, 1: 20}, "on_vertex_fixed": {3: 20, 1: 20}, "near_vertex_mixed": {3: 20, 1: 50},
          "multi_run": {4: 20, 3: 1, 1: 20}, "overtopped_shallow": {6: 20, 1: 20},
          "stations48": {2: 10, 1: 10}, "stations120": {2: 5, 1: 5}, "stations250": {2: 5, 1: 5}}


@pytest.mark.parametrize("spec", PE.CENSUS, ids=[f"{s[0]}-{s[1]}" for s in PE.CENSUS])
def test_case_reaches_its_paths(spec):
    p, r, counts, _ = run_of(spec)
    print(spec[0], counts)
    for path, n in CLAIMS[spec[0]].items():
        assert counts[path] >= n, (spec, path, counts)


def test_on_vertex_starts_on_the_vertex_bit_for_bit():
    for kind in ("on_vertex", "on_vertex_fixed"):
        p, r, _, _ = run_of(next(s for s in PE.CENSUS if s[0] == kind))
        hw = p.h0 + p.geo["z_bed"]
        assert all(np.any(p.geo["irr_z"][i] == hw[i]) for i in range(p.N))
        # downstream nodes stay within 1e-6 of the vertex while the wave is upstream: the walk path at every level there
        assert np.all(np.abs(r["depth"][:3, -1] - p.h0[-1]) < DH)


def test_multi_run_crosses_one_two_three_runs():
    p, r, _, _ = run_of(next(s for s in PE.CENSUS if s[0] == "multi_run"))
    seen = set()
    for _, _, h in r["iterates"]:
        for i in range(p.N):
            x, z, _, _ = PE.node_section(p, i)
            seen.add(len(IO.subchannels(x, z, h[i] + z.min())))
    assert {1, 2, 3} <= seen, seen


def test_every_path_is_reached_and_waves_mix():
    total = {1: 0, 2: 0, 3: 0, 4: 0, 6: 0}
    for spec in PE.CENSUS:
        for k, v in run_of(spec)[2].items():
            total[k] += v
    assert all(v >= 20 for v in total.values()), total
    _, _, _, per_iter = run_of(next(s for s in PE.CENSUS if s[0] == "near_vertex_mixed"))
    for M, W in SHAPES:
        assert mixed_wave(per_iter, M, W), (M, W)
