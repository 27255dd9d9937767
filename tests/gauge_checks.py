"""What the gauge tests share (tests/test_gauge_host.py, tests/test_gpu_gauges.py): a sequential Python restatement of fs::score_series
(flow-sim_amd/csrc/fs_gauge.hpp) - the walk of one member's series of one gauge signal against its observations - that the host driver
and the device are held to bit for bit, the same scores from vectorised numpy with the bar their sums are held to, and numpy's gauge
rows from the fields fs_batch_derive and the history give."""
import math

import numpy as np

GS_ROWS = ("count", "bias", "rmse", "nse", "peak_sim", "peak_sim_level", "peak_error", "peak_lag")
NAN = float("nan")
EPS = 2.0 ** -52


def score_series(marked, sim, obs):
    """dict of GS_ROWS: the two walks in level order, every operation one float64 operation (Python floats do not fuse).  A level
    counts when it is marked and observed (obs not NaN); the peaks are first-index maxima, a NaN simulated value takes the peak at
    its first level and keeps it (np.max / np.argmax)."""
    f = np.float64
    cnt, ls, lo = 0, -1, -1
    sum_o, ps, po = f(0.0), f(0.0), f(0.0)
    counted = []
    for k in range(len(marked)):
        if not marked[k] or obs[k] != obs[k]:
            continue
        s, o = f(sim[k]), f(obs[k])
        if cnt == 0 or (ps == ps and not (s <= ps)):
            ps, ls = s, k
        if cnt == 0 or o > po:
            po, lo = o, k
        sum_o = sum_o + o
        cnt += 1
        counted.append(k)
    if cnt == 0:
        return dict(count=0.0, bias=NAN, rmse=NAN, nse=NAN, peak_sim=NAN, peak_sim_level=-1.0, peak_error=NAN, peak_lag=NAN)
    mean_o = sum_o / f(cnt)
    se, sq, so = f(0.0), f(0.0), f(0.0)
    for k in counted:
        e, d = f(sim[k]) - f(obs[k]), f(obs[k]) - mean_o
        se = se + e
        sq = sq + e * e
        so = so + d * d
    with np.errstate(divide="ignore", invalid="ignore"):
        nse = f(1.0) - sq / so
    with np.errstate(invalid="ignore"):
        return dict(count=float(cnt), bias=float(se / f(cnt)), rmse=math.sqrt(sq / f(cnt)) if sq == sq else NAN, nse=float(nse), peak_sim=float(ps),
                    peak_sim_level=float(ls), peak_error=float(ps - po), peak_lag=float(ls - lo))


def score_numpy(marked, sim, obs):
    """(scores, bars) by vectorised numpy over the counted levels; bars: the (m + 2) eps scale by which a sequential sum may differ from
    numpy's pairwise one, per row (0: exact).  Series without a NaN simulated value at a counted level only."""
    marked, sim, obs = np.asarray(marked, dtype=bool), np.asarray(sim, dtype=np.float64), np.asarray(obs, dtype=np.float64)
    c = marked & ~np.isnan(obs)
    m = int(c.sum())
    if m == 0:
        return score_series(marked, sim, obs), {k: 0.0 for k in GS_ROWS}
    idx = np.flatnonzero(c)
    s, o = sim[idx], obs[idx]
    e = s - o
    mean_o = np.mean(o)
    sq, so = np.sum(e * e), np.sum((o - mean_o) ** 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        nse = 1.0 - sq / so
    got = dict(count=float(m), bias=float(np.mean(e)), rmse=float(np.sqrt(sq / m)), nse=float(nse), peak_sim=float(np.max(s)),
               peak_sim_level=float(idx[np.argmax(s)]), peak_error=float(np.max(s) - np.max(o)), peak_lag=float(idx[np.argmax(s)] - idx[np.argmax(o)]))
    # A sequential sum of m terms differs from the exact one by at most (m - 1) eps sum|t|, numpy's pairwise one by less; with the
    # division (and the root, which halves a relative error) that is (m + 2) eps times the scale: max|e| for bias and rmse (both are
    # at most max|e|).  nse = 1 - sq / so: each sum is relative-(m + 2) eps, and the sequential mean, itself (m + 2) eps max|o| off,
    # moves so only in second order (the deviations sum to zero) - 4 (m + 2) eps max(1, sq / so) covers both sums with a factor two.
    bar = (m + 2) * EPS
    big_e = float(np.max(np.abs(e)))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(sq / so)
    bars = dict(count=0.0, bias=bar * big_e, rmse=bar * big_e, nse=4 * bar * max(1.0, ratio) if so > 0 else math.inf,
                peak_sim=0.0, peak_sim_level=0.0, peak_error=0.0, peak_lag=0.0)
    return got, bars


def same(a, b):
    """the same float64, NaN being one value"""
    return (a != a and b != b) or a == b


def rows_numpy(fields, node, weight, nodes=None):
    """[n, 4, B]: numpy's gauge rows (depth, flow, stage, velocity) at (node, weight) - scalars, or [B] per reach - from `fields`
    (envelope_checks.fields_of: name -> [n, B, N]); a + w (b - a) in float64, a itself where w == 0, NaN where the reach of `nodes`
    [B] nodes does not have the gauge"""
    n, B, N = fields["depth"].shape
    node = np.broadcast_to(np.asarray(node), (B,))
    weight = np.broadcast_to(np.asarray(weight, dtype=np.float64), (B,))
    nodes = np.full(B, N) if nodes is None else np.asarray(nodes)
    out = np.full((n, 4, B), NAN)
    for r in range(B):
        i, w = int(node[r]), float(weight[r])
        if i >= nodes[r] or (w != 0.0 and i + 1 >= nodes[r]):
            continue
        for q, name in enumerate(("depth", "flow", "stage", "velocity")):
            a = fields[name][:, r, i]
            if w == 0.0:
                out[:, q, r] = a
            else:
                with np.errstate(invalid="ignore"):
                    out[:, q, r] = a + w * (fields[name][:, r, i + 1] - a)
    return out
