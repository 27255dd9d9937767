"""What the envelope tests share (tests/test_gpu_envelope.py, tests/test_gpu_postprocess_geometry.py): numpy's crossings, the six
quantities of a batch from its history and fs_batch_derive, the bit-for-bit comparison of an envelope with numpy on them, the checks of
fs_batch_profile_bands against numpy on a downloaded row, and a ragged batch of prismatic reaches."""
import numpy as np

from flowsim_amd import BoundarySpec, PreissmannBatch
from flowsim_amd import _abi as A
from synth import rect_problem

EPS = 2.0 ** -52
STEPS = 5


def crossings_of(x, thr):
    """numpy's first / last / count of x[k] >= thr along axis 0 (-1, -1, 0: never)"""
    hit = x >= thr
    n = x.shape[0]
    count = hit.sum(axis=0)
    first = np.where(count > 0, np.argmax(hit, axis=0), -1)
    last = np.where(count > 0, n - 1 - np.argmax(hit[::-1], axis=0), -1)
    return first, last, count


def fields_of(b, first, n):
    """name -> [n, B, N] of the six quantities from the batch's history and fs_batch_derive"""
    h, Q = b.history_arrays(first, n)
    d = b.derive(first, n, fields=("level", "velocity", "froude_number", "top_width"))
    return dict(depth=h, stage=d["level"], flow=Q, velocity=d["velocity"], froude_number=d["froude_number"], top_width=d["top_width"])


def assert_envelope_is_numpy_on(env, x, name, where=None, what=""):
    """bit for bit: env[name] against np.max / argmax / min / argmin over axis 0 of x [n, B, N] (where: a [B, N] mask)"""
    where = np.ones(x.shape[1:], dtype=bool) if where is None else where
    e = env[name]
    assert np.array_equal(e["max"][where], np.max(x, axis=0)[where]), (what, name, "max")
    assert np.array_equal(e["min"][where], np.min(x, axis=0)[where]), (what, name, "min")
    assert np.array_equal(e["max_level"][where], np.argmax(x, axis=0)[where]), (what, name, "max_level")
    assert np.array_equal(e["min_level"][where], np.argmin(x, axis=0)[where]), (what, name, "min_level")


def ragged_batch(lengths, dtype, n_steps=STEPS, seed=900, N=None):
    """one RECT_UNIFORM batch of prismatic reaches of these node counts in rows of N (the longest reach's count unless given)"""
    probs = [rect_problem(n, seed=seed + s, n_steps=n_steps) for s, n in enumerate(lengths)]
    B, N, p0 = len(probs), N or max(lengths), probs[0]
    b = PreissmannBatch(B, N, p0.nt, dtype=dtype, section_mode="rect_uniform", history=True)
    b.set_scheme(p0.theta, p0.dt, p0.dx, 1e-3 if dtype == "f32" else p0.tol, p0.max_iter)
    b.set_geometry_uniform([p.geo["b_main"][0] for p in probs], [p.geo["n_main"][0] for p in probs], [p.geo["z_bed"][0] for p in probs],
                           [p.geo["z_bed"][-1] for p in probs])
    b.set_reach_nodes(list(lengths))
    b.set_boundary(A.UPSTREAM, BoundarySpec(A.BC_FLOW_HYDROGRAPH, {}, np.stack([p.us.target for p in probs], axis=1)))
    b.set_boundary(A.DOWNSTREAM, BoundarySpec(A.BC_NORMAL_DEPTH, dict(bed_slope=np.array([p.ds.bed_slope for p in probs]), bed_level=np.zeros(B))))
    pad = lambda a: np.concatenate([a, np.full(N - len(a), -777.0)])
    b.set_state(np.stack([pad(p.h0) for p in probs]), np.stack([pad(p.Q0) for p in probs]))
    return b


def check_profile(b, x, enters, quantity, stat, counts=None):
    """profile_bands of one row against numpy on the downloaded row x [B, N]; enters [B, N]: the members numpy keeps at each node;
    counts [B, N]: the downloaded crossing counts (exceed is then held to the counted fraction).  The bars are those of
    tests/test_gpu_reduce.py: min, max and order statistics exact, quantiles between their neighbours and within 4 eps of numpy's,
    mean and std within (m + 2) eps max|x|."""
    B, N = x.shape
    levels = (0.05, 0.5, 0.95, 0.0, 1.0)
    got = b.profile_bands(quantity, stat, levels)
    only = b.profile_bands(quantity, stat, ())
    assert only["quantiles"].shape == (N, 0) and got["quantiles"].shape == (N, 5)
    for k in ("min", "max", "mean", "std"):
        assert np.array_equal(only[k], got[k], equal_nan=True)
    m_max = int(enters.sum(axis=0).max())
    ks = []
    if m_max > 1:
        ks = [k for k in sorted(set(np.linspace(0, m_max - 1, A.BANDS_MAX_Q).astype(int).tolist() + [1, m_max - 2])) if 0 <= k <= m_max - 1]
        ks = [k for k in ks if (m_max - 1) * (k / (m_max - 1)) == k][:A.BANDS_MAX_Q]
        assert len(ks) >= min(m_max, 3)
        on_samples = b.profile_bands(quantity, stat, [k / (m_max - 1) for k in ks])
    for node in range(N):
        v = x[enters[:, node], node]
        m = len(v)
        assert got["n_members"][node] == m, node
        if m == 0:
            assert all(np.isnan(got[k][node]) for k in ("min", "max", "mean", "std")) and np.all(np.isnan(got["quantiles"][node]))
            assert got["exceed"] is None or np.isnan(got["exceed"][node])
            continue
        srt, big = np.sort(v), np.max(np.abs(v))
        assert got["min"][node] == srt[0] and got["max"][node] == srt[-1], node
        assert abs(got["mean"][node] - np.mean(v)) <= (m + 2) * EPS * big, node
        assert abs(got["std"][node] - np.std(v)) <= (m + 2) * EPS * big, node
        assert got["quantiles"][node, 3] == srt[0] and got["quantiles"][node, 4] == srt[-1], node
        for i, q in enumerate(levels[:3]):
            vi = (m - 1) * q
            a, c = srt[int(np.floor(vi))], srt[min(int(np.floor(vi)) + 1, m - 1)]
            g = got["quantiles"][node, i]
            assert a <= g <= c, (node, q)
            assert abs(g - np.quantile(v, q)) <= 4 * EPS * max(abs(a), abs(c)), (node, q)
        if m == m_max and ks:
            for i, k in enumerate(ks):
                assert on_samples["quantiles"][node, i] == srt[k], (node, k)
        if counts is not None:
            assert got["exceed"][node] == np.sum(counts[enters[:, node], node] > 0) / m, node
    return got
