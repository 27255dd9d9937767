"""The derived fields of a history (Solver.prepare_results, solver.py:65-127) and the six envelope quantities, in numpy float64 from
the oracle's own section functions: the reference the post-processing kernels (flow-sim_amd/csrc/fs_derive.hpp, fs_envelope.hpp)
are held to on ANY history - the device's own included, so that a test of them tests them and not the solver.
tests/test_derived_reference.py holds this module to the reference's prepare_results arrays of the golden fixtures.

derived_f32 restates the trapezoid-family formulas operation by operation in numpy float32: the rounding noise of an honest fp32
implementation, from which tests/test_gpu_postprocess_geometry.py takes its fp32 bars.  surface_census counts the polyline edge
cases a history reaches: surfaces that sit on a vertex bit for bit, and the wetted runs."""
import numpy as np

from oracle import irregular_oracle as IO
from oracle import preissmann_oracle as O

FIELDS = ("level", "area", "top_width", "froude_number", "velocity", "wave_celerity", "amplitude", "peak_amplitude")
QUANTITIES = ("depth", "stage", "flow", "velocity", "froude_number", "top_width")       # flowsim_amd._abi.ENV_QUANTITIES


def polyline_nodes(geo):
    """[(node, x, z)] of the polyline nodes of one channel's geo dict (none: a trapezoid-family channel)"""
    if "irr_npts" not in geo:
        return []
    cnt = np.asarray(geo["irr_npts"])
    return [(int(i), np.asarray(geo["irr_x"][i, :cnt[i]], dtype=np.float64), np.asarray(geo["irr_z"][i, :cnt[i]], dtype=np.float64))
            for i in np.flatnonzero(cnt > 0)]


def area_top(geo, h):
    """(A, T) [n, N] at the depths h [n, N] of ONE channel: section_props at the trapezoid-family nodes, the polyline below the
    stage h + z_bed where irr_npts > 0"""
    h = np.asarray(h, dtype=np.float64)
    rows = {k: np.asarray(geo[k], dtype=np.float64) for k in O.GEO_KEYS if k in geo}
    A, _, _, T, _ = O.section_props(rows, h)
    A, T = np.array(A, dtype=np.float64), np.array(T, dtype=np.float64)
    for i, x, z in polyline_nodes(geo):
        for k in range(h.shape[0]):
            A[k, i], _, _, T[k, i] = IO.properties(x, z, h[k, i] + rows["z_bed"][i])
    return A, T


def derived(geo, h, Q):
    """name -> [n, N] float64 (peak_amplitude: [N]) of FIELDS for the history h, Q [n, N] of one channel; row 0 is the amplitudes'
    reference, as in the reference"""
    h, Q = np.asarray(h, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    A, T = area_top(geo, h)
    with np.errstate(divide="ignore", invalid="ignore"):
        V = Q / A
        c = V + np.sqrt(O.G * A / T)
    amplitude = h - h[0]
    return dict(level=h + np.asarray(geo["z_bed"], dtype=np.float64), area=A, top_width=T, froude_number=O.froude(T, A, Q), velocity=V,
                wave_celerity=c, amplitude=amplitude, peak_amplitude=amplitude.max(axis=0))


def envelope(geo, h, Q):
    """name -> dict(series [n, N], max, min [N], max_level, min_level [N]: np.argmax / np.argmin) of QUANTITIES"""
    d = derived(geo, h, Q)
    series = dict(depth=np.asarray(h, dtype=np.float64), stage=d["level"], flow=np.asarray(Q, dtype=np.float64), velocity=d["velocity"],
                  froude_number=d["froude_number"], top_width=d["top_width"])
    return {q: dict(series=x, max=np.max(x, axis=0), max_level=np.argmax(x, axis=0), min=np.min(x, axis=0), min_level=np.argmin(x, axis=0))
            for q, x in series.items()}


def surface_census(geo, h):
    """(on_vertex, runs) [n, N] of the polyline nodes of a channel at the depths h (trapezoid-family nodes: False, 0): whether the
    stage h + z_bed equals a vertex elevation bit for bit, and the number of wetted runs (runs of vertices strictly below it)"""
    h = np.asarray(h, dtype=np.float64)
    on, runs = np.zeros(h.shape, dtype=bool), np.zeros(h.shape, dtype=np.int64)
    for i, _, z in polyline_nodes(geo):
        for k in range(h.shape[0]):
            hw = h[k, i] + float(geo["z_bed"][i])
            below = (hw - z) > 0.0
            on[k, i] = bool(np.any(z == hw))
            runs[k, i] = int(below[0]) + int(np.sum(below[1:] & ~below[:-1]))
    return on, runs


def uniform_geo(width, z_us, z_ds, n_nodes, side_slope=0.0, dtype=np.float64):
    """geo rows of a prismatic reach as the uniform modes define it (cross_section.py:887-900: the bed interpolated over the reach's
    own nodes), evaluated in dtype from parameters rounded to dtype"""
    R = dtype
    w2 = np.arange(n_nodes).astype(R) / R(n_nodes - 1)
    z = R(z_us) * (R(1) - w2) + R(z_ds) * w2
    zero = np.zeros(n_nodes, dtype=R)
    return dict(z_bed=z, b_main=np.full(n_nodes, R(width)), m_main=np.full(n_nodes, R(side_slope)), is_compound=zero, h_bf=zero,
                b_fp_l=zero, b_fp_r=zero, m_fp=zero)


def derived_f32(geo, h, Q):
    """derived() of a trapezoid-family channel with every operation in numpy float32, on geometry rounded to float32 first; h, Q
    [n, N] float32.  name -> [n, N] float32"""
    R = np.float32
    assert not polyline_nodes(geo), "polylines are evaluated in fp64 only"
    h, Q = np.asarray(h), np.asarray(Q)
    assert h.dtype == R and Q.dtype == R
    g = {k: np.asarray(geo[k]).astype(R) for k in ("z_bed", "b_main", "m_main", "h_bf", "b_fp_l", "b_fp_r", "m_fp")}
    comp = np.asarray(geo["is_compound"]) > 0.5
    b, m, hb, mfp = g["b_main"], g["m_main"], g["h_bf"], g["m_fp"]
    d = np.maximum(R(0), h)
    T = b + R(2) * m * d
    A = (b + T) / R(2) * d
    over = comp & (d > hb)
    dfp = d - hb
    Tb = b + R(2) * m * hb
    A_over = (b + Tb) / R(2) * hb + (g["b_fp_l"] + R(0.5) * mfp * dfp) * dfp + (g["b_fp_r"] + R(0.5) * mfp * dfp) * dfp
    T_over = (g["b_fp_l"] + Tb + g["b_fp_r"]) + R(2) * mfp * dfp
    A, T = np.where(over, A_over, A), np.where(over, T_over, T)
    dry = d <= R(0)
    A, T = np.where(dry, R(0), A), np.where(dry, R(0), T)
    with np.errstate(divide="ignore", invalid="ignore"):
        V = Q / A
        c = V + np.sqrt(R(O.G) * A / T)
        Fr = (Q / np.maximum(A, R(1e-6))) / np.sqrt(R(O.G) * np.maximum(A / np.maximum(T, R(1e-6)), R(1e-6)))
    amplitude = h - h[0]
    out = dict(level=h + g["z_bed"], area=A, top_width=T, froude_number=Fr, velocity=V, wave_celerity=c, amplitude=amplitude,
               peak_amplitude=amplitude.max(axis=0))
    assert all(v.dtype == R for v in out.values())
    return out
