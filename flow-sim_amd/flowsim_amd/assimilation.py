"""Assimilation of gauge observations into a running ensemble: what a forecaster puts around PreissmannBatch.assimilate (the analysis
step of a stochastic ensemble Kalman filter, include/flowsim_abi.h: fs_batch_assimilate).  The library draws no random numbers and
knows no distances: the observation perturbations and the localisation taper are made here, on the host, from a seed and chainages."""
from collections import namedtuple

import numpy as np

Observation = namedtuple("Observation", "gauge signal value variance")
Observation.__doc__ = """one observation: gauge (index into the batch's set_gauges), signal (a name or index of _abi.GAUGE_ROWS), the
observed value and its error variance"""


def gaspari_cohn(distance, radius):
    """The compactly supported fifth-order correlation function of Gaspari and Cohn (1999, eq. 4.10) of |distance| / radius: 1 at 0,
    decreasing, 0 from 2 radius on.  distance: any shape (chainage of the nodes minus chainage of the gauge); radius > 0."""
    if not radius > 0.0:
        raise ValueError("gaspari_cohn: radius must be > 0")
    z = np.abs(np.asarray(distance, dtype=np.float64)) / float(radius)
    out = np.zeros_like(z)
    a = z <= 1.0
    b = (z > 1.0) & (z < 2.0)
    za, zb = z[a], z[b]
    out[a] = -0.25 * za ** 5 + 0.5 * za ** 4 + 0.625 * za ** 3 - 5.0 / 3.0 * za ** 2 + 1.0
    out[b] = zb ** 5 / 12.0 - 0.5 * zb ** 4 + 0.625 * zb ** 3 + 5.0 / 3.0 * zb ** 2 - 5.0 * zb + 4.0 - 2.0 / (3.0 * zb)
    return np.clip(out, 0.0, 1.0)


def taper(node_chainage, gauge_chainage, radius):
    """[n_obs, N]: gaspari_cohn of the distance of every node to the gauge of each observation"""
    x, g = np.asarray(node_chainage, dtype=np.float64), np.asarray(gauge_chainage, dtype=np.float64)
    return gaspari_cohn(x[None, :] - g[:, None], radius)


def perturbations(seed, variances, B, active=None):
    """[n_obs, B] draws of N(0, variances[j]) from numpy's default generator seeded with `seed`: the same seed, the same bits.
    active: a boolean mask [B]; the draws are then centred over the active members (their mean is removed, so that the perturbed
    observations average the observation itself) and set to 0 for the others."""
    var = np.asarray(variances, dtype=np.float64)
    if var.ndim != 1 or np.any(~(var >= 0.0)):
        raise ValueError("perturbations: variances is [n_obs], >= 0")
    e = np.random.default_rng(seed).standard_normal((len(var), int(B))) * np.sqrt(var)[:, None]
    if active is not None:
        active = np.asarray(active, dtype=bool)
        if active.shape != (int(B),) or not active.any():
            raise ValueError("perturbations: active is a boolean mask [B] with a member set")
        e = np.where(active[None, :], e - e[:, active].mean(axis=1, keepdims=True), 0.0)
    return np.ascontiguousarray(e)


def cycle(batch, schedule, depth_floor=1e-3):
    """Steps `batch` to each observation level and assimilates there.  schedule: an iterable of (level, observations,
    perturbations, taper) in ascending level order (perturbations and taper may be None); yields (level, diagnostics), the
    diagnostics being what PreissmannBatch.assimilate returns.  The batch is left at the last observation level, analysed."""
    for level, observations, perturb, tap in schedule:
        ahead = int(level) - batch.level
        if ahead < 0:
            raise ValueError(f"cycle: level {level} lies behind the batch, which is at level {batch.level}")
        if ahead:
            batch.step(ahead)
        yield int(level), batch.assimilate(observations, perturb, tap, depth_floor)
