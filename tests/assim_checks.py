"""What the assimilation tests share (tests/test_assim_host.py, tests/test_gpu_assimilate.py): a sequential Python restatement of
fs_batch_assimilate (include/flowsim_abi.h) - the host part of fs::analysis_coefficients, the chunked moments and the update of
flow-sim_amd/csrc/fs_assim.hpp, in the orders the header states - that the host driver and the device are held to bit for bit; the
textbook form of the same analysis in numpy; and the bars the restatement itself is held to."""
import math

import numpy as np

CHUNK = 256
EPS = 2.0 ** -52
f = np.float64


class Refused(Exception):
    pass


def coefficients(y, active, value, variance, perturb=None):
    """dict(n_active, ybar [m], S [m, B], C [m, m], L [m, m], Z [m, B]) from the gathered values y [m, B]: every operation one
    float64 operation, sums over the active members in member order.  Raises Refused as the library refuses."""
    y = np.asarray(y, dtype=f)
    m, B = y.shape
    act = [r for r in range(B) if active[r]]
    na = len(act)
    if na < 2:
        raise Refused("active member(s)")
    ybar, S = np.zeros(m), np.zeros((m, B))
    for j in range(m):
        s = f(0.0)
        for r in act:
            if y[j, r] != y[j, r]:
                raise Refused("NaN")
            s = s + y[j, r]
        ybar[j] = s / f(na)
        for r in act:
            S[j, r] = y[j, r] - ybar[j]
    Cm = np.zeros((m, m))
    for j in range(m):
        for l in range(j + 1):
            s = f(0.0)
            with np.errstate(over="ignore"):
                for r in act:
                    s = s + S[j, r] * S[l, r]
            c = s / f(na - 1)
            if j == l:
                c = c + f(variance[j])
            Cm[j, l] = Cm[l, j] = c
    L = np.zeros((m, m))                              # unit lower triangle below the diagonal, the pivots on it
    for j in range(m):
        for l in range(j + 1):
            s = Cm[j, l]
            for k in range(l):
                s = s - (L[j, k] * L[k, k]) * L[l, k]
            if j == l:
                if not (s > 0.0) or not math.isfinite(s):
                    raise Refused("not positive definite")
                L[j, j] = s
            else:
                L[j, l] = s / L[l, l]
    Z = np.zeros((m, B))
    for r in act:
        w, z = np.zeros(m), np.zeros(m)
        for j in range(m):
            target = f(value[j]) + f(perturb[j][r]) if perturb is not None else f(value[j])
            s = target - y[j, r]
            for k in range(j):
                s = s - L[j, k] * w[k]
            w[j] = s
        for j in range(m - 1, -1, -1):
            s = w[j] / L[j, j]
            for k in range(j + 1, m):
                s = s - L[k, j] * z[k]
            z[j] = s
        Z[:, r] = z
    return dict(n_active=na, ybar=ybar, S=S, C=Cm, L=L, Z=Z)


def moments(x, active, S):
    """(mean [N], var [N], P [m, N]) of one field x [B, N] (float64 values of the batch dtype): vectorised over the nodes, sequential
    over the members - chunks of CHUNK by batch index, active members in member order, chunk partials added in chunk order"""
    x = np.asarray(x, dtype=f)
    B, N = x.shape
    m = S.shape[0]
    act = [r for r in range(B) if active[r]]
    na = len(act)
    c = x[act[0]]
    tot = None
    for r0 in range(0, B, CHUNK):
        s1, s2, p = np.zeros(N), np.zeros(N), np.zeros((m, N))
        for r in range(r0, min(B, r0 + CHUNK)):
            if not active[r]:
                continue
            d = x[r] - c
            s1 = s1 + d
            s2 = s2 + d * d
            for j in range(m):
                p[j] = p[j] + d * S[j, r]
        tot = [s1, s2, p] if tot is None else [tot[0] + s1, tot[1] + s2, tot[2] + p]
    s1, s2, p = tot
    mean = c + s1 / f(na)
    var = (s2 - (s1 * s1) / f(na)) / f(na - 1)
    return mean, var, p / f(na - 1)


def update(xk, xg, active, P, Z, taper, dtype, floor=None):
    """(new xk, new xg, clamped [B]) of one field: inc = sum_j (taper_j P_j) Z_jr in j order from 0.0, added in float64 and rounded to
    the batch dtype; floor: the depth floor (the depth field only)"""
    xk, xg = np.array(xk, dtype=f), np.array(xg, dtype=f)
    B, N = xk.shape
    m = P.shape[0]
    clamped = np.zeros(B, dtype=np.int32)
    for r in range(B):
        if not active[r]:
            continue
        inc = np.zeros(N)
        for j in range(m):
            w = P[j] if taper is None else np.asarray(taper[j], dtype=f) * P[j]
            inc = inc + w * Z[j, r]
        with np.errstate(invalid="ignore"):
            vk, vg = xk[r] + inc, xg[r] + inc
            if floor is not None:
                low = ~(vk >= floor)
                vk = np.where(low, floor, vk)
                vg = np.where(low | ~(vg >= floor), floor, vg)
                clamped[r] = int(low.sum())
        xk[r], xg[r] = vk.astype(dtype).astype(f), vg.astype(dtype).astype(f)
    return xk, xg, clamped


def analysis(y, mark_active, hk, Qk, hg, Qg, value, variance, perturb=None, taper=None, floor=1e-3, dtype=np.float64):
    """the whole call on gathered values y [m, B] and states [B, N]: dict(n_active, prior [4, N], cross_cov [2, m, N], hk, Qk, hg, Qg,
    clamped, Z, C)"""
    co = coefficients(y, mark_active, value, variance, perturb)
    mh, vh, Ph = moments(hk, mark_active, co["S"])
    mq, vq, Pq = moments(Qk, mark_active, co["S"])
    nhk, nhg, clamped = update(hk, hg, mark_active, Ph, co["Z"], taper, dtype, floor)
    nqk, nqg, _ = update(Qk, Qg, mark_active, Pq, co["Z"], taper, dtype)
    return dict(n_active=co["n_active"], prior=np.stack([mh, vh, mq, vq]), cross_cov=np.stack([Ph, Pq]), hk=nhk, Qk=nqk, hg=nhg, Qg=nqg,
                clamped=clamped, Z=co["Z"], C=co["C"], S=co["S"], ybar=co["ybar"])


def textbook(X, H, value, variance, perturb, active):
    """x + P H^T (H P H^T + R)^-1 (d - H x) in numpy on the state matrix X [B, n] with a LINEAR observation operator H [m, n]; the
    sample covariance over the active members, unbiased.  Returns the analysed X (inactive rows unchanged)."""
    X = np.asarray(X, dtype=f)
    act = np.flatnonzero(active)
    Xa = X[act]
    A_ = Xa - Xa.mean(axis=0)
    Pm = A_.T @ A_ / (len(act) - 1)
    K = Pm @ H.T @ np.linalg.inv(H @ Pm @ H.T + np.diag(variance))
    out = X.copy()
    for r in act:
        d = np.asarray(value, dtype=f) + (perturb[:, r] if perturb is not None else 0.0) - H @ X[r]
        out[r] = X[r] + K @ d
    return out


def same(a, b):
    """the same float64 values, NaN being one value"""
    a, b = np.asarray(a, dtype=f), np.asarray(b, dtype=f)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)
