"""Adversarial rows for the cross-member band kernels (bands_kernel in fs_reduce.hpp, profile_bands_kernel in fs_envelope.hpp) and a
float64 restatement of what those kernels document.  A LIBRARY, not a test: tests/test_band_cases.py checks it on the CPU,
tests/test_gpu_band_select.py runs the kernels on its rows.  Every row is built from a fixed seed (the crc32 of the case's name).

The restatement follows the kernel's text step by step: the order-preserving key (band_key / band_unkey), the leading bytes min and
max share (lead), the two ranks around the virtual index (m - 1) q, one most-significant-byte pass per remaining byte with a histogram
per rank, and quantile_lerp as written.  While it selects it takes a CENSUS of the paths the kernel's counting loop would take on
that row: which waves of 64 lanes add a popcount once, which add lane by lane, where a wave's first active lane sits."""
import math
import zlib
from fractions import Fraction

import numpy as np

OK, MAX_ITER, NAN, ILL_CONDITIONED = 0, 1, 2, 4          # include/flowsim_abi.h
THREADS, WAVE, MAX_Q = 256, 64, 16                      # kBandThreads, the wave, kBandMaxQ
EPS = 2.0 ** -52
U64 = np.uint64
TOP = U64(1) << U64(63)

B_SMALL = (1, 2, 63, 64, 65, 255, 256, 257, 511, 513)
B_LARGE = (4099, 32769)
B_PATTERNED = (65, 257, 513)                            # the sizes every left-out pattern is applied at (and B_LARGE where a family is large)
PATTERNS = ("none", "first1", "first5", "first64", "every2nd", "wave_mid", "all_but_one", "all")
Q_FIXED = {"q0": (), "q2": (0.0, 1.0), "q3": (0.05, 0.5, 0.95)}
Q_SETS = ("q0", "q2", "q3", "q16")
_FILL = (0.05, 0.25, 0.5, 0.75, 0.95, 1.0 / 3.0, 2.0 / 3.0, 0.999, 0.001, 0.1, 0.9, 0.4, 0.6, 0.2, 0.8, 0.3)


# ---- the kernel's documented pieces, in float64 / uint64 ----------------------------------------------------------------------
def band_key(v):
    """the order-preserving integer image of a double; -0.0 is folded into +0.0 first (the kernel's `+ 0.0`)"""
    u = (np.asarray(v, dtype=np.float64) + 0.0).view(U64)
    return np.where(u >> U64(63) != 0, ~u, u | TOP)


def band_unkey(k):
    k = np.asarray(k, dtype=U64)
    return np.where(k >> U64(63) != 0, k & ~TOP, ~k).view(np.float64)


def lead_bytes(kmin, kmax):
    """bytes, from the top, that kmin and kmax share (kmin != kmax)"""
    return (64 - int(int(kmin) ^ int(kmax)).bit_length()) // 8


def ranks(m, q):
    """the two ranks around the virtual index (m - 1) q and the weight of the upper one"""
    vi = np.float64(m - 1) * np.float64(q)
    fl = np.floor(vi)
    lo = min(max(int(fl), 0), m - 1)
    hi = min(lo + 1, m - 1)
    g = np.float64(0.0) if vi >= np.float64(m - 1) else vi - fl
    return lo, hi, g


def quantile_lerp(a, b, gamma):
    """fs_reduce.hpp's quantile_lerp, line by line (numpy scalars: one rounding per operation, nothing fused)"""
    a, b, gamma = np.float64(a), np.float64(b), np.float64(gamma)
    if gamma == 0.0 or a == b:
        return a
    with np.errstate(all="ignore"):
        d = b - a
        v = b - d * (np.float64(1.0) - gamma) if gamma >= 0.5 else a + d * gamma
    if v < a:
        v = a
    if v > b:
        v = b
    return v


def virtual_index_is_integer(m, q):
    vi = np.float64(m - 1) * np.float64(q)
    return bool(vi == np.floor(vi)) or bool(vi >= m - 1)


# ---- cases --------------------------------------------------------------------------------------------------------------------
class Case:
    """one row of B members: x (float64 or float32: which entry point it goes to), status[B], and what kind of row it is"""

    def __init__(self, name, family, x, status, kind="finite", large=False):
        self.name, self.family, self.x, self.status, self.kind, self.large = name, family, x, status.astype(np.int32), kind, large
        self.B = len(x)

    def __repr__(self):
        return self.name

    @property
    def kept(self):
        return (self.status == OK) | (self.status == ILL_CONDITIONED)

    def values(self):
        """the kept members as the kernel sees them: doubles, -0.0 folded"""
        return self.x[self.kept].astype(np.float64) + 0.0

    def q(self, qset):
        return q_levels(qset, np.sort(self.values()))


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def left_out(pattern, B):
    out = np.zeros(B, dtype=bool)
    if pattern == "first1":
        out[:1] = True
    elif pattern == "first5":
        out[:5] = True
    elif pattern == "first64":
        out[:64] = True
    elif pattern == "every2nd":
        out[0::2] = True                                  # the even members: every wave's first active lane is lane 1
    elif pattern == "wave_mid":
        w = (B // WAVE) // 2
        out[w * WAVE:(w + 1) * WAVE] = True
    elif pattern == "all_but_one":
        out[:] = True
        out[(2 * B) // 3] = False
    elif pattern == "all":
        out[:] = True
    else:
        assert pattern == "none", pattern
    return out


def status_of(out):
    """left-out members alternate FS_NAN / FS_MAX_ITER; every fifth kept member carries the warning FS_ILL_CONDITIONED and stays in"""
    B = len(out)
    st = np.where(np.arange(B) % 5 == 3, ILL_CONDITIONED, OK)
    return np.where(out, np.where(np.arange(B) % 2 == 0, NAN, MAX_ITER), st).astype(np.int32)


def _key_block(base, low_bits, B, rng):
    """doubles whose bit patterns are base's with the low `low_bits` bits replaced: base + k ulp(base) for 0 <= k < 2^low_bits.  k = 0 and
    k = 2^low_bits - 1 are both present (B >= 2), so the keys differ first in exactly the byte that holds bit low_bits - 1."""
    u0 = int(np.float64(base).view(U64)) & ~((1 << low_bits) - 1)
    k = rng.integers(0, 1 << low_bits, size=B, dtype=np.uint64, endpoint=False)
    k[0], k[-1] = 0, (1 << low_bits) - 1
    if low_bits <= 16:                                    # small integers k: heavy ties
        k[1:-1] = rng.integers(0, min(1 << low_bits, 24), size=max(B - 2, 0), dtype=np.uint64)
    return (U64(u0) + k).view(np.float64)


def _family_rows(D):
    """(family, tag, builder(B, rng) -> x, sizes, patterned, kind, large) for the device type D"""
    rows = []

    def add(family, tag, build, sizes, patterned=False, kind="finite", large=False):
        rows.append((family, tag, build, sizes, patterned, kind, large))

    if D == np.float64:
        add("a", "uniform", lambda B, r: r.uniform(-1.0, 1.0, B), B_SMALL + B_LARGE, patterned=True, large=True)
        add("b", "wide", lambda B, r: r.choice([-1.0, 1.0], B) * 10.0 ** r.uniform(-150.0, 150.0, B), B_SMALL)
        for lead in range(1, 8):
            for sign, base in (("pos", 1.2345), ("neg", -1234.5)):
                add("c", f"lead{lead}{sign}", lambda B, r, lead=lead, base=base: _key_block(base, 64 - 8 * lead, B, r), (2, 65, 257))
        add("d", "ties", lambda B, r: r.permutation(np.repeat([-2.5, -1.0, 0.75, 3.0, 7.0], _split(B, 5, r))), B_SMALL + B_LARGE,
            patterned=True, large=True)
        add("e", "const", lambda B, r: np.full(B, 3.25), (1, 2, 64, 257))
        add("e", "zeros", lambda B, r: np.where(r.integers(0, 2, B) == 0, -0.0, 0.0), (1, 2, 64, 257))
        add("e", "subnormal", lambda B, r: r.choice([-0.0, 5e-324, -5e-324, 1e-320, -1e-320, 0.0], B), (2, 64, 257))
        add("f", "blocks", _blocks, B_SMALL, patterned=True)
        add("g", "integers", lambda B, r: r.integers(-1, 7, B).astype(np.float64), B_SMALL)
        add("h", "nan", lambda B, r: _with(r.uniform(-1.0, 1.0, B), {B // 2: np.nan}), (1, 65, 257), kind="nan")
        add("i", "pinf", lambda B, r: _with(r.uniform(-1.0, 1.0, B), {B // 3: np.inf}), (65, 257), kind="inf")
        add("i", "ninf", lambda B, r: _with(r.uniform(-1.0, 1.0, B), {B // 3: -np.inf}), (65, 257), kind="inf")
        add("i", "bothinf", lambda B, r: _with(r.uniform(-1.0, 1.0, B), {1: np.inf, B - 2: -np.inf, B // 2: np.inf}), (65, 257), kind="inf")
    else:
        f = np.float32
        add("j", "uniform32", lambda B, r: r.uniform(-1.0, 1.0, B).astype(f), (1, 65, 257, 513), patterned=True)
        for lead in range(1, 5):                          # a float32's 32 bits end inside the double's fifth byte
            for sign, base in (("pos", 1.2345), ("neg", -1234.5)):
                add("j", f"lead{lead}{sign}32", lambda B, r, lead=lead, base=base: _key_block32(base, lead, B, r), (2, 65, 257))
        add("j", "ties32", lambda B, r: r.permutation(np.repeat(np.array([-2.5, -1.0, 0.1, 3.0, 7.0], dtype=f), _split(B, 5, r))),
            (1, 65, 257, 513), patterned=True)
    return rows


def _key_block32(base, lead, B, rng):
    """float32 values whose DOUBLE keys share exactly `lead` bytes: the double's bit 64 - 8 lead - 1 is the float's bit 35 - 8 lead - 1"""
    low = 35 - 8 * lead                                   # double bit p = float bit p - 29 (the mantissas are left-aligned, 52 against 23 bits)
    u0 = int(np.float32(base).view(np.uint32)) & ~((1 << low) - 1)
    k = rng.integers(0, min(1 << low, 1 << 20), size=B, dtype=np.uint32)
    k[0], k[-1] = 0, (1 << low) - 1
    return (np.uint32(u0) + k).view(np.float32)


def _split(B, parts, rng):
    """B members in `parts` runs, every run as even as B allows, in a random order of sizes"""
    base = np.full(parts, B // parts)
    base[:B % parts] += 1
    return rng.permutation(base)


def _with(x, at):
    for i, v in at.items():
        x[i] = v
    return x


def _blocks(B, rng):
    """blocks of 64 consecutive equal members (a wave that adds its popcount once) between blocks of 64 distinct members of both signs
    (a wave that adds lane by lane), aligned to the waves"""
    x = rng.uniform(-1.0, 1.0, B)
    consts = (0.625, -0.375, 0.625, 1.5)
    for j in range(0, (B + WAVE - 1) // WAVE, 2):
        x[j * WAVE:(j + 1) * WAVE] = consts[(j // 2) % len(consts)]
    return x


def _build(D):
    cases = []
    for family, tag, build, sizes, patterned, kind, large in _family_rows(D):
        for B in sizes:
            big = B in B_LARGE
            pats = PATTERNS if patterned and (B in B_PATTERNED or big) else ("none",)
            for pat in pats:
                name = f"{family}-{tag}-B{B}-{pat}"
                cases.append(Case(name, family, build(B, _rng(name)), status_of(left_out(pat, B)), kind, big))
    return cases


CASES_F64 = _build(np.float64)
CASES_F32 = _build(np.float32)
ALL_CASES = CASES_F64 + CASES_F32
FAMILIES = sorted({c.family for c in ALL_CASES})


def q_levels(qset, s):
    """the quantile levels of a named set for a row whose kept members, sorted, are s.  q16: k / (m - 1) for k = 0, 1, m - 2, m - 1, then
    levels whose ranks sit at the first, at the last and inside the longest run of ties of s, then fixed levels up to 16."""
    if qset != "q16":
        return np.array(Q_FIXED[qset], dtype=np.float64)
    m = len(s)
    lv = [0.0, 1.0]
    finite = m > 1 and bool(np.all(np.isfinite(s)))
    if m > 1:
        lv = [k / (m - 1) for k in (0, 1, m - 2, m - 1)]
    if finite:
        edges = np.flatnonzero(np.diff(s) != 0)
        starts, ends = np.concatenate([[0], edges + 1]), np.concatenate([edges, [m - 1]])
        j = int(np.argmax(ends - starts))
        a, e = int(starts[j]), int(ends[j])
        if e > a:
            lv += [(a + 0.5) / (m - 1), (e - 0.5) / (m - 1), a / (m - 1), e / (m - 1), ((a + e) // 2 + 0.25) / (m - 1)]
            if a >= 1:
                lv.append((a - 0.5) / (m - 1))
    out = []
    for v in lv + list(_FILL):
        v = min(max(float(v), 0.0), 1.0)
        if v not in out:
            out.append(v)
    return np.array(out[:MAX_Q], dtype=np.float64)


# ---- what the kernels must return ---------------------------------------------------------------------------------------------
def exact_moments(v):
    """mean and population standard deviation of the doubles v, each correctly rounded from the exact rational value (the square root
    adds its own half ulp).  Doubles are dyadic: everything is integer arithmetic at the smallest exponent."""
    m = len(v)
    f, e = np.frexp(np.asarray(v, dtype=np.float64))
    mant, e = (f * 2.0 ** 53).astype(np.int64).tolist(), (e - 53).tolist()
    emin = min(e)
    X = [t << (k - emin) for t, k in zip(mant, e)]
    S, SS = sum(X), sum(t * t for t in X)
    scale = Fraction(2) ** emin
    return float(Fraction(S, m) * scale), math.sqrt(float(Fraction(m * SS - S * S, m * m) * scale * scale))


def row_stats(v):
    """v: the kept members of one row (doubles, -0.0 folded).  What does not depend on the quantile levels: the count, np.sort, the sums
    the bars are made of, and - on a finite row - the exact mean and standard deviation."""
    m = len(v)
    e = dict(m=m, none=m == 0 or bool(np.any(np.isnan(v))))
    if e["none"]:
        return e
    s = np.sort(v)
    e.update(sorted=s, min=s[0], max=s[-1], abs_sum=math.fsum(np.abs(s)), abs_max=float(np.max(np.abs(s))), finite=bool(np.all(np.isfinite(s))))
    if e["finite"]:
        e["mean"], e["std"] = exact_moments(s)
    return e


def expected(v, q, stats=None):
    """row_stats(v) plus, for the levels q, the statistics as the kernel documents them: the two order statistics of every level from
    np.sort, whether its virtual index is an integer, and quantile_lerp of the two"""
    e = dict(stats if stats is not None else row_stats(v), q=np.asarray(q, dtype=np.float64))
    if e["none"]:
        return e
    s, m = e["sorted"], e["m"]
    rk = [ranks(m, t) for t in e["q"]]
    e["lo"] = np.array([s[lo] for lo, _, _ in rk], dtype=np.float64)
    e["hi"] = np.array([s[hi] for _, hi, _ in rk], dtype=np.float64)
    e["integer"] = np.array([virtual_index_is_integer(m, t) for t in e["q"]], dtype=bool)
    e["quantiles"] = np.array([quantile_lerp(s[lo], s[hi], g) for lo, hi, g in rk], dtype=np.float64)
    return e


# ---- the select, restated, with its census ------------------------------------------------------------------------------------
def select(x, kept, q):
    """The radix select of bands_kernel on the row x (doubles) with the members `kept`, for the levels q.  Returns (order statistics
    [2 n_q] as doubles: the lower and the upper rank of every level, census).  Rows without a member or with a NaN have no select."""
    B = len(x)
    idx = np.flatnonzero(kept)
    v = np.asarray(x, dtype=np.float64)[idx] + 0.0
    m = len(idx)
    c = dict(lead=None, passes=0, popcount_waves=0, perlane_waves=0, both_paths_in_one_pass=False, first_lane_nonzero=False,
             wave_without_member=False, negative_keys=False, positive_keys=False, negative_zero=False, select_skipped=False,
             rank_first_of_run=False, rank_last_of_run=False, rank_inside_run=False, no_row=False)
    if m == 0 or np.any(np.isnan(v)):
        c["no_row"] = True
        return None, c
    keys = band_key(v)
    c["negative_keys"], c["positive_keys"] = bool(np.any(keys < TOP)), bool(np.any(keys >= TOP))
    c["negative_zero"] = bool(np.any(np.signbit(np.asarray(x, dtype=np.float64)[idx]) & (v == 0.0)))
    waves_in = np.zeros((B + WAVE - 1) // WAVE, dtype=bool)
    waves_in[idx // WAVE] = True
    c["wave_without_member"] = not bool(np.all(waves_in))          # (a wave of lanes below B whose members are all left out)
    kmin, kmax = band_key(np.min(v)), band_key(np.max(v))
    targets = []
    for t in q:
        lo, hi, _ = ranks(m, t)
        targets += [lo, hi]
    s = np.sort(v)
    for r in targets:
        a, e = int(np.searchsorted(s, s[r], "left")), int(np.searchsorted(s, s[r], "right")) - 1
        if e > a:
            c["rank_first_of_run" if r == a else "rank_last_of_run" if r == e else "rank_inside_run"] = True
    if kmin == kmax:
        c["select_skipped"] = True
        return np.full(len(targets), band_unkey(kmin)), c
    lead = lead_bytes(kmin, kmax)
    c["lead"], c["passes"] = lead, 8 - lead
    found = {}
    for r0 in sorted(set(targets)):
        rank, act, act_idx = r0, keys, idx                          # the members that carry this target's bytes so far
        pfx = int(kmin) & (0 if lead == 0 else (~0 << (64 - 8 * lead)) & 0xFFFFFFFFFFFFFFFF)
        for shift in range(56 - 8 * lead, -1, -8):
            bins = ((act >> U64(shift)) & U64(255)).astype(np.int64)
            wave, first = np.unique(act_idx // WAVE, return_index=True)
            same = np.logical_and.reduceat(bins == np.repeat(bins[first], np.diff(np.append(first, len(bins)))), first)
            n_pop, n_lane = int(np.sum(same)), int(np.sum(~same))
            c["popcount_waves"] += n_pop
            c["perlane_waves"] += n_lane
            c["both_paths_in_one_pass"] |= n_pop > 0 and n_lane > 0
            c["first_lane_nonzero"] |= bool(np.any(act_idx[first] % WAVE != 0))
            hist = np.bincount(bins, minlength=256)
            below, b = 0, 0
            while b < 255 and not rank < below + hist[b]:
                below += int(hist[b])
                b += 1
            rank -= below
            pfx |= b << shift
            keep = bins == b
            act, act_idx = act[keep], act_idx[keep]
        found[r0] = pfx
    return band_unkey(np.array([found[r] for r in targets], dtype=U64)), c
