"""What the host side of the C ABI computes before anything goes to the device (flow-sim_amd/csrc/fs_host_pack.hpp) on the CPU, under
AddressSanitizer and UBSan: polylines packed into the device layout with their stage tables (plan_irregular, pack_polylines),
the extended geometry table (extend_table), the validation of boundary arguments (check_bc, check_bc_per_reach) and the per-reach
scheme array (merge_reach_scheme) - until now these ran only behind a handle, which needs a GPU to exist.

tests/host_pack/host_pack_driver.cpp is built with the system compiler and held against tests/golden/host_pack/record.json.  The
inputs are the seeded channels of tests/poly_edges.py (on-vertex stages, flat berms, vertical walls, elevations closer than 1e-6, up
to 245 stations), the geometry of the irr_* fixtures (nodes without a polyline among them), the gerd table, one channel per batch
and distinct channels per reach, with stage tables and on the edge walk, and polylines that each refusal of pack_polylines
answers; for validation a grid of argument sets in which every text of the header occurs and in which two checks apply at once.

The record was written by the code this header replaced, not by this one: the same driver source compiled host-only by hipcc
(--cuda-host-only -DFS_MINIMAL=1, an 8-byte stand-in for the __hip_fatbin_* symbol) against a stand-in header that included
the fs_abi.hip of the parent commit and answered each call through its entry points and file-local functions on a handle built
in place, with host-memory stand-ins for the dozen HIP calls they make.  Arrays are compared bit for bit through their SHA-256 (xt,
zt, lim, extended tables and tz of a 245-station channel are 0.4 MB; the record holds 64 characters for each); both builds target
baseline x86-64 and call the same libm.  The one text no case reaches is the std::bad_alloc one of plan_irregular."""
import hashlib
import itertools
import json
import os
import re
import shutil

import numpy as np
import pytest

from conftest import GOLDEN
from flowsim_amd import _abi as A
from oracle import preissmann_oracle as O

from host_driver import CSRC, PACK_DRIVER, build, line, run
import poly_edges as PE

RECORD = os.path.join(GOLDEN, "host_pack", "record.json")
NFIXED, N_CURVE, SURFACE_AREA = len(A.SC_NAMES), A.SC_NAMES.index("n_curve"), A.SC_NAMES.index("surface_area")
DEFAULT_CAP = 8 << 30


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- polylines ------------------------------------------------------------------------------------------------------------------
def channel(geo):
    """one set: (table [NPARAM, N], x [N, P], z [N, P], limits [N, 2], n_pts [N])"""
    tab = np.stack([np.asarray(geo[k], dtype=np.float64) for k in A.GEO_ROWS])
    return (tab, np.array(geo["irr_x"], dtype=np.float64), np.array(geo["irr_z"], dtype=np.float64),
            np.array(geo["irr_limits"], dtype=np.float64), np.array(geo["irr_npts"], dtype=np.int32))


def cut(ch, N, P):
    """the first N nodes of a channel, rows padded to P stations by repeating the last one"""
    tab, x, z, lim, cnt = ch
    pad = lambda a: np.concatenate([a[:N], np.repeat(a[:N, -1:], P - a.shape[1], axis=1)], axis=1)
    return tab[:, :N].copy(), pad(x), pad(z), lim[:N].copy(), cnt[:N].copy()


def poly_cases():
    """name -> (sets, force_walk, max_bytes)"""
    ch = {f"{kind}-{N}": channel(PE.BUILDERS[kind](N, np.random.default_rng(seed)).geo) for kind, N, seed in PE.CENSUS}
    for name in ("irr_single", "irr_levee", "irr_mixed"):
        fx, meta = O.load_fixture(os.path.join(GOLDEN, name + ".npz"))
        ch[name] = channel(O.problem_from_fixture(fx, meta).geo)
    cases = {name: ([c], 0, DEFAULT_CAP) for name, c in ch.items()}
    for name in ("on_vertex-24", "stations48-16", "irr_mixed"):
        cases[name + "/walk"] = ([ch[name]], 1, DEFAULT_CAP)
    # one channel per reach: three ten-station channels; two of different widths (the narrower padded, fewer nodes of the longer)
    three = [ch["on_vertex-24"], ch["on_vertex_fixed-24"], cut(ch["near_vertex_mixed-64"], 24, 10)]
    two = [ch["multi_run-20"], cut(ch["overtopped_shallow-24"], 20, 15)]
    mixed = [cut(ch["irr_single"], 13, 16), cut(ch["irr_mixed"], 13, 16)]
    cases.update({"sets3": (three, 0, DEFAULT_CAP), "sets3/walk": (three, 1, DEFAULT_CAP), "sets2": (two, 0, DEFAULT_CAP),
                  "sets2_fixtures": (mixed, 0, DEFAULT_CAP)})
    # the size bound: tables exactly at the bound, one byte below it the walk
    N, P = ch["multi_run-20"][1].shape
    size = 2 * N * (((P + 16) & ~15) + 32 * P) * 8
    cases["sets2/at_cap"] = (two, 0, size)
    cases["sets2/over_cap"] = (two, 0, size - 1)
    # what pack_polylines refuses; two faults at once: the first node's, and within a node the order of the checks
    def broken(name, fn, base="multi_run-20", sets=None):
        c = tuple(a.copy() for a in ch[base])
        fn(*c)
        cases["bad/" + name] = ((sets or []) + [c], 0, DEFAULT_CAP)
    def count_one(tab, x, z, lim, cnt): cnt[3] = 1
    def count_over(tab, x, z, lim, cnt): cnt[3] = x.shape[1] + 1
    def nan_x(tab, x, z, lim, cnt): x[4, 2] = np.nan
    def nan_z_padding_ok(tab, x, z, lim, cnt): cnt[4] -= 2; z[4, -1] = np.nan       # beyond the count: not looked at
    def descending(tab, x, z, lim, cnt): x[5, 3] = x[5, 2] - 1.0
    def bed(tab, x, z, lim, cnt): tab[0, 6] += 0.5
    def bed_then_count(tab, x, z, lim, cnt): tab[0, 2] += 0.5; cnt[5] = 1
    def count_then_bed(tab, x, z, lim, cnt): cnt[2] = 1; tab[0, 5] += 0.5
    def nan_and_descending(tab, x, z, lim, cnt): x[5, 3] = x[5, 2] - 1.0; z[5, 3] = np.nan
    def descending_before_nan(tab, x, z, lim, cnt): x[5, 3] = x[5, 2] - 1.0; z[5, 4] = np.nan
    def descending_and_bed(tab, x, z, lim, cnt): x[5, 3] = x[5, 2] - 1.0; tab[0, 5] += 0.5
    for fn in (count_one, count_over, nan_x, nan_z_padding_ok, descending, bed, bed_then_count, count_then_bed, nan_and_descending,
               descending_before_nan, descending_and_bed):
        broken(fn.__name__, fn)
    broken("second_set", bed, sets=[ch["multi_run-20"]])
    return cases


def table_cases():
    fx, meta = O.load_fixture(os.path.join(GOLDEN, "gerd.npz"))
    geo = O.problem_from_fixture(fx, meta).geo
    tab = np.stack([np.asarray(geo[k], dtype=np.float64) for k in A.GEO_ROWS])
    bare = tab.copy()
    bare[A.GEO_ROWS.index("n_main"), ::3] = 0.0          # no roughness: the reciprocal rows hold 0, not inf
    bare[A.GEO_ROWS.index("n_left"), 1::3] = 0.0
    bare[A.GEO_ROWS.index("n_right"), 2::3] = -1.0
    return {"gerd": tab, "gerd_no_roughness": bare}


def run_poly(exe, tmp, name, sets, walk, cap):
    S, (N, P) = len(sets), sets[0][1].shape
    assert all(s[1].shape == (N, P) for s in sets)
    fin, fout = (os.path.join(str(tmp), name.replace("/", "_") + e) for e in (".in", ".out"))
    with open(fin, "wb") as f:
        f.write(np.array([N, P, S, walk, cap], dtype=np.int64).tobytes())
        for i in range(4):
            f.write(np.stack([s[i] for s in sets]).astype(np.float64).tobytes())
        f.write(np.stack([s[4] for s in sets]).astype(np.int32).tobytes())
    got = {"input": hashlib.sha256(open(fin, "rb").read()).hexdigest(), "status": run(exe, ["poly", fin, fout], timeout=600).strip()}
    if got["status"].startswith("ok"):
        out = np.fromfile(fout, dtype=np.float64)
        stride = ((P + 16) & ~15) + 32 * P
        sizes = {"xt": S * P * N, "zt": S * P * N, "lim": S * 2 * N, "tabs": S * 21 * N, "tz": 0 if got["status"].split()[1] == "1" else S * N * stride}
        assert out.size == sum(sizes.values()), (name, out.size, sizes)
        at = 0
        for k, n in sizes.items():
            got[k] = sha(out[at:at + n])
            at += n
    return got


def run_table(exe, tmp, name, tab):
    fin, fout = (os.path.join(str(tmp), name + e) for e in (".tin", ".tout"))
    with open(fin, "wb") as f:
        f.write(np.array([tab.shape[1]], dtype=np.int64).tobytes() + np.ascontiguousarray(tab).tobytes())
    run(exe, ["table", fin, fout], timeout=600)
    out = np.fromfile(fout, dtype=np.float64)
    assert out.size == 21 * tab.shape[1]
    return {"input": sha(tab), "ext": sha(out)}


# ---- validation -----------------------------------------------------------------------------------------------------------------
def curve_column(variant, rows):
    """FS_SC_* rows of one reservoir: n_curve and what its checks look at"""
    nc, good = variant
    col = np.zeros(rows)
    col[A.SC_NAMES.index("alpha")] = 1.0
    col[SURFACE_AREA] = 2.5e6 if (nc != 0 or good) else 0.0
    if rows > N_CURVE:
        col[N_CURVE] = nc
    if nc >= 2 and NFIXED + 2 * nc <= rows:
        col[NFIXED:NFIXED + nc] = np.arange(nc) * (1.0 if good else -1.0) + 600.0
        if not good and nc == 3:
            col[NFIXED:NFIXED + nc] = [600.0, 601.0, 601.0]          # the last pair only, and equal: not increasing
        col[NFIXED + nc:NFIXED + 2 * nc] = 1e6 * (1 + np.arange(nc))
    return col


CURVES = [(-1, True), (0, True), (0, False), (1, True), (2, True), (2, False), (3, True), (3, False)]
NEED = [0, 1, 1, 2, 4, 5, 10, 5]


def check_lines():
    out = []
    B = 3
    # fs_batch_set_bc: every kind (two beyond each end), parameter counts around the kind's own, with and without parameters / target
    for side, kind, per_reach, has_p, has_t, tables in itertools.product((0, 1), range(-2, 12), (0, 1), (0, 1), (0, 1), (0, 1)):
        need = NEED[kind] if 0 <= kind < len(NEED) else 3
        for n_params in sorted({0, need, need + 1, 3}):
            out.append(line("wide", side, kind, n_params, per_reach, has_p, has_t, B, tables, *np.linspace(0.5, 2.0, max(n_params, NFIXED) * B)))
    # ... the general reservoir: one shared, and one per reach with two reaches that fail different checks
    for side, rows, has_p in itertools.product((0, 1), (NFIXED - 1, NFIXED, NFIXED + 4, NFIXED + 5, NFIXED + 6), (1, 0)):
        for v in CURVES:
            out.append(line("wide", side, A.BC_STORAGE_CURVE, rows, 0, has_p, 0, B, 1, *curve_column(v, max(rows, NFIXED))))
        for v0, v1 in itertools.product(CURVES, CURVES):
            p = np.stack([curve_column(v0, max(rows, NFIXED)), curve_column(v1, max(rows, NFIXED))], axis=1)
            out.append(line("wide", side, A.BC_STORAGE_CURVE, rows, 1, has_p, 0, 2, 1, *p.ravel()))
    # fs_batch_set_bc_per_reach_wide: every triple of kinds
    kinds = (-1, A.BC_FLOW_HYDROGRAPH, A.BC_NORMAL_DEPTH, A.BC_STORAGE, A.BC_STORAGE_CURVE, A.BC_HOST_ROW, 10)
    rows = NFIXED + 4
    for side, has_t, tables in itertools.product((0, 1), (0, 1), (0, 1)):
        for ks in itertools.product(kinds, kinds, kinds):
            p = np.stack([curve_column((2, True), rows) if k == A.BC_STORAGE_CURVE else np.linspace(0.5, 2.0, rows) for k in ks], axis=1)
            out.append(line("per", side, rows, has_t, B, tables, *ks, *p.ravel()))
    # ... reservoirs whose rows fail, beside each other and beside other kinds
    for side, tables, rows in itertools.product((0, 1), (0, 1), (A.BC_MAX_PARAMS, NFIXED, NFIXED + 4, NFIXED + 6)):
        for (v0, v1), ks in itertools.product(itertools.product(CURVES, CURVES), ((8, 8), (8, 3), (10, 8), (9, 8), (1, 8))):
            p = np.stack([curve_column(v0, rows), curve_column(v1, rows)], axis=1)
            out.append(line("per", side, rows, 0, 2, tables, *ks, *p.ravel()))
    # the per-reach scheme array
    vals = np.arange(15, dtype=np.float64).reshape(5, 3) / 7.0 + 0.1
    for mask in (0, 1, 6, 8, 16, 21, 31):
        out.append(line("scheme", 3, mask, 0.6, 30.0, 250.0, 1e-4, 100.0, *vals.ravel()))
    return out


def run_checks(exe, tmp):
    lines = check_lines()
    fin = os.path.join(str(tmp), "checks.txt")
    with open(fin, "w") as f:
        f.write("\n".join(lines) + "\n")
    out = run(exe, ["checks", fin], timeout=600).splitlines()
    assert len(out) == len(lines)
    return {"input": hashlib.sha256("\n".join(lines).encode()).hexdigest(), "lines": out}


# fs::poly_tables_walk: (n_sets, N, max_pts, force_walk, max_bytes) -> "walk MiB".  Sixteen stations take (32 + 32 * 16) * 8 = 4 352
# bytes of tables per node, two channels of 24 nodes 208 896 bytes; the comparison with the bound is a strict >.
WALK = {
    (2, 24, 16, 0, 208897): "0 0",                # the tables one byte below the bound
    (2, 24, 16, 0, 208896): "0 0",                # at it: tables still
    (2, 24, 16, 0, 208895): "1 0",                # one byte above: the edge walk
    (1, 1, 2, 1, DEFAULT_CAP): "1 0",             # FS_POLY_WALK with 640 bytes of tables
    (1, 1, 2, 0, DEFAULT_CAP): "0 0",
    # around the default bound of 8 GiB (no table has an odd byte count: the nearest are 2^33 - 512 and 2^33 + 3 840 bytes), in whole MiB
    (1, 1973790, 16, 0, DEFAULT_CAP): "0 8191",
    (1, 1973791, 16, 0, DEFAULT_CAP): "1 8192",
    (1973791, 1, 16, 0, DEFAULT_CAP + 3840): "0 8192",
    (1, 1973791, 16, 0, DEFAULT_CAP + 3839): "1 8192",
}


def test_tables_or_the_edge_walk(tmp_path):
    """the one decision both irregular setters of fs_abi.hip and plan_irregular take; the expected answers are written out above"""
    if shutil.which("g++") is None:
        pytest.skip("no system C++ compiler")
    fin = os.path.join(str(tmp_path), "walk.txt")
    with open(fin, "w") as f:
        f.write("".join(line("walk", *case) + "\n" for case in WALK))
    out = run(build(PACK_DRIVER, tmp_path), ["checks", fin], timeout=600).splitlines()
    assert out == list(WALK.values()), [(c, g, w) for (c, w), g in zip(WALK.items(), out) if g != w]


def encode(lines):
    """answers as indices into the list of distinct ones (thousands of cases, a few dozen answers)"""
    texts = sorted(set(lines))
    return {"texts": texts, "index": [texts.index(ln) for ln in lines]}


def measure(exe, tmp):
    """everything the record holds, from this driver"""
    return {"poly": {name: run_poly(exe, tmp, name, *c) for name, c in poly_cases().items()},
            "table": {name: run_table(exe, tmp, name, t) for name, t in table_cases().items()},
            "checks": run_checks(exe, tmp)}


@pytest.fixture(scope="module")
def record():
    return json.load(open(RECORD))


@pytest.fixture(scope="module")
def measured(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no system C++ compiler")
    tmp = tmp_path_factory.mktemp("host_pack")
    return measure(build(PACK_DRIVER, tmp), tmp)


def test_the_inputs_are_the_recorded_ones(measured, record):
    """(a record held against other inputs would fail below for the wrong reason)"""
    assert set(measured["poly"]) == set(record["poly"]) and set(measured["table"]) == set(record["table"])
    for kind in ("poly", "table"):
        for name, got in measured[kind].items():
            assert got["input"] == record[kind][name]["input"], (kind, name)
    assert measured["checks"]["input"] == record["checks"]["input"]


def test_polylines_pack_bit_for_bit(measured, record):
    for name, got in measured["poly"].items():
        want = record["poly"][name]
        assert got["status"] == want["status"], name
        for k in ("xt", "zt", "lim", "tabs", "tz"):
            assert got.get(k) == want.get(k), (name, k)


def test_extended_tables_bit_for_bit(measured, record):
    for name, got in measured["table"].items():
        assert got["ext"] == record["table"][name]["ext"], name


def test_every_check_answers_as_recorded(measured, record):
    want = [record["checks"]["texts"][i] for i in record["checks"]["index"]]
    got = measured["checks"]["lines"]
    assert len(got) == len(want)
    diff = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not diff, (len(diff), [(check_lines()[i][:60], got[i], want[i]) for i in diff[:3]])


def test_the_record_holds_every_case_and_every_text(record):
    """categories: one set and several, nodes without a polyline, tables and the walk, each refusal; every text of the header"""
    poly = record["poly"]
    walks = {n for n, r in poly.items() if r["status"].startswith("ok 1")}
    assert {"on_vertex-24/walk", "sets3/walk", "sets2/over_cap"} <= walks and "sets2/at_cap" not in walks and "stations250-6" not in walks
    assert all("tz" in r and r["tz"] != sha(np.empty(0)) for n, r in poly.items() if r["status"].startswith("ok 0"))
    cases = poly_cases()
    assert any(np.any(s[4] == 0) for s in cases["irr_mixed"][0]) and any(np.any(s[4] == 0) for s in cases["sets2_fixtures"][0])
    assert len(cases["sets3"][0]) == 3 and cases["stations250-6"][0][0][1].shape[1] >= 245
    answers = set(record["checks"]["texts"]) | {r["status"] for r in poly.values()}
    src = open(os.path.join(CSRC, "fs_host_pack.hpp")).read()
    texts = set(re.findall(r'return "([^"]+)";', src))
    assert len(texts) == 14, sorted(texts)
    assert texts <= answers, sorted(texts - answers)
    # two checks at once: the first node's fault, and within a node the count before the stations before the bed level
    assert "Z_BED" in poly["bad/bed_then_count"]["status"] and "n_pts" in poly["bad/count_then_bed"]["status"]
    assert "same shape" in poly["bad/nan_and_descending"]["status"] and "ascending" in poly["bad/descending_before_nan"]["status"]
    assert "ascending" in poly["bad/descending_and_bed"]["status"] and poly["bad/nan_z_padding_ok"]["status"].startswith("ok")
    assert any(t.startswith("ok 1 1 9") for t in answers) and any(t.startswith("ok 1 0 8") for t in answers) and "ok" in answers


MUTATIONS = {
    # unused vertex slots hold zero, not the last vertex
    "zero_padding": ("xt[j * N + i] = x[src]; zt[j * N + i] = z[src];",
                     "xt[j * N + i] = j < (size_t)c ? x[src] : 0.0; zt[j * N + i] = j < (size_t)c ? z[src] : 0.0;"),
    # a general reservoir on a reach: the side is looked at before the section mode
    "check_order": ("""      if (!tables) return "fs_batch_set_bc_per_reach: FS_BC_STORAGE_CURVE needs section mode FS_SEC_TABLE or FS_SEC_IRREGULAR";
      if (side != FS_DOWNSTREAM) return "fs_batch_set_bc: the storage boundary is downstream only";
""", """      if (side != FS_DOWNSTREAM) return "fs_batch_set_bc: the storage boundary is downstream only";
      if (!tables) return "fs_batch_set_bc_per_reach: FS_BC_STORAGE_CURVE needs section mode FS_SEC_TABLE or FS_SEC_IRREGULAR";
"""),
}


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_the_record_catches_a_mutation(record, tmp_path, name):
    """fs_host_pack.hpp copied with one statement changed: the record has cases whose answer moves"""
    if shutil.which("g++") is None:
        pytest.skip("no system C++ compiler")
    old, new = MUTATIONS[name]
    src = open(os.path.join(CSRC, "fs_host_pack.hpp")).read()
    assert src.count(old) == 1, name
    with open(tmp_path / "fs_host_pack.hpp", "w") as f:
        f.write(src.replace(old, new))
    exe = build(PACK_DRIVER, tmp_path, [tmp_path, CSRC])          # the copy first: the driver's #include "fs_host_pack.hpp" finds it
    if name == "zero_padding":
        moved = [n for n, c in poly_cases().items() if not n.startswith("bad/")
                 and any(run_poly(exe, tmp_path, n, *c).get(k) != record["poly"][n].get(k) for k in ("xt", "zt"))]
    else:
        want = [record["checks"]["texts"][i] for i in record["checks"]["index"]]
        moved = [i for i, (g, w) in enumerate(zip(run_checks(exe, tmp_path)["lines"], want)) if g != w]
    print(name, len(moved), moved[:8])
    assert moved, name
