"""The kernel dispatch (flow-sim_amd/csrc/fs_dispatch.hpp: fits, pick) on the CPU, over the key table built from the library's own
instantiation lists (fs_entry_list.hpp) - until now the choice was only seen through GPU batches.

tests/dispatch/dispatch_driver.cpp is built with the system compiler under AddressSanitizer and UBSan and answers for a grid of
queries: both arithmetic types x the four section modes x 19 node counts x every pair of boundary kinds x need_diag x need_any x
the four hetero values = 243 200 queries, under each of ten settings of the environment's overrides.  Its `plan` command answers
what a launch of an entry reserves and keeps (fs::plan_launch), held to the layouts the kernels address as written out in plan_check.

tests/golden/dispatch/choices.npz is the record they are held against: the 115 keys in table order ("keys": dtype, sec, M, W, full, bck,
diag, longk, tail, team), the chosen index or -1 of every query under every setting ("choice_<setting>"), and the tables of the
FS_MINIMAL builds ("minimal_<variant>").  It was written by the code this dispatch replaced, not by this one: a scratch program
that included the fs_abi.hip of that commit, compiled host-only (hipcc --cuda-host-only, the fs_part_*.hip units likewise at -O0 so
that the extern templates resolve, empty stand-ins for the __hip_fatbin_* symbols), looped its pick_kernel over the same grid in
the same order under the same environment settings, and printed its kEntries; the FS_MINIMAL tables came from the same program
compiled with -DFS_MINIMAL=1 / 2 / 3 (and -DFS_NO_TAIL, -DFS_TEAM_8X4)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

from host_driver import CSRC, build, run

DRIVER = os.path.join(ROOT, "tests", "dispatch", "dispatch_driver.cpp")
RECORD = os.path.join(ROOT, "tests", "golden", "dispatch", "choices.npz")
HIPCC = "/opt/rocm/bin/hipcc"
CLANG = "/opt/rocm/lib/llvm/bin/clang"

SETTINGS = {
    "none": {}, "no_team": {"FS_NO_TEAM": "1"}, "shape_8_4": {"FS_KERNEL_SHAPE": "8,4"}, "shape_8_8": {"FS_KERNEL_SHAPE": "8,8"},
    "general": {"FS_KERNEL_GENERAL": "1"}, "team_m_8": {"FS_TEAM_M": "8"},
    # forced: the general rect fp64 (16, 4) entry, which fits 2.5 % of the grid; a tail-only entry, which fits a handful; two out of range
    "index_5": {"FS_KERNEL_INDEX": "5"}, "index_109": {"FS_KERNEL_INDEX": "109"}, "index_115": {"FS_KERNEL_INDEX": "115"},
    "index_minus_1": {"FS_KERNEL_INDEX": "-1"},
}
CHOOSING = ("none", "no_team", "shape_8_4", "shape_8_8", "general", "team_m_8")      # the settings that choose, not force
OVERRIDE_VARS = ("FS_KERNEL_INDEX", "FS_KERNEL_SHAPE", "FS_KERNEL_GENERAL", "FS_NO_TEAM", "FS_TEAM_M")
# the grid, outermost first (dispatch_driver.cpp); N in the record ("grid_N")
N_KINDS, GRID_TAIL = 10, (10, 10, 2, 2, 4)
F64, F32 = 0, 1
RECT, TRAP, TABLE, IRREGULAR = 0, 1, 2, 3
FLOW, NORMAL_DEPTH, RATING_BLEND = 0, 3, 6


def run_driver(exe, args, env_extra):
    return run(exe, args, env_extra, drop_env=OVERRIDE_VARS, timeout=300)


def grid_choices(exe, setting, tmp):
    out = os.path.join(str(tmp), f"grid_{setting}.bin")
    run_driver(exe, ["grid", out], SETTINGS[setting])
    return np.fromfile(out, dtype=np.int16)


def query(exe, dtype, sec, N, usk, dsk, need_diag=0, need_any=0, hetero=0, env=None):
    """(index, why)"""
    idx, why = run_driver(exe, ["query", *map(str, (dtype, sec, N, usk, dsk, need_diag, need_any, hetero))], env or {}).split("\n")[:2]
    return int(idx), why


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no system C++ compiler")
    return build(DRIVER, tmp_path_factory.mktemp("dispatch"))


@pytest.fixture(scope="module")
def record():
    return np.load(RECORD)


def test_the_table_is_the_recorded_one(driver, record):
    table = np.array([ln.split() for ln in run_driver(driver, ["table"], {}).splitlines()], dtype=np.int16)
    assert table.shape == (115, 10) and record["keys"].shape == (115, 10)
    assert np.array_equal(table, record["keys"]), np.nonzero(np.any(table != record["keys"], axis=1))[0]


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_every_recorded_choice_is_reproduced(driver, record, tmp_path, setting):
    want = record["choice_" + setting]
    assert want.size == 2 * 4 * len(record["grid_N"]) * int(np.prod(GRID_TAIL)) == 243200
    got = grid_choices(driver, setting, tmp_path)
    assert got.size == want.size
    diff = np.nonzero(got != want)[0]
    assert diff.size == 0, (setting, diff.size, [np.unravel_index(i, (2, 4, len(record["grid_N"])) + GRID_TAIL) for i in diff[:5]])


def test_the_record_reaches_every_entry(record):
    """a property of the grid: an entry no query chooses would be one whose place in the order nothing here checks"""
    reached = set()
    for s in CHOOSING:
        c = record["choice_" + s]
        reached |= set(c[c >= 0].tolist())
    assert reached == set(range(115)), sorted(set(range(115)) - reached)
    assert set(record["grid_N"].tolist()) >= {2, 64, 65, 121, 128, 129, 256, 512, 513, 1024, 2048, 4096, 4097, 8192, 9000, 16384, 16385,
                                              32768, 32769}
    # refusals are part of the behaviour: over half of the default setting's queries have no kernel
    none = record["choice_none"]
    assert 0.5 < np.mean(none < 0) < 0.56 and len(set(none[none >= 0].tolist())) == 107
    # the forced settings: entry 5 or nothing; nothing out of range
    assert set(record["choice_index_5"].tolist()) == {-1, 5} and set(record["choice_index_109"].tolist()) <= {-1, 109}
    assert np.all(record["choice_index_115"] == -1) and np.all(record["choice_index_minus_1"] == -1)


def test_the_refusals_say_why(driver):
    """the two texts of fs::pick (the storage-curve and boundary-kind texts are fs_abi.hip's: tests/test_gpu_*.py)"""
    assert query(driver, F64, RECT, 40000, FLOW, NORMAL_DEPTH) == (
        -1, "no kernel instantiation for N=40000 (supported: 2..32768 nodes for the uniform section modes, 2..16384 for tables and polylines)")
    assert query(driver, F64, TABLE, 16385, FLOW, NORMAL_DEPTH)[1].startswith("no kernel instantiation for N=16385 (supported")
    assert query(driver, F32, RECT, 100, FLOW, NORMAL_DEPTH, env={"FS_KERNEL_INDEX": "5"}) == (-1, "FS_KERNEL_INDEX=5 does not fit this batch")
    assert query(driver, F64, RECT, 100, FLOW, NORMAL_DEPTH, env={"FS_KERNEL_INDEX": "115"}) == (-1, "FS_KERNEL_INDEX=115 does not fit this batch")
    assert query(driver, F64, RECT, 2000, FLOW, NORMAL_DEPTH, env={"FS_KERNEL_INDEX": "7x"}) == (-1, "FS_KERNEL_INDEX=7x does not fit this batch")
    assert query(driver, F64, RECT, 4000, FLOW, NORMAL_DEPTH, need_diag=1, env={"FS_KERNEL_INDEX": "5"}) == (5, "")


def test_the_order_of_preference_in_plain_cases(driver, record):
    """tests/test_gpu_bench_kernels.py::test_dispatch_prefers_the_most_specific_instantiation restated (rectangular fp64 reaches, flow
    hydrograph in, normal depth out): smallest capacity, then fewest waves per reach, then the most specific variant (boundary
    pair fixed > closed-form rows > general; the build without history stores when the batch keeps none and there is one)."""
    keys = record["keys"]
    cls = 2 + NORMAL_DEPTH

    def chosen(sec, N, dsk, history, **kw):
        i, why = query(driver, F64, sec, N, FLOW, dsk, need_diag=int(history), **kw)
        assert i >= 0, why
        return dict(zip(KEY_FIELDS, keys[i].tolist()))

    want = {   # N -> (M, W, full, class, diag without history)
        4096: (16, 4, 1, cls, 0), 4000: (16, 4, 0, cls, 0), 2048: (16, 2, 1, cls, 0), 1024: (16, 1, 1, cls, 0), 512: (8, 1, 1, cls, 0),
        300: (8, 1, 0, cls, 1), 513: (16, 1, 0, 1, 1), 200: (4, 1, 0, 1, 1), 100: (2, 1, 0, 1, 1), 40: (2, 1, 0, 1, 1),
        2000: (16, 2, 0, 1, 1),      # (16, 2) and (8, 4) both hold 2 048 rows: fewer waves per reach
    }
    for N, (M, W, full, bck, diag) in want.items():
        for history in (False, True):
            k = chosen(RECT, N, NORMAL_DEPTH, history)
            assert (k["M"], k["W"], k["full"], k["bck"], k["diag"]) == (M, W, full, bck, 1 if history else diag), (N, history, k)
            assert (k["longk"], k["tail"], k["team"]) == (0, -1, 0)
    # asked for by shape, the (8, 4) kernel takes the 2 000-node reach
    k = chosen(RECT, 2000, NORMAL_DEPTH, True, env={"FS_KERNEL_SHAPE": "8,4"})
    assert (k["M"], k["W"], k["full"], k["bck"]) == (8, 4, 0, 1)
    # beyond one lane grid: a team of workgroups (full: a whole number of lane grids); without teams, and for tables, the multi-pass kernel
    k = chosen(RECT, 8192, NORMAL_DEPTH, False)
    assert (k["team"], k["M"], k["W"], k["full"], k["bck"], k["diag"]) == (1, 16, 4, 1, cls, 0)
    k = chosen(RECT, 9000, NORMAL_DEPTH, True)
    assert (k["team"], k["M"], k["W"], k["full"], k["bck"], k["diag"]) == (1, 16, 4, 0, 1, 1)
    k = chosen(RECT, 9000, NORMAL_DEPTH, True, env={"FS_NO_TEAM": "1"})
    assert (k["longk"], k["team"], k["M"], k["W"], k["bck"]) == (1, 0, 8, 4, 0)
    k = chosen(TABLE, 9000, NORMAL_DEPTH, True)
    assert (k["longk"], k["M"], k["W"], k["bck"]) == (1, 4, 4, -1)
    # the gate-curve ensemble shape (121 nodes, tables): the tail-only form, (N - 1) mod 2 == 0 - unless the reaches differ in length
    k = chosen(TABLE, 121, RATING_BLEND, False)
    assert (k["M"], k["W"], k["bck"], k["diag"], k["tail"]) == (2, 1, 2 + RATING_BLEND, 0, 0)
    assert chosen(TABLE, 122, RATING_BLEND, False)["tail"] == 1
    k = chosen(TABLE, 121, RATING_BLEND, False, hetero=1)
    assert (k["M"], k["W"], k["bck"], k["diag"], k["tail"]) == (2, 1, 2 + RATING_BLEND, 0, -1)
    # an iteration budget needs the kernels that take any boundary kind
    assert chosen(TABLE, 121, RATING_BLEND, False, need_any=1)["bck"] == -1


MUTATIONS = {
    # more waves per reach first at equal capacity
    "waves_tie_break": (", k.W, -specificity}", ", -k.W, -specificity}"),
    # a tail-only entry for any node count
    "tail_condition": ("(q.N - 1) % k.M != k.tail", "false"),
}


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_the_record_catches_a_mutation(record, tmp_path, name):
    """fs_dispatch.hpp copied with one token changed: the grid has queries whose choice moves"""
    if shutil.which("g++") is None:
        pytest.skip("no system C++ compiler")
    old, new = MUTATIONS[name]
    src = open(os.path.join(CSRC, "fs_dispatch.hpp")).read()
    assert src.count(old) == 1, name
    with open(tmp_path / "fs_dispatch.hpp", "w") as f:
        f.write(src.replace(old, new))
    exe = build(DRIVER, tmp_path, [tmp_path, CSRC])          # the copy first: the driver's #include "fs_dispatch.hpp" finds it
    moved = {s: int(np.sum(grid_choices(exe, s, tmp_path) != record["choice_" + s])) for s in CHOOSING}
    print(name, moved)
    assert moved["none"] > 0, moved


# ---- the launch plan (fs::plan_launch): what launch_steps reserves and keeps for the entry a batch got ----
KEY_FIELDS = ("dtype", "sec", "M", "W", "full", "bck", "diag", "longk", "tail", "team")
SLOT = 12 * 16      # fs_kernel.hpp, KernelArgs::team_mail: [B][2][G W + 1][kTeamWords = 12] of 16-byte (value, tag) words


def plan_cases(keys):
    """(entry, sec, N, B, n_steps, storage_downstream): every team and multi-pass entry where a rounding slip in ceil(N / grid) shows -
    one row past a lane grid, two grids, one row short of the capacity, the capacity - and one single-workgroup entry per section mode"""
    sizes, single = [], {}
    for i, row in enumerate(keys.tolist()):
        k = dict(zip(KEY_FIELDS, row))
        grid = 64 * k["W"] * k["M"]
        if k["team"] or k["longk"]:
            sizes += [(i, k["sec"], N) for N in (grid + 1, 2 * grid, grid * 64 // k["W"] - 1, grid * 64 // k["W"])]
        elif not k["full"] and k["tail"] < 0:
            single.setdefault(k["sec"], (i, k["sec"], grid))
    return [(*s, B, n_steps, storage) for s in sizes + sorted(single.values()) for B in (1, 3) for n_steps in (1, 2) for storage in (0, 1)]


def plan_check(exe, keys, tmp):
    """(the cases that fit their entry, those of them whose plan is not what the layout comments of fs_kernel.hpp - KernelArgs:
    kc_scratch, passes, team_size, team_mail - and the two restore kernels of fs_abi.hip say)"""
    cases = plan_cases(keys)
    with open(tmp / "plans.txt", "w") as f:
        f.write("".join(" ".join(map(str, c)) + "\n" for c in cases))
    out = [list(map(int, ln.split())) for ln in run_driver(exe, ["plan", tmp / "plans.txt"], {}).splitlines()]
    assert len(out) == len(cases)
    fit, bad = [], []
    for case, (fits, *got, stride) in zip(cases, out):      # got: passes, kc_scratch_elems, team_size, team_mail_bytes, keep_entry, keep_stage
        (i, sec, N, B, n_steps, storage), k = case, dict(zip(KEY_FIELDS, keys[case[0]].tolist()))
        if not fits:
            continue
        grid, W, uniform = 64 * k["W"] * k["M"], k["W"], sec in (RECT, TRAP)
        G = -(-N // grid)
        assert G <= 64 // W
        want = [G * k["longk"], B * 4 * G * grid * (k["longk"] and not uniform), G * k["team"], B * 2 * (G * W + 1) * SLOT * k["team"],
                int(k["longk"] and uniform and n_steps > 1), int(storage and n_steps > 1)]
        # the end of the last slot a team addresses - reach B - 1, parity 1, the upstream row's slot G W - with mailboxes `stride` bytes apart
        last_end = (((B - 1) * 2 + 1) * stride + G * W * SLOT + SLOT) * k["team"]
        fit.append(case)
        if got != want or last_end != got[3]:
            bad.append((case, got, want, last_end))
    return fit, bad


def test_the_launch_plan_is_what_the_kernels_address(driver, record, tmp_path):
    """crossed with B in {1, 3}, n_steps in {1, 2} and a storage boundary downstream or none.  A single-workgroup entry gets no
    passes, scratch, team or entry state; its reservoir stage is kept like every kernel's (restore_failed_stage), by the same rule."""
    keys = record["keys"]
    fit, bad = plan_check(driver, keys, tmp_path)
    kinds = {(int(keys[c[0]][7]), int(keys[c[0]][9]), c[1]) for c in fit}
    assert {(0, 0, sec) for sec in (RECT, TRAP, TABLE, IRREGULAR)} <= kinds and {(1, 0, RECT), (1, 0, TABLE), (0, 1, RECT)} <= kinds
    assert {c[0] for c in fit} == {c[0] for c in plan_cases(keys)}, "an entry none of whose sizes fits it"
    print(len(fit), "cases fit,", len({c[0] for c in fit}), "entries")
    assert not bad, (len(bad), bad[:3])


def test_the_plan_check_catches_a_mailbox_one_slot_short(record, tmp_path):
    """fs_dispatch.hpp copied with G W slots per mailbox in place of G W + 1 (none for the upstream row): every team case fails"""
    if shutil.which("g++") is None:
        pytest.skip("no system C++ compiler")
    old, new = "(size_t)(G * W + 1) * kTeamWords * 16", "(size_t)(G * W) * kTeamWords * 16"
    src = open(os.path.join(CSRC, "fs_dispatch.hpp")).read()
    assert src.count(old) == 1
    with open(tmp_path / "fs_dispatch.hpp", "w") as f:
        f.write(src.replace(old, new))
    fit, bad = plan_check(build(DRIVER, tmp_path, [tmp_path, CSRC]), record["keys"], tmp_path)
    team = [c for c in fit if record["keys"][c[0]][9]]
    assert team and [b[0] for b in bad] == team, (len(bad), len(team))


MINIMAL = {"1": ["-DFS_MINIMAL=1"], "2": ["-DFS_MINIMAL=2"], "3": ["-DFS_MINIMAL=3"], "1_no_tail": ["-DFS_MINIMAL=1", "-DFS_NO_TAIL"],
           "1_team_8x4": ["-DFS_MINIMAL=1", "-DFS_TEAM_8X4"]}
TABLE_PROBE = """
import ctypes, sys
lib = ctypes.CDLL(sys.argv[1])
e = (ctypes.c_int32 * 8)()
for i in range(lib.fs_kernel_table_size()):
    assert lib.fs_kernel_table_entry(i, e) == 0
    print(*e, lib.fs_kernel_table_entry_tail(i), lib.fs_kernel_table_entry_team(i))
"""


@pytest.mark.parametrize("variant", list(MINIMAL))
def test_the_tables_of_the_minimal_builds(record, tmp_path, variant):
    """fs_abi.hip alone with -DFS_MINIMAL=... (flow-sim_amd/csrc/build_variants.sh; =1 is also the sanitizer build of
    tests/test_sanitizers.py), host code only: its table through the fs_kernel_table_* accessors, which need no device"""
    if not (os.path.exists(HIPCC) and os.path.exists(CLANG)):
        pytest.skip("no ROCm compiler")
    obj, stub, sobj, lib = (str(tmp_path / n) for n in ("fs_abi.o", "fatbin_stub.c", "fatbin_stub.o", "libflowsim_hip.so"))
    r = subprocess.run([HIPCC, "-O0", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-host-only", "-Wno-unused-result", *MINIMAL[variant],
                        "-c", "-o", obj, os.path.join(CSRC, "fs_abi.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    # (the device image the host object would embed: an empty stand-in, as in tests/test_sanitizers.py - nothing here launches)
    und = [ln.split()[-1] for ln in subprocess.run(["nm", "-u", obj], capture_output=True, text=True).stdout.splitlines() if "__hip_fatbin" in ln]
    open(stub, "w").write("".join(f"const char {u}[8] = {{0}};\n" for u in und) or "int fs_no_stub;\n")
    subprocess.run([CLANG, "-fPIC", "-c", stub, "-o", sobj], check=True, capture_output=True)
    r = subprocess.run([HIPCC, "-shared", "-o", lib, obj, sobj, "-L/opt/rocm/lib", "-lrocprofiler-sdk-roctx", "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([sys.executable, "-c", TABLE_PROBE, lib], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    table = np.array([ln.split() for ln in r.stdout.splitlines()], dtype=np.int16)
    want = record["minimal_" + variant]
    assert table.shape == want.shape and np.array_equal(table, want), (table.shape, want.shape)
