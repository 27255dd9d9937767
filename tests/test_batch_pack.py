"""The Python half of the C ABI's argument layout (flow-sim_amd/flowsim_amd/_pack.py) on the CPU: what PreissmannBatch's setters hand
to the library, without a library.

a. tests/golden/batch_pack/record.json holds dtype, shape and SHA-256 of every array (and every count and flag) of every case of
   cases() below.  The record was written by the code these functions replaced, not by them: a script imported cases() from this
   module and answered each packer's name through the setters of the parent commit's batch.py, on PreissmannBatch objects made
   with __new__ (B, N, L, mode and a dummy handle set by hand) whose library was a stub that kept the arguments of every call and
   returned 0, with batch._dptr the identity and _abi.check a no-op; int32 arguments were read back from their ctypes pointers
   with the element count the call implies.  The inputs are therefore the same by construction, and the comparison is bit for bit.
b. Every packed boundary goes as a `wide` or `per` line through the `checks` mode of tests/host_pack/host_pack_driver.cpp (built
   and run under ASan/UBSan as tests/test_host_pack.py does): fs::check_bc / fs::check_bc_per_reach accept what Python packs.
c. The module packs where the library has not been built."""
import hashlib
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, fixture_paths
from fixture_batch import boundary_spec, merge_specs
from flowsim_amd import BoundarySpec
from flowsim_amd import _abi as A
from flowsim_amd import _pack
from host_driver import PACK_DRIVER, build, line, run
from oracle import preissmann_oracle as O

RECORD = os.path.join(GOLDEN, "batch_pack", "record.json")
NF = len(A.SC_NAMES)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def problem(name):
    return O.problem_from_fixture(*O.load_fixture(os.path.join(GOLDEN, name + ".npz")))


def single_reach_fixtures():
    """(name, Problem) of the fixtures with one member and one-dimensional targets"""
    for path in fixture_paths():
        fx, meta = O.load_fixture(path)
        if fx["initial_conditions"].ndim == 2 and all(fx[k].ndim == 1 for k in fx.files if k.endswith("_target")):
            yield os.path.basename(path)[:-4], O.problem_from_fixture(fx, meta)


def copies(spec, B=3):
    """B specs of the kind of `spec` that differ where no check looks: bed level, hydrograph, the areas of the curve"""
    out = []
    for r in range(B):
        p = dict(spec.params)
        if p.get("bed_level") is not None:
            p["bed_level"] = p["bed_level"] + 0.125 * r
        if p.get("curve") is not None:
            p["curve"] = np.asarray(p["curve"], dtype=np.float64) * [1.0, 1.0 + 0.25 * r]
        out.append(BoundarySpec(spec.kind, p, None if spec.target is None else np.asarray(spec.target) * (1.0 + 0.25 * r)))
    return out


CURVE5 = np.array([[600.0, 1e6], [601.0, 2e6], [602.5, 3.5e6], [604.0, 4e6], [610.0, 9e6]])
RESERVOIR = dict(min_stage=600.0, Y_min=599.0, Y_max=612.0, bed_level=598.5, surface_area=2.5e6, beta=0.75, rc_type=1.0, rc_a=12.0,
                 rc_b=1.5)
TARGET = np.linspace(100.0, 160.0, 7)


def boundary_cases():
    """(name, form, side, B, L, spec | [specs], what the library is to answer): form 'wide' through fs_batch_set_bc, 'per' through
    fs_batch_set_bc_per_reach_wide"""
    for fname, p in single_reach_fixtures():
        for side, bc in ((A.UPSTREAM, p.us), (A.DOWNSTREAM, p.ds)):
            spec = boundary_spec(bc, p.nt)
            n = p.nt if spec.target is None else len(spec.target)
            for L in ((n,) if spec.target is None else (n, n - 1, n + 2)):
                tag = f"{fname}/{'us' if side == A.UPSTREAM else 'ds'}/L{L}"
                yield tag + "/one", "wide", side, 1, L, spec, "ok"
                yield tag + "/merged", "wide", side, 3, L, merge_specs(copies(spec), 3), "ok"
                yield tag + "/per_reach", "per", side, 3, L, copies(spec), "ok"
    ds = A.DOWNSTREAM
    curve = lambda **kw: BoundarySpec(A.BC_STORAGE_CURVE, dict(RESERVOIR, **kw))
    yield "curve/shared", "wide", ds, 3, 4, curve(curve=CURVE5, alpha=0.5), "ok"
    yield "curve/scalar_per_reach", "wide", ds, 3, 4, curve(curve=CURVE5, Y_max=np.array([612.0, 613.0, 615.5])), "ok"
    yield "curve/curve_per_reach", "wide", ds, 2, 4, curve(curve=np.stack([CURVE5[:3], CURVE5[2:]])), "ok"
    yield "curve/alpha_none", "wide", ds, 3, 4, curve(curve=CURVE5[:2], alpha=None), "ok"
    yield "curve/alpha_none_per_reach", "wide", ds, 3, 4, curve(curve=CURVE5[:2], alpha=None, beta=[0.5, 0.75, 1.0]), "ok"
    yield "curve/no_curve", "wide", ds, 3, 4, curve(), "ok"
    yield "curve/no_curve_per_reach", "per", ds, 2, 4, [curve(), curve(surface_area=1e6)], "ok"
    mixed = [curve(curve=CURVE5), curve(curve=CURVE5[1:3], alpha=None),
             BoundarySpec(A.BC_STORAGE, dict(surface_area=2e6, min_stage=600.0, Y_min=599.0, Y_max=612.0, bed_level=598.5)),
             BoundarySpec(A.BC_NORMAL_DEPTH, dict(bed_slope=1e-4, bed_level=598.5))]
    yield "curve/mixed", "per", ds, 4, 4, mixed, "ok"
    yield "curve/mixed_host_row", "per", ds, 4, 4, mixed[:3] + [BoundarySpec(A.BC_HOST_ROW)], "ok"
    yield "curve/mixed_kind_17", "per", ds, 4, 4, mixed[:3] + [BoundarySpec(17)], "Invalid boundary condition."
    yield ("curve/mixed_flow_no_target", "per", ds, 4, 4, mixed[:3] + [BoundarySpec(A.BC_FLOW_HYDROGRAPH)],
           "Insufficient arguments for boundary condition.")
    yield "host_row", "wide", ds, 3, 4, BoundarySpec(A.BC_HOST_ROW), "ok"
    yield "flow_no_target", "wide", A.UPSTREAM, 3, 4, BoundarySpec(A.BC_FLOW_HYDROGRAPH), "Insufficient arguments for boundary condition."
    yield "target/shared", "wide", A.UPSTREAM, 3, 9, BoundarySpec(A.BC_FLOW_HYDROGRAPH, {}, TARGET), "ok"
    yield ("target/per_column", "wide", A.UPSTREAM, 3, 5,
           BoundarySpec(A.BC_STAGE_HYDROGRAPH, dict(bed_level=[1.0, 2.0, 3.0]), np.outer(TARGET, [1.0, 1.5, 2.0])), "ok")
    ragged = [BoundarySpec(A.BC_FLOW_HYDROGRAPH, {}, TARGET), BoundarySpec(A.BC_FIXED_DEPTH, dict(initial_depth=2.0)),
              BoundarySpec(A.BC_STAGE_HYDROGRAPH, dict(bed_level=1.0), TARGET[:3] / 50.0), BoundarySpec(A.BC_FLOW_HYDROGRAPH, {}, TARGET[:5])]
    yield "target/ragged", "per", A.UPSTREAM, 4, 5, ragged, "ok"


def pack_boundary(P, form, B, L, spec):
    if form == "wide":
        params, n_params, per_reach = P.bc_params(spec, B)
        return dict(params=params, n_params=n_params, per_reach=per_reach, target=P.bc_target(spec.target, L, B))
    kinds, params, rows = P.bc_params_per_reach(spec, B)
    return dict(kinds=kinds, params=params, rows=rows, target=P.bc_target_per_reach([s.target for s in spec], L, B))


def stacked_polylines(probs):
    """one channel per reach as fixture_batch.per_reach_polyline_batch stacks them: nodes padded with the last node, stations with
    the last station"""
    N, P = max(p.N for p in probs), max(p.geo["irr_x"].shape[1] for p in probs)
    nodes = lambda a: np.concatenate([np.asarray(a), np.repeat(np.asarray(a)[-1:], N - len(a), axis=0)], axis=0)
    pts = lambda a: np.concatenate([a, np.repeat(a[:, -1:], P - a.shape[1], axis=1)], axis=1)
    geo = {k: np.stack([nodes(p.geo[k]) for p in probs]) for k in A.GEO_ROWS}
    geo["irr_npts"] = np.stack([nodes(p.geo["irr_npts"]) for p in probs]).astype(np.int32)
    geo["irr_x"] = np.stack([nodes(pts(np.asarray(p.geo["irr_x"], dtype=np.float64))) for p in probs])
    geo["irr_z"] = np.stack([nodes(pts(np.asarray(p.geo["irr_z"], dtype=np.float64))) for p in probs])
    geo["irr_limits"] = np.stack([nodes(p.geo["irr_limits"]) for p in probs])
    return geo, N


def geometry_cases():
    gerd = {k: np.asarray(v)[:24] for k, v in problem("gerd").geo.items() if k in A.GEO_ROWS}
    yield "table/shared", lambda P: dict(tab=P.geometry_table(gerd, 3, 24, False))
    own = dict(gerd, z_bed=np.stack([gerd["z_bed"] + 0.5 * r for r in range(3)]), n_main=np.outer([1.0, 1.1, 0.9], gerd["n_main"]))
    yield "table/per_reach", lambda P: dict(tab=P.geometry_table(own, 3, 24, True))
    mixed = problem("irr_mixed")
    yield "irregular/shared", lambda P: dict(zip(("tab", "n_pts", "x", "z", "limits", "per_reach"), P.irregular_arrays(mixed.geo, 2, mixed.N)))
    geo, N = stacked_polylines([problem("irr_single"), mixed])
    yield "irregular/per_reach", lambda P: dict(zip(("tab", "n_pts", "x", "z", "limits", "per_reach"), P.irregular_arrays(geo, 2, N)))
    yield "uniform/rect", lambda P: dict(p=P.uniform_params(False, 3, [8.0, 9.5, 11.0], 0.03, 12.5, [11.0, 10.5, 10.0]))
    yield "uniform/rect_slope_ignored", lambda P: dict(p=P.uniform_params(False, 3, 8.0, [0.02, 0.03, 0.04], 12.5, 11.0, side_slope=1.5))
    yield "uniform/trap_no_slope", lambda P: dict(p=P.uniform_params(True, 3, [8.0, 9.5, 11.0], 0.03, 12.5, 11.0))
    yield "uniform/trap", lambda P: dict(p=P.uniform_params(True, 3, 8.0, 0.03, [12.5, 12.0, 11.5], 11.0, side_slope=[1.0, 1.5, 2.0]))
    yield "n_override/none", lambda P: dict(ov=P.n_override(None, 3))
    yield "n_override/list", lambda P: dict(ov=P.n_override([0.02, 0.03, 0.045], 3))


def broadcast_cases():
    B, N = 3, 5
    row, grid = np.linspace(1.0, 2.0, N), np.linspace(0.5, 7.5, B * N).reshape(B, N)
    yield "per_reach/scalar", lambda P: dict(v=P.per_reach(0.6, B))
    yield "per_reach/int_scalar", lambda P: dict(v=P.per_reach(30, B))
    yield "per_reach/list", lambda P: dict(v=P.per_reach([0.55, 0.6, 1.0], B))
    yield "per_reach/float32", lambda P: dict(v=P.per_reach(np.array([0.1, 0.2, 0.3], dtype=np.float32), B))
    yield "per_reach/max_iter_scalar", lambda P: dict(v=P.per_reach(40, B, np.int32))
    yield "per_reach/max_iter_list", lambda P: dict(v=P.per_reach([40, 7, 100], B, np.int32))
    yield "per_reach/none", lambda P: dict(v=P.opt_per_reach(None, B))
    yield "per_reach/optional", lambda P: dict(v=P.opt_per_reach([1.0, 2.0, 3.0], B))
    yield "per_node/scalar", lambda P: dict(v=P.per_node(2.5, B, N))
    yield "per_node/row", lambda P: dict(v=P.per_node(row, B, N))
    yield "per_node/grid", lambda P: dict(v=P.per_node(grid, B, N))
    yield "per_node/transposed_view", lambda P: dict(v=P.per_node(np.asfortranarray(grid), B, N))
    yield "bed_slope/none", lambda P: dict(zip(("v", "per_reach"), P.bed_slope(None, B, N)))
    yield "bed_slope/row_with_none", lambda P: dict(zip(("v", "per_reach"), P.bed_slope([1e-4, None, 2e-4, 2e-4, None], B, N)))
    yield "bed_slope/grid", lambda P: dict(zip(("v", "per_reach"), P.bed_slope(grid * 1e-4, B, N)))
    yield "host_rows", lambda P: dict(rows=P.host_rows([1.0, 0.0, 1.0], 0.0, [0.25, -0.5, 1e-9], B))
    yield "host_rows/scalars", lambda P: dict(rows=P.host_rows(1.0, 2.0, 3.0, 1))


def cases():
    """(name, callable(P) -> dict of arrays, counts and flags); P: anything with the functions of flowsim_amd._pack"""
    for name, form, side, B, L, spec, answer in boundary_cases():
        yield "bc/" + name, lambda P, a=(form, B, L, spec): pack_boundary(P, *a)
    yield from geometry_cases()
    yield from broadcast_cases()


def digest(v):
    if isinstance(v, np.ndarray):
        assert v.flags.c_contiguous
        return dict(dtype=str(v.dtype), shape=list(v.shape), sha256=hashlib.sha256(v.tobytes()).hexdigest())
    return None if v is None else int(v)


def measure(P):
    return {name: {k: digest(v) for k, v in fn(P).items()} for name, fn in cases()}


# ---- a. held to the parent's arrays ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def record():
    return json.load(open(RECORD))


def test_packers_reproduce_the_recorded_arrays(record):
    got = measure(_pack)
    assert list(got) == list(record)
    diff = [(name, k) for name in got for k in set(got[name]) | set(record[name]) if got[name].get(k, "-") != record[name].get(k, "-")]
    assert not diff, (len(diff), diff[:8])


def test_the_cases_cover_what_the_setters_take(record):
    names = {n.split("/")[1] for n in record if n.endswith("/one")}
    assert names == {n for n, _ in single_reach_fixtures()} and len(names) >= 15
    kinds = {spec.kind for name, form, _, _, _, spec, _ in boundary_cases() if name.endswith("/one")}
    assert kinds == set(range(A.BC_HOST_ROW))          # every kind the device evaluates
    assert record["bc/curve/mixed"]["rows"] == 26 == NF + 2 * len(CURVE5)
    assert record["bc/host_row"] == dict(params=None, n_params=3, per_reach=1, target=None)
    assert record["bc/akbari/ds/L21/one"]["params"]["shape"] == [2] and record["bc/akbari/ds/L21/merged"]["params"]["shape"] == [2, 3]
    assert record["bc/akbari/us/L21/one"]["params"] is None and record["bc/akbari/us/L21/one"]["n_params"] == 0
    for L in (20, 21, 23):          # truncated, exact, padded
        assert record[f"bc/akbari/us/L{L}/per_reach"]["target"]["shape"] == [L, 3]
    assert record["bc/target/ragged"]["target"]["shape"] == [5, 4] and record["bc/curve/mixed"]["target"] is None
    assert record["irregular/per_reach"]["per_reach"] == 1 and record["irregular/shared"]["per_reach"] == 0
    assert record["per_reach/max_iter_list"]["v"]["dtype"] == "int32" and record["bed_slope/row_with_none"]["v"]["shape"] == [5]


def test_values_behind_the_hashes():
    """a few of the arrays spelled out: the record says they are the parent's, this says what they are"""
    (specs,) = [spec for name, _, _, _, _, spec, _ in boundary_cases() if name == "curve/mixed_kind_17"]
    kinds, p, rows = _pack.bc_params_per_reach(specs, 4)
    assert rows == 26 and p.shape == (26, 4) and kinds.tolist() == [A.BC_STORAGE_CURVE, A.BC_STORAGE_CURVE, A.BC_STORAGE, 17]
    sc = lambda name: A.SC_NAMES.index(name)
    assert p[sc("alpha")].tolist() == [1.0, 0.0, 0.0, 0.0] and p[sc("n_curve")].tolist()[:2] == [5.0, 2.0]
    assert p[sc("rc_a"), :2].tolist() == [12.0, 12.0] and p[sc("K_q"), :2].tolist() == [0.0, 0.0]
    assert np.array_equal(p[NF:NF + 5, 0], CURVE5[:, 0]) and np.array_equal(p[NF + 5:NF + 10, 0], CURVE5[:, 1])
    assert np.array_equal(p[NF:NF + 4, 1], [601.0, 602.5, 2e6, 3.5e6]) and not p[NF + 4:, 1].any() and not p[:, 3].any()
    assert p[:5, 2].tolist() == [2e6, 600.0, 599.0, 612.0, 598.5] and not p[5:, 2].any()
    t = _pack.bc_target(TARGET, 9, 2)
    assert np.array_equal(t[:7, 1], TARGET) and np.all(t[7:] == TARGET[-1])
    t = _pack.bc_target_per_reach([TARGET, None, TARGET[:3]], 5, 3)
    assert np.array_equal(t[:, 0], TARGET[:5]) and not t[:, 1].any() and t[:, 2].tolist() == [*TARGET[:3], TARGET[2], TARGET[2]]
    assert _pack.bc_target_per_reach([None, None], 5, 2) is None and _pack.bc_target(None, 5, 2) is None
    with pytest.raises(KeyError):
        _pack.bc_params(BoundarySpec(17), 3)
    v, per = _pack.bed_slope([1e-4, None], 3, 2)
    assert per == 0 and v[0] == 1e-4 and np.isnan(v[1])


# ---- b. the library's own validation accepts what Python packs ------------------------------------------------------------------
def check_line(form, side, B, packed):
    p = packed["params"]
    if form == "wide":
        return line("wide", side, packed["kind"], packed["n_params"], packed["per_reach"], p is not None, packed["target"] is not None, B, 1,
                    *([] if p is None else p.ravel()))
    return line("per", side, packed["rows"], packed["target"] is not None, B, 1, *packed["kinds"], *p.ravel())


def expected(form, spec, answer):
    if form == "wide" or answer != "ok":
        return answer
    kinds = [s.kind for s in spec]
    rep = A.BC_HOST_ROW if A.BC_HOST_ROW in kinds else A.BC_STORAGE_CURVE if A.BC_STORAGE_CURVE in kinds else kinds[0]
    return f"ok {int(any(k in (A.BC_STORAGE, A.BC_STORAGE_CURVE) for k in kinds))} {int(A.BC_HOST_ROW in kinds)} {rep}"


def test_the_library_accepts_what_python_packs(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no system C++ compiler")
    todo = list(boundary_cases())
    lines = []
    for name, form, side, B, L, spec, answer in todo:
        packed = pack_boundary(_pack, form, B, L, spec)
        if form == "wide":
            packed["kind"] = spec.kind
        lines.append(check_line(form, side, B, packed))
    fin = tmp_path / "checks.txt"
    fin.write_text("\n".join(lines) + "\n")
    out = run(build(PACK_DRIVER, tmp_path), ["checks", fin], timeout=600).splitlines()
    assert len(out) == len(todo)
    wrong = [(name, got) for (name, form, _, _, _, spec, answer), got in zip(todo, out) if got != expected(form, spec, answer)]
    assert not wrong, (len(wrong), wrong[:5])
    answers = dict(zip((t[0] for t in todo), out))
    assert answers["curve/mixed_kind_17"] == "Invalid boundary condition." and answers["curve/mixed_host_row"] == f"ok 1 1 {A.BC_HOST_ROW}"
    assert sum(a.startswith("ok") for a in out) == len(out) - 3


# ---- c. no library needed -------------------------------------------------------------------------------------------------------
def test_packing_needs_no_library(tmp_path):
    code = ("import numpy as np\n"
            "from types import SimpleNamespace as S\n"
            "from flowsim_amd import _pack, _abi\n"
            "spec = S(kind=_abi.BC_STORAGE_CURVE, params=dict(surface_area=1e6, curve=[[600.0, 1e6], [601.0, 2e6]]), target=None)\n"
            "p, n, per = _pack.bc_params(spec, 2)\n"
            "assert p.shape == (20,) and n == 20 and per == 0 and p[_abi.SC_NAMES.index('n_curve')] == 2.0\n"
            "assert _abi._lib is None\n")
    env = dict(os.environ, FS_LIB=str(tmp_path / "no_such_library.so"), PYTHONPATH=os.path.join(ROOT, "flow-sim_amd"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
