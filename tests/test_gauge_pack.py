"""The argument packing of the interior gauges on the CPU (flowsim_amd/_pack.py: gauge_positions, gauge_options and what the
PreissmannBatch methods hand to the C ABI), the header and the binding naming the same rows, and the new entry points answered without
a device: a NULL handle is refused with a text that names the entry point.

The methods are run on a batch whose library is a recorder: every call is kept with the values its ctypes arguments point at, so what
is held here is what the library would read - dtypes, shapes, the per-reach flag, NULL where the caller gave nothing."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from flowsim_amd import _abi as A
from flowsim_amd import _pack as P
from flowsim_amd import ensemble
from flowsim_amd.batch import PreissmannBatch

EPS = np.finfo(np.float64).eps
NAN = float("nan")


# ---- the header and the binding -------------------------------------------------------------------------------------------------------
def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flowsim_abi.h")).read(), flags=re.S)


def test_the_header_and_the_binding_name_the_same_rows():
    text = header_text()
    body = text[text.index("enum { FS_GAUGE_DEPTH = 0"):]
    rows = re.findall(r"FS_GAUGE_([A-Z_]+)", body[:body.index("FS_GAUGE_NROWS")])
    assert tuple(s.lower() for s in rows) == A.GAUGE_ROWS and len(A.GAUGE_ROWS) == 4      # the hydrograph block's shape
    body = text[text.index("enum { FS_GS_COUNT = 0"):]
    rows = re.findall(r"FS_GS_([A-Z_]+)", body[:body.index("FS_GS_NROWS")])
    assert tuple(s.lower() for s in rows) == A.GS_ROWS
    assert int(re.search(r"#define FS_GAUGE_MAX (\d+)", text).group(1)) == A.GAUGE_MAX == 32
    assert int(re.search(r"#define FS_ABI_VERSION (\d+)", text).group(1)) == A.ABI_VERSION == 3
    for name in ("fs_batch_set_gauges", "fs_batch_gauges", "fs_batch_get_gauges", "fs_batch_gauges_device_ptr", "fs_batch_gauge_bands",
                 "fs_batch_gauge_lookup", "fs_batch_gauge_score"):
        assert name in A.SIGNATURES and re.search(r"\b" + name + r"\s*\(", text), name


# ---- gauge_positions ------------------------------------------------------------------------------------------------------------------
def test_exact_multiples_sit_on_a_node():
    dx = 250.0
    node, weight = P.gauge_positions([0.0, dx, 7 * dx, 119 * dx, 120 * dx], dx, 121)
    assert node.dtype == np.int32 and weight.dtype == np.float64 and node.flags.c_contiguous and weight.flags.c_contiguous
    assert node.tolist() == [0, 1, 7, 119, 120] and np.all(weight == 0.0) and not np.any(np.signbit(weight))
    for dx in (0.1, 1.0 / 3.0, 123.456, 1e-3, 2.0 ** 0.5):
        k = np.arange(0, 64)
        node, weight = P.gauge_positions(k * dx, dx, 64)                          # k * dx / dx need not be k: the snap makes it so
        assert node.tolist() == k.tolist() and np.all(weight == 0.0), dx


def test_between_two_nodes():
    node, weight = P.gauge_positions([62.5, 300.0, 29999.0], 250.0, 121)
    assert node.tolist() == [0, 1, 119] and weight.tolist() == [0.25, 300.0 / 250.0 - 1.0, 29999.0 / 250.0 - 119.0]
    assert np.all((weight >= 0.0) & (weight < 1.0))


def test_the_snap_rule():
    for s in (1.0, 7.0, 100.0, 4000.0):
        tol = 4 * EPS * max(1.0, s)
        inside, outside = s + 0.9 * tol, s + 1.5 * tol
        node, weight = P.gauge_positions([inside, s - 0.9 * tol, outside, s - 1.5 * tol], 1.0, 5000)
        assert node.tolist() == [int(s), int(s), int(s), int(s) - 1], s
        assert weight[0] == 0.0 and weight[1] == 0.0 and 0.0 < weight[2] < 1e-11 and 1.0 - 1e-11 < weight[3] < 1.0, (s, weight)
    node, weight = P.gauge_positions([2.0 ** -60], 1.0, 3)                          # within 4 eps max(1, .) of node 0
    assert (node[0], weight[0]) == (0, 0.0)


def test_the_end_of_the_reach():
    for nodes, dx in ((121, 250.0), (2, 0.1), (33, 1.0 / 3.0), (4097, 123.456)):
        node, weight = P.gauge_positions([(nodes - 1) * dx], dx, nodes)
        assert (node[0], weight[0]) == (nodes - 1, 0.0), (nodes, dx)


def test_out_of_range_and_mixed_shapes_raise():
    for x in (-1e-9, 30000.0001, np.inf, -np.inf):
        with pytest.raises(ValueError, match="outside the reach|must be finite"):
            P.gauge_positions([10.0, x], 250.0, 121)
    with pytest.raises(ValueError, match="must be finite"):
        P.gauge_positions([NAN], 250.0, 121)
    with pytest.raises(ValueError, match="disagree on the number of reaches"):
        P.gauge_positions([1.0], [250.0, 250.0], [121, 121, 121])
    with pytest.raises(ValueError, match="disagree on the number of reaches"):
        P.gauge_positions(np.ones((3, 2)), [250.0, 250.0], 121)
    with pytest.raises(ValueError, match=r"chainage is \[G\] or \[B, G\]"):
        P.gauge_positions(5.0, 250.0, 121)
    with pytest.raises(ValueError, match=r"chainage is \[G\] or \[B, G\]"):
        P.gauge_positions([1.0], np.ones((2, 2)), 121)
    with pytest.raises(ValueError, match="nodes must be integers"):
        P.gauge_positions([1.0], 250.0, 121.0)
    with pytest.raises(ValueError, match="nodes >= 2 and dx > 0"):
        P.gauge_positions([0.0], 250.0, 1)
    with pytest.raises(ValueError, match="nodes >= 2 and dx > 0"):
        P.gauge_positions([0.0], [250.0, 0.0], 5)


def test_per_reach_spacing_and_node_counts():
    dx, nodes = np.array([100.0, 250.0, 0.5]), np.array([9, 2, 33])
    node, weight = P.gauge_positions([0.0, 0.25], dx, 33)                           # one list of chainages, every reach its own dx
    assert node.shape == weight.shape == (3, 2) and node.dtype == np.int32
    assert node.tolist() == [[0, 0], [0, 0], [0, 0]] and weight[:, 1].tolist() == [0.0025, 0.001, 0.5]
    x = np.stack([[800.0, 50.0], [250.0, 125.0], [16.0, 15.75]])
    node, weight = P.gauge_positions(x, dx, nodes)
    assert node.tolist() == [[8, 0], [1, 0], [32, 31]] and weight.tolist() == [[0.0, 0.5], [0.0, 0.5], [0.0, 0.5]]
    with pytest.raises(ValueError, match="outside the reach"):
        P.gauge_positions(x + np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 0.0]]), dx, nodes)      # beyond the two-node reach's own end
    node, weight = P.gauge_positions([[3.0], [4.5]], 1.5, 9)                         # per-reach chainage alone
    assert node.tolist() == [[2], [3]] and np.all(weight == 0.0)


# ---- gauge_options --------------------------------------------------------------------------------------------------------------------
def test_the_runners_keyword():
    chainage, every, q, observed, signal, rows = P.gauge_options(dict(chainage=[100.0, 2000.0]))
    assert chainage.tolist() == [100.0, 2000.0] and (every, observed, signal, rows) == (1, None, "stage", True) and q.tolist() == [0.05, 0.5, 0.95]
    obs = np.full((1, 5), NAN)
    chainage, every, q, observed, signal, rows = P.gauge_options(dict(chainage=(5.0,), every=np.int64(24), quantiles=(), observed=obs, signal="flow",
                                                                      rows=False))
    assert (every, signal, rows, len(q)) == (24, "flow", False, 0) and type(every) is int and observed.shape == (1, 5)
    with pytest.raises(ValueError, match=r"gauges: unknown keys \['chanage'\]"):
        P.gauge_options(dict(chanage=[1.0]))
    with pytest.raises(ValueError, match="chainage is required"):
        P.gauge_options(dict(every=2))
    for bad in (0, -2, 1.5, "3", True, None):
        with pytest.raises(ValueError, match="every must be an integer >= 1"):
            P.gauge_options(dict(chainage=[1.0], every=bad))
    with pytest.raises(ValueError, match="unknown gauge signal 'level'"):
        P.gauge_options(dict(chainage=[1.0], signal="level"))
    with pytest.raises(ValueError, match="quantile levels must be in"):
        P.gauge_options(dict(chainage=[1.0], quantiles=(1.5,)))
    for bad in ([], np.ones((2, 2)), np.ones(A.GAUGE_MAX + 1)):
        with pytest.raises(ValueError, match=r"chainage is \[G\] with 1 <= G <= 32"):
            P.gauge_options(dict(chainage=bad))
    for run in (ensemble.run_manning_ensemble, ensemble.run_scenario_ensemble, ensemble.run_geometry_ensemble):
        assert inspect.signature(run).parameters["gauges"].default is None


def test_signals_observations_and_position_arrays():
    assert [P.gauge_row(k) for k in A.GAUGE_ROWS] == [0, 1, 2, 3] and P.gauge_row(2) == 2 and P.gauge_row(np.int32(3)) == 3
    with pytest.raises(ValueError, match="unknown gauge signal"):
        P.gauge_row("froude_number")
    o, per_reach = P.gauge_observed([1.0, NAN, 3.0], 3, 5)
    assert per_reach == 0 and o.dtype == np.float64 and np.isnan(o[1])               # "no observation" stays
    o, per_reach = P.gauge_observed(np.zeros((3, 5), dtype=np.float32).T.copy().T, 3, 5)
    assert per_reach == 1 and o.flags.c_contiguous and o.dtype == np.float64
    with pytest.raises(ValueError, match=r"observed must be \[n\] = \[3\] or \[n, B\] = \[3, 5\]"):
        P.gauge_observed(np.zeros((5, 3)), 3, 5)
    node, weight, per_reach = P.gauge_arrays([0, 3], [0.0, 0.5], 7)
    assert (node.dtype, weight.dtype, per_reach) == (np.int32, np.float64, 0)
    node, weight, per_reach = P.gauge_arrays(np.zeros((7, 2)), np.zeros((7, 2)), 7)
    assert per_reach == 1 and node.shape == (7, 2)
    for node, weight in (([0, 1], [0.0]), (np.zeros((3, 2)), np.zeros((3, 2))), (0, 0.0)):
        with pytest.raises(ValueError, match="node and weight are both"):
            P.gauge_arrays(node, weight, 7)


# ---- what the methods hand to the library ---------------------------------------------------------------------------------------------
class Recorder:
    """stands where the loaded library stands: every fs_* call returns 0 and is kept as (name, [argument values]); a pointer argument
    is kept as the ctypes pointer itself (None: NULL), which read() turns into the values behind it"""

    def __init__(self, level):
        self.calls, self.level = [], level

    def fs_batch_level(self, h):
        return self.level

    def __getattr__(self, name):
        if not name.startswith("fs_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, list(args)))
            return 0
        return call


def read(ptr, n):
    return None if ptr is None else [ptr[i] for i in range(n)]


def recorded_batch(B=3, N=9, L=6, level=4):
    b = object.__new__(PreissmannBatch)
    b.B, b.N, b.L, b._h, b._lib, b.gauge_positions = B, N, L, 1234, Recorder(level), None
    return b


def test_set_gauges_packs_shared_and_per_reach_positions():
    b = recorded_batch()
    node, weight = b.set_gauges(node=[0, 8, 7, 3, 3], weight=[0.0, 0.0, 0.5, 0.25, 0.25])
    name, (h, G, pn, pw, per_reach) = b._lib.calls[-1]
    assert (name, h, G, per_reach) == ("fs_batch_set_gauges", 1234, 5, 0)
    assert isinstance(pn, A._I) and isinstance(pw, A._D)
    assert read(pn, 5) == [0, 8, 7, 3, 3] and read(pw, 5) == [0.0, 0.0, 0.5, 0.25, 0.25]
    assert b.gauge_positions[0] is node and b.gauge_positions[1] is weight
    b.set_gauges(chainage=[0.0, 625.0], dx=250.0)
    name, (h, G, pn, pw, per_reach) = b._lib.calls[-1]
    assert (G, per_reach) == (2, 0) and read(pn, 2) == [0, 2] and read(pw, 2) == [0.0, 0.5]
    b.set_gauges(chainage=[0.0, 2.0], dx=[1.0, 2.0, 4.0], nodes=[9, 2, 5])        # per reach: [B, G], row by row
    name, (h, G, pn, pw, per_reach) = b._lib.calls[-1]
    assert (G, per_reach) == (2, 1) and read(pn, 6) == [0, 2, 0, 1, 0, 0] and read(pw, 6) == [0.0, 0.0, 0.0, 0.0, 0.0, 0.5]
    b.set_gauges(node=[], weight=[])                                                  # no gauges: the library frees the block
    assert b._lib.calls[-1][1][1] == 0
    n_calls = len(b._lib.calls)
    for kw in (dict(), dict(chainage=[1.0]), dict(chainage=[1.0], dx=1.0, node=[0], weight=[0.0]), dict(node=[0])):
        with pytest.raises(ValueError, match="set_gauges:"):
            b.set_gauges(**kw)
    with pytest.raises(ValueError, match="node and weight are both"):
        b.set_gauges(node=np.zeros((2, 2)), weight=np.zeros((2, 2)))                 # [B, G] of another B
    assert len(b._lib.calls) == n_calls                                              # nothing reached the library


def test_ranges_rows_bands_lookup_and_score():
    b = recorded_batch(B=3, L=6, level=4)
    b.gauges()
    assert b._lib.calls[-1] == ("fs_batch_gauges", [1234, 0, 5])
    b.gauges(2, 2)
    assert b._lib.calls[-1] == ("fs_batch_gauges", [1234, 2, 2])
    b.gauges(current=True)
    assert b._lib.calls[-1] == ("fs_batch_gauges", [1234, -1, 1])
    with pytest.raises(ValueError, match="current=True evaluates the current state"):
        b.gauges(1, current=True)
    rows = b.gauge_rows(1, 1)
    name, (h, g, first, n, out) = b._lib.calls[-1]
    assert (name, g, first, n) == ("fs_batch_get_gauges", 1, 1, 4) and rows.shape == (4, 4, 3) and C.addressof(out.contents) == rows.ctypes.data
    bands = b.gauge_bands(2, (0.5, 0.95), 1, 3)
    name, (h, g, first, n, q, n_q, mom, qu, cnt) = b._lib.calls[-1]
    assert (name, g, first, n, n_q) == ("fs_batch_gauge_bands", 2, 1, 3, 2) and read(q, 2) == [0.5, 0.95]
    assert bands["quantiles"].shape == (3, 4, 2) and bands["min"].shape == (3, 4) and bands["n_members"].dtype == np.int32
    bands = b.gauge_bands(0, ())
    assert b._lib.calls[-1][1][4] is None and b._lib.calls[-1][1][7] is None and bands["quantiles"].shape == (5, 4, 0)      # NULL, not empty arrays
    with pytest.raises(ValueError, match="at most 16 quantile levels"):
        b.gauge_bands(0, np.linspace(0, 1, 17))
    res = b.gauge_lookup(1, "flow", "stage", [10.0, 20.0], y_offset=2.5, target=[1.0, 2.0], first=1)
    name, (h, g, first, n, x_row, y_row, off, xq, n_q, tgt, values, rmse, info) = b._lib.calls[-1]
    assert (name, g, first, n, x_row, y_row, n_q) == ("fs_batch_gauge_lookup", 1, 1, 4, 1, 2, 2)
    assert read(off, 3) == [2.5] * 3 and read(xq, 2) == [10.0, 20.0] and read(tgt, 2) == [1.0, 2.0]
    assert res["values"].shape == (2, 3) and res["rmse"].shape == (3,) and res["monotone"].shape == (3,)
    res = b.gauge_lookup(0, 0, 3, [1.0])
    args = b._lib.calls[-1][1]
    assert (args[4], args[5]) == (0, 3) and args[6] is None and args[9] is None and args[11] is None and res["rmse"] is None
    with pytest.raises(ValueError, match="target must have the shape of xq"):
        b.gauge_lookup(0, 0, 3, [1.0, 2.0], target=[1.0])
    obs = [400.0, NAN, 401.0, 402.0, NAN]
    score = b.gauge_score(1, "stage", obs)
    name, (h, g, signal, first, n, po, per_reach, out) = b._lib.calls[-1]
    assert (name, g, signal, first, n, per_reach) == ("fs_batch_gauge_score", 1, 2, 0, 5, 0)
    got = read(po, 5)
    assert got[0] == 400.0 and np.isnan(got[1]) and got[2:4] == [401.0, 402.0] and np.isnan(got[4])
    assert tuple(score) == A.GS_ROWS and all(v.shape == (3,) for v in score.values())
    b.gauge_score(0, 3, np.arange(6.0).reshape(2, 3), first=2, n=2)
    name, (h, g, signal, first, n, po, per_reach, out) = b._lib.calls[-1]
    assert (signal, first, n, per_reach) == (3, 2, 2, 1) and read(po, 6) == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0]
    with pytest.raises(ValueError, match=r"observed must be \[n\] = \[5\]"):
        b.gauge_score(0, "stage", [1.0, 2.0])
    b.gauges_device_ptr(3)
    assert b._lib.calls[-1] == ("fs_batch_gauges_device_ptr", [1234, 3])


def test_the_methods_exist_with_their_defaults():
    def defaults(fn):
        return [(k, p.default) for k, p in list(inspect.signature(fn).parameters.items())[1:]]
    assert defaults(PreissmannBatch.set_gauges)[:3] == [("chainage", None), ("node", None), ("weight", None)]
    assert defaults(PreissmannBatch.gauges) == [("first", 0), ("n", None), ("current", False)]
    assert defaults(PreissmannBatch.gauge_rows) == [("g", inspect.Parameter.empty), ("first", 0), ("n", None)]
    assert defaults(PreissmannBatch.gauge_bands) == [("g", inspect.Parameter.empty), ("quantiles", (0.05, 0.5, 0.95)), ("first", 0), ("n", None)]
    assert [k for k, _ in defaults(PreissmannBatch.gauge_lookup)][:4] == ["g", "x_row", "y_row", "xq"]
    assert defaults(PreissmannBatch.gauge_score) == [("g", inspect.Parameter.empty), ("signal", inspect.Parameter.empty),
                                                     ("observed", inspect.Parameter.empty), ("first", 0), ("n", None)]


# ---- the library without a device -----------------------------------------------------------------------------------------------------
def test_a_null_handle_is_refused_with_a_text():
    lib = A.lib()
    out = np.zeros(64)
    ptr = out.ctypes.data_as(C.POINTER(C.c_double))
    node = np.zeros(1, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    calls = {
        "fs_batch_set_gauges": lambda: lib.fs_batch_set_gauges(None, 1, node, ptr, 0),
        "fs_batch_gauges": lambda: lib.fs_batch_gauges(None, 0, 1),
        "fs_batch_get_gauges": lambda: lib.fs_batch_get_gauges(None, 0, 0, 1, ptr),
        "fs_batch_gauge_bands": lambda: lib.fs_batch_gauge_bands(None, 0, 0, 1, None, 0, ptr, None, None),
        "fs_batch_gauge_lookup": lambda: lib.fs_batch_gauge_lookup(None, 0, 0, 1, 0, 1, None, ptr, 1, None, ptr, None, None),
        "fs_batch_gauge_score": lambda: lib.fs_batch_gauge_score(None, 0, 2, 0, 1, ptr, 0, ptr),
    }
    for name, call in calls.items():
        assert call() == -1
        assert name in lib.fs_last_error().decode(), name
    assert not lib.fs_batch_gauges_device_ptr(None, 0)
