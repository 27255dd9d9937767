"""Host side of the ensemble post-processing (fs_batch_summarize, fs_batch_lookup): the per-series walks of
flow-sim_amd/csrc/fs_reduce.hpp are plain C++.  tests/reduce/reduce_driver.cpp is built here with the system compiler under
AddressSanitizer and UBSan, run as a program on the boundary columns of the reference's own histories (tests/golden/akbari.npz,
example.npz, gerd.npz, gerd_full.npz) and held to numpy and to the reference's loops evaluated in Python."""
import json
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from flowsim_amd import _abi as A
from flowsim_amd.ensemble import summary_text

import host_driver

DRIVER = os.path.join(ROOT, "tests", "reduce", "reduce_driver.cpp")
EPS = 2.0 ** -52
SUMMARY_CASES = ("akbari", "example", "gerd_full")
QUERIES = np.array([1562.5, 2100.0, 2500.0, 3000.0, 1e9])
TARGET = np.array([497.5, 500.0, 502.0, 505.0, 507.0])


def columns(name):
    fx = np.load(os.path.join(GOLDEN, name + ".npz"))
    return fx["depth"][:, 0], fx["flow"][:, 0], fx["depth"][:, -1], fx["flow"][:, -1]


def lookup_cases():
    """name -> (xp, fp): upstream stage over upstream flow of the two GERD histories, and a series with a repeated abscissa"""
    out = {}
    for name in ("gerd", "gerd_full"):
        h_in, q_in, _, _ = columns(name)
        out[name] = (q_in, h_in + 480.25)
    out["repeated"] = (np.array([1000.0, 1562.5, 1562.5, 1562.5, 2500.0, 2500.0, 4000.0]), np.array([1.0, 2.0, 3.0, 5.0, 7.0, 11.0, 13.0]))
    out["single"] = (np.array([2000.0]), np.array([4.5]))
    return out


def numbers(a):
    return " ".join(repr(float(v)) for v in a)


@pytest.fixture(scope="module")
def driver_output(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("reduce")
    exe = host_driver.build(DRIVER, tmp, extra_flags=["-ffp-contract=off"])
    lines = []
    for name in SUMMARY_CASES:
        cols = columns(name)
        lines.append(f"S {name} {len(cols[0])} " + " ".join(numbers(c) for c in cols))
        lines.append(f"S {name}_first {1} " + " ".join(numbers(c[:1]) for c in cols))
    lines.append("S empty 0")
    for name, (xp, fp) in lookup_cases().items():
        lines.append(f"L {name} {len(xp)} {len(QUERIES)} {numbers(xp)} {numbers(fp)} {numbers(QUERIES)} {numbers(TARGET)}")
    path = tmp / "records.txt"
    path.write_text("\n".join(lines) + "\n")
    got = {}
    for line in host_driver.run(exe, [path], timeout=60).splitlines():
        f = line.split()
        got[(f[0], f[1])] = np.array([float(v) for v in f[2:]])
    assert len(got) == len(lines)
    return got


def summary_of(got, name):
    return dict(zip(A.SUM_ROWS, got[("S", name)]))


def reference_median_level(q):
    """solver.py:219-229 as written"""
    cumulative = [np.sum(q[:i]) for i in range(q.size)]
    for i in range(len(cumulative)):
        if cumulative[i] >= 0.5 * cumulative[-1]:
            return i
    raise AssertionError("the reference's loop found no level")


def median_margin_ok(q):
    """no cum_i lies within the summation bound (sequential against pairwise over m levels) of its threshold"""
    cum = np.array([np.sum(q[:i]) for i in range(q.size)])
    bound = q.size * EPS * np.sum(np.abs(q))
    return bool(np.all(np.abs(cum - 0.5 * cum[-1]) > bound))


def test_the_header_and_the_binding_name_the_same_rows():
    text = open(os.path.join(ROOT, "include", "flowsim_abi.h")).read()
    start = text.index("enum { FS_SUM_LEVELS")
    body = text[start:text.index("FS_SUM_NROWS", start)]
    names = re.findall(r"FS_SUM_([A-Z_]+)", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert tuple(n.lower() for n in names) == A.SUM_ROWS


@pytest.mark.parametrize("name", SUMMARY_CASES)
def test_peaks_and_their_levels_are_numpys(driver_output, name):
    s = summary_of(driver_output, name)
    cols = dict(zip(("h_in", "q_in", "h_out", "q_out"), columns(name)))
    assert s["levels"] == len(cols["q_in"])
    for key, col in cols.items():
        assert s["peak_" + key] == np.max(col), key
        assert s["peak_" + key + "_level"] == np.argmax(col), key


@pytest.mark.parametrize("name", SUMMARY_CASES)
def test_sums_are_within_the_summation_bound_of_numpys(driver_output, name):
    s = summary_of(driver_output, name)
    _, q_in, _, q_out = columns(name)
    m = len(q_in)
    for got, terms in ((s["q_in"], q_in), (s["q_out"], q_out), (s["q_net"], q_in - q_out)):
        bound = m * EPS * np.sum(np.abs(terms))
        print(name, got, np.sum(terms), abs(got - np.sum(terms)), bound)
        assert abs(got - np.sum(terms)) <= bound


@pytest.mark.parametrize("name", SUMMARY_CASES)
def test_median_volume_levels_are_the_references(driver_output, name):
    s = summary_of(driver_output, name)
    _, q_in, _, q_out = columns(name)
    # every fixture passes the margin test on both columns, so none is left out of the assertion (akbari and example must stay in)
    assert median_margin_ok(q_in) and median_margin_ok(q_out), name
    assert s["median_in_level"] == reference_median_level(q_in)
    assert s["median_out_level"] == reference_median_level(q_out)


def test_one_level_and_no_level(driver_output):
    for name in SUMMARY_CASES:
        s = summary_of(driver_output, name + "_first")
        h_in, q_in, h_out, q_out = (c[0] for c in columns(name))
        assert s["levels"] == 1 and s["median_in_level"] == 0 and s["median_out_level"] == 0
        assert (s["q_in"], s["q_out"], s["q_net"]) == (q_in, q_out, q_in - q_out)
        assert (s["peak_h_in"], s["peak_q_in"], s["peak_h_out"], s["peak_q_out"]) == (h_in, q_in, h_out, q_out)
        assert all(s[k] == 0 for k in A.SUM_ROWS if k.endswith("_level"))
    s = summary_of(driver_output, "empty")
    assert s["levels"] == 0 and s["q_in"] == 0 and s["q_out"] == 0 and s["q_net"] == 0
    assert all(np.isnan(s[k]) for k in A.SUM_ROWS if k.startswith("peak_") and not k.endswith("_level"))
    assert all(s[k] == -1 for k in A.SUM_ROWS if k.endswith("_level"))


@pytest.mark.parametrize("name", ["akbari", "example"])
def test_summary_text_is_the_references(driver_output, name):
    meta = json.loads(str(np.load(os.path.join(GOLDEN, name + ".npz"))["meta"]))
    s = {k: np.array([v]) for k, v in summary_of(driver_output, name).items()}
    dt = int(meta["dt"])
    text = summary_text(s, 0, dt, meta["dx"], (meta["nt"] - 1) * dt)
    assert text == str(np.load(os.path.join(GOLDEN, "result_summaries.npz"))[name])


def test_the_negative_outflow_of_example_is_in_the_fixture():
    q_out = columns("example")[3]
    assert np.min(q_out[:3]) < -999.0                 # why "first i" has to be taken literally: the cumulative outflow is not monotone
    assert np.any(np.diff(np.cumsum(q_out)) < 0)


def test_lookup_is_np_interp_where_the_abscissae_never_descend(driver_output):
    for name in ("gerd", "repeated", "single"):
        xp, fp = lookup_cases()[name]
        assert np.all(np.diff(xp) >= 0)
        got = driver_output[("L", name)]
        want = np.interp(QUERIES, xp, fp)
        bound = 8 * EPS * np.max(np.abs(fp))
        print(name, got[2:], want, np.max(np.abs(got[2:] - want)), bound)
        assert got[0] == 0
        assert np.all(np.abs(got[2:] - want) <= bound)
        rmse = np.mean((want - TARGET) ** 2) ** 0.5
        assert abs(got[1] - rmse) <= 8 * EPS * rmse
    xp, fp = lookup_cases()["gerd"]
    assert len(xp) == 49 and np.all(np.diff(xp) > 0)
    assert QUERIES[0] < xp[0] and xp[0] < QUERIES[1] < xp[-1] and QUERIES[-1] > xp[-1]      # clamped below and above, and inside
    # queried exactly at a repeated abscissa: the last of the repeats, as numpy
    xp, fp = lookup_cases()["repeated"]
    assert driver_output[("L", "repeated")][2] == np.interp(1562.5, xp, fp) == 5.0
    assert driver_output[("L", "repeated")][4] == np.interp(2500.0, xp, fp) == 11.0


def test_lookup_flags_the_descending_flow_of_gerd_full(driver_output):
    xp, _ = lookup_cases()["gerd_full"]
    assert np.sum(np.diff(xp) < 0) == 167
    got = driver_output[("L", "gerd_full")]
    assert int(got[0]) & 1 == 1
    assert np.all(np.isfinite(got[2:]))
