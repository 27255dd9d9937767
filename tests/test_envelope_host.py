"""Host side of the flood envelopes (fs_batch_envelope): the walk over one series of flow-sim_amd/csrc/fs_envelope.hpp is plain C++.
tests/envelope/envelope_driver.cpp is built here with the system compiler under AddressSanitizer and UBSan, run as a program on
columns of the reference's own histories (tests/golden/akbari.npz, irr_levee.npz, bc_compound_normal.npz) and on made-up series, and
held to np.max / argmax / min / argmin and to a written-out crossing loop."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import host_driver

DRIVER = os.path.join(ROOT, "tests", "envelope", "envelope_driver.cpp")
FIXTURES = ("akbari", "irr_levee", "bc_compound_normal")
FIELDS = ("depth", "flow", "derived_level", "derived_velocity", "derived_froude_number", "derived_top_width")
NAN = float("nan")


def fixture_series():
    """name -> (series, threshold): every column of every field of the three fixtures, against the middle of its range"""
    out = {}
    for name in FIXTURES:
        fx = np.load(os.path.join(GOLDEN, name + ".npz"))
        for f in FIELDS:
            for node in range(fx[f].shape[1]):
                col = np.array(fx[f][:, node])
                out[f"{name}.{f}.{node}"] = (col, 0.5 * (col.min() + col.max()))
    return out


def made_up_series():
    s = np.array([1.0, 3.0, 2.0, 3.0, -1.0, -1.0, 0.5])
    return {
        "empty": (np.array([]), 1.0),
        "single": (np.array([2.5]), 2.5),
        "single_below": (np.array([2.5]), 2.6),
        "all_equal": (np.full(6, 4.25), 4.25),
        "repeated_extremes": (s, 2.5),                       # the maximum 3 at levels 1 and 3, the minimum -1 at 4 and 5
        "nan_in_the_middle": (np.array([1.0, 5.0, NAN, 7.0, NAN, -3.0]), 4.0),
        "nan_first": (np.array([NAN, 5.0, 1.0]), 0.0),
        "threshold_on_a_sample": (s, 3.0),                   # >= counts the two samples that equal it
        "threshold_above_all": (s, 3.5),
        "threshold_below_all": (s, -2.0),
        "threshold_nan": (s, NAN),
        "negative_zero": (np.array([0.0, -0.0, 0.0]), 0.0),
    }


def crossing_loop(v, threshold):
    first, last, count = -1, -1, 0
    for k, x in enumerate(v):
        if x >= threshold:
            if first < 0:
                first = k
            last = k
            count += 1
    return first, last, count


def numbers(a):
    return " ".join(repr(float(v)) for v in a)


@pytest.fixture(scope="module")
def cases():
    return {**fixture_series(), **made_up_series()}


@pytest.fixture(scope="module")
def driver_output(tmp_path_factory, cases):
    tmp = tmp_path_factory.mktemp("envelope")
    exe = host_driver.build(DRIVER, tmp, extra_flags=["-ffp-contract=off"])
    lines = [f"E {name} {len(v)} {float(thr)!r} {numbers(v)}" for name, (v, thr) in cases.items()]
    path = tmp / "records.txt"
    path.write_text("\n".join(lines) + "\n")
    got = {}
    for line in host_driver.run(exe, [path], timeout=60).splitlines():
        f = line.split()
        got[f[1]] = np.array([float(v) for v in f[2:]])
    assert len(got) == len(lines)
    return got


def same(a, b):
    return (np.isnan(a) and np.isnan(b)) or a == b


def test_every_fixture_column_is_numpys(driver_output):
    names = list(fixture_series())
    assert len(names) == len(FIELDS) * (30 + 11 + 41)
    for name, (v, thr) in fixture_series().items():
        mx, mxl, mn, mnl, first, last, count = driver_output[name]
        assert (mx, mxl, mn, mnl) == (np.max(v), np.argmax(v), np.min(v), np.argmin(v)), name
        assert (first, last, count) == crossing_loop(v, thr), name
        assert count == np.sum(v >= thr)


def test_made_up_series_are_numpys(driver_output):
    for name, (v, thr) in made_up_series().items():
        if len(v) == 0:
            continue
        mx, mxl, mn, mnl, first, last, count = driver_output[name]
        with np.errstate(invalid="ignore"):
            want = (np.max(v), np.argmax(v), np.min(v), np.argmin(v))
        assert all(same(g, w) for g, w in zip((mx, mxl, mn, mnl), want)), (name, driver_output[name], want)
        assert (first, last, count) == crossing_loop(v, thr), name


def test_no_sample_one_sample_and_equal_samples(driver_output):
    got = driver_output["empty"]
    assert np.isnan(got[0]) and np.isnan(got[2]) and got[1] == got[3] == -1 and tuple(got[4:]) == (-1, -1, 0)
    assert tuple(driver_output["single"]) == (2.5, 0, 2.5, 0, 0, 0, 1)
    assert tuple(driver_output["single_below"]) == (2.5, 0, 2.5, 0, -1, -1, 0)
    assert tuple(driver_output["all_equal"]) == (4.25, 0, 4.25, 0, 0, 5, 6)


def test_the_first_index_of_a_repeated_extreme_wins(driver_output):
    assert tuple(driver_output["repeated_extremes"]) == (3.0, 1, -1.0, 4, 1, 3, 2)
    assert tuple(driver_output["negative_zero"][[1, 3]]) == (0, 0)


def test_a_nan_sample_is_the_extreme_and_its_first_index_the_level(driver_output):
    got = driver_output["nan_in_the_middle"]
    assert np.isnan(got[0]) and np.isnan(got[2]) and got[1] == got[3] == 2
    assert tuple(got[4:]) == (1, 3, 2)                        # NaN samples are not at or above anything
    got = driver_output["nan_first"]
    assert np.isnan(got[0]) and np.isnan(got[2]) and got[1] == got[3] == 0 and tuple(got[4:]) == (1, 2, 2)


def test_thresholds_on_above_and_below_the_samples_and_not_assessed(driver_output):
    assert tuple(driver_output["threshold_on_a_sample"][4:]) == (1, 3, 2)
    assert tuple(driver_output["threshold_above_all"][4:]) == (-1, -1, 0)
    assert tuple(driver_output["threshold_below_all"][4:]) == (0, 6, 7)
    assert tuple(driver_output["threshold_nan"][4:]) == (-1, -1, 0)
    assert tuple(driver_output["threshold_nan"][:4]) == (3.0, 1, -1.0, 4)      # the extremes do not depend on the threshold
