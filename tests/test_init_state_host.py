"""Host side of the device initial conditions (fs_batch_init_state).

The Brent iteration the normal-depth kernel runs (fs::brent_root, flow-sim_amd/csrc/fs_init_state.hpp) is plain C++: built here
with the system compiler under AddressSanitizer and UBSan and held, root and evaluation count, to scipy.optimize.brentq - the routine
the reference calls (cross_section.py:184-202) - on functions made of + - * sqrt only, which both sides evaluate to the same bits.

The backwater profiles of the 12 polyline channels (tests/golden/init_state_polyline.npz: the reference's own, tools/
gen_init_state_golden.py) pin the host mirror here and the device march in tests/test_gpu_init_state.py."""
import json
import math
import os

import numpy as np
import pytest
from scipy.optimize import brentq

from conftest import GOLDEN, ROOT
from oracle import preissmann_oracle as O
from oracle.gen_random_sweep import build_from_recipe

import host_driver

DRIVER = os.path.join(ROOT, "tests", "init_state", "brent_driver.cpp")

sq = math.sqrt
FUNCTIONS = {
    "cubic": (lambda x: x * x * x - 2.0 * x - 5.0, 2.0, 3.0),
    "sqrt_shift": (lambda x: sq(x) - 1.7, 0.0, 100.0),
    "conveyance_like": (lambda h: 120.0 - (20.0 * h) * (20.0 * h) * sq(20.0 * h) / (20.0 + 2.0 * h) * sq(2e-4) / 0.03, 0.0, 100.0),
    "far_root": (lambda x: (x - 99.999) * (x + 3.0), 0.0, 100.0),
    "flat_then_steep": (lambda x: (x - 1.0) * (x - 1.0) * (x - 1.0) * (x - 1.0) * (x - 1.0) * (x - 1.0) * (x - 1.0) - 1e-9, 0.0, 3.0),
    "root_at_a": (lambda x: x * (x - 5.0) - 0.0, 0.0, 3.0),
    "high_datum": (lambda x: 35.0 - 9.0 * (x - 480.25) * sq(x - 480.25), 480.25, 580.25),
    "no_bracket": (lambda x: x * x + 1.0, -1.0, 2.0),
}


def test_brent_root_is_scipys_brentq(tmp_path):
    exe = host_driver.build(DRIVER, tmp_path, extra_flags=["-ffp-contract=off"])      # the functions must round as Python rounds them
    got = {f[0]: (float(f[1]), int(f[2]), int(f[3])) for f in (line.split() for line in host_driver.run(exe, [], timeout=60).splitlines())}
    assert sorted(got) == sorted(FUNCTIONS)
    for name, (f, a, b) in FUNCTIONS.items():
        root, evals, bracketed = got[name]
        if name == "no_bracket":
            with pytest.raises(ValueError):
                brentq(f, a, b)
            assert not bracketed and root == b and evals == 2
            continue
        want, res = brentq(f, a, b, full_output=True)
        assert bracketed and res.converged
        assert root == want, (name, root, want)                       # the same iterates, so the same bits
        assert evals == res.function_calls, (name, evals, res.function_calls)


POLY = np.load(os.path.join(GOLDEN, "init_state_polyline.npz"))
SWEEP = {i: (fx, m) for i, fx, m in O.sweep_cases(os.path.join(GOLDEN, "random_sweep.npz")) if m["family"] == "polyline"}


def test_the_polyline_fixture_is_what_it_says():
    meta = json.loads(str(POLY["meta"]))
    assert [c["case"] for c in meta["cases"]] == sorted(SWEEP) and len(SWEEP) == 12
    assert all(m["ic"] != "GVF_equation" for _, m in SWEEP.values())          # why the file exists
    for c in meta["cases"]:
        ic = POLY[f"c{c['case']:02d}_initial_conditions"]
        assert ic.shape == (SWEEP[c["case"]][1]["N"], 2) and np.all(ic[:, 1] == SWEEP[c["case"]][1]["Qb"]) and np.all(ic[:, 0] > 0)


@pytest.mark.parametrize("case", sorted(SWEEP))
def test_mirror_marches_the_polyline_backwater_as_the_reference_does(case, capsys):
    _, m = SWEEP[case]
    solver, _, _ = build_from_recipe(dict(m["recipe"], ic="GVF_equation"))
    assert type(solver).__module__.startswith("flowsim_amd")
    ch = solver.channel
    if not ch.conditions_initialized:
        ch.initialize_conditions(solver.number_of_nodes)
    assert "Warning" not in capsys.readouterr().out              # no clamp, no floor: the device flags stay 0 on these
    np.testing.assert_allclose(ch.initial_conditions, POLY[f"c{case:02d}_initial_conditions"], rtol=1e-10, atol=1e-12)
