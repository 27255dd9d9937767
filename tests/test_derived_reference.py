"""tests/derived_reference.py against the reference's own Solver.prepare_results arrays: every fixture under tests/golden that
carries derived_* keys, on the fixture's own history.  Measured over them: the worst relative difference (floor 1e-6) is 8.1e-15,
the Froude number of gerd; the polyline fixtures agree to 0.0.  The bar of 1e-13 leaves a 12-fold margin for another numpy's
summation order."""
import glob
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
import derived_reference as DR
from kernel_harness import rel_err
from oracle import preissmann_oracle as O

BAR = 1e-13


def with_derived():
    out = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))):
        with np.load(path) as f:
            if any(k.startswith("derived_") for k in f.files) and "kind" not in json.loads(str(f["meta"])):
                out.append(path)
    return out


PATHS = with_derived()


def test_the_fixtures_the_helper_is_held_to():
    names = {os.path.basename(p)[:-4] for p in PATHS}
    assert {"akbari", "example", "gerd", "bc_compound_normal", "irr_single", "irr_levee", "irr_mixed", "irr_on_vertex", "irr_storage"} <= names


@pytest.mark.parametrize("path", PATHS, ids=[os.path.basename(p)[:-4] for p in PATHS])
def test_helper_is_the_references_prepare_results(path):
    fx, meta = O.load_fixture(path)
    members = list(range(meta["B"])) if meta.get("B") else [None]
    for m in members:
        p = O.problem_from_fixture(fx, meta, m)
        pick = (lambda a, nd: a) if m is None else (lambda a, nd: a[m] if a.ndim > nd else a)
        h, Q = pick(fx["depth"], 2), pick(fx["flow"], 2)
        d = DR.derived(p.geo, h, Q)
        for f in DR.FIELDS:
            want = pick(fx["derived_" + f], 1 if f == "peak_amplitude" else 2)
            err = rel_err(d[f], want, 1e-6)
            print(os.path.basename(path), m, f, err)
            assert d[f].shape == want.shape and err <= BAR, (f, m, err)
        env = DR.envelope(p.geo, h, Q)
        assert tuple(env) == DR.QUANTITIES
        for q, ref in (("stage", "derived_level"), ("velocity", "derived_velocity"), ("froude_number", "derived_froude_number"),
                       ("top_width", "derived_top_width"), ("depth", "depth"), ("flow", "flow")):
            x = env[q]["series"]
            assert rel_err(x, pick(fx[ref], 2), 1e-6) <= BAR, q
            assert np.array_equal(env[q]["max"], x.max(axis=0)) and np.array_equal(env[q]["max_level"], np.argmax(x, axis=0))
            assert np.array_equal(env[q]["min"], x.min(axis=0)) and np.array_equal(env[q]["min_level"], np.argmin(x, axis=0))


def test_census_counts_vertices_on_the_surface_and_wetted_runs():
    # a W: two channels behind a crest at 1.0
    x, z = np.array([0.0, 1, 2, 3, 4.0]), np.array([2.0, 0.0, 1.0, 0.25, 2.0])
    geo = dict({k: np.zeros(1) for k in O.GEO_KEYS}, irr_npts=np.array([5]), irr_x=x[None], irr_z=z[None])
    on, runs = DR.surface_census(geo, np.array([[0.125], [0.25], [0.5], [1.0], [1.5]]))
    assert on[:, 0].tolist() == [False, True, False, True, False] and runs[:, 0].tolist() == [1, 1, 2, 2, 1]
    # the reference's convention at the crest (z = 1.0 = the stage): the two edges next to it contribute nothing, though their
    # other ends are under water; what is left is the two outer edges up to their water's-edge points
    A, T = DR.area_top(geo, np.array([[1.0]]))
    cx = (3.0 + 0.75 / 1.75) - 3.0
    assert abs(T[0, 0] - (0.5 + cx)) <= 1e-15 and abs(A[0, 0] - (0.25 + 0.375 * cx)) <= 1e-15
    assert abs(T[0, 0] - (0.5 + 1.5 + 1.0 + cx)) > 1.0, "not the geometric width below the stage"


def test_fp32_restatement_tracks_the_helper():
    fx, meta = O.load_fixture(os.path.join(GOLDEN, "bc_compound_normal.npz"))
    p = O.problem_from_fixture(fx, meta)
    half = np.where(np.arange(p.nt) % 2 == 0, 0.5, 1.0)[:, None]          # every other level below the banks
    h, Q = (fx["depth"] * half).astype(np.float32), fx["flow"].astype(np.float32)
    assert np.any((p.geo["is_compound"] > 0.5) & (h > p.geo["h_bf"])) and np.any(h <= p.geo["h_bf"])          # both branches
    lo, hi = DR.derived_f32(p.geo, h, Q), DR.derived(p.geo, h, Q)
    for f in DR.FIELDS:
        err = rel_err(lo[f].astype(np.float64), hi[f], 1e-6)
        print(f, err)
        assert err <= 64 * 2.0 ** -24, f          # a handful of roundings each, no cancellation at these depths
