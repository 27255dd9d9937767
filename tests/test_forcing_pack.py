"""The library-free packers of the forcing calls (flowsim_amd/_pack.py: sample_tables, table_index, pool_descriptor, weir_scale)
against hand-built arrays, forcing.PoolSpec of the GERD case against the case's constants, and every rejection."""
import numpy as np
import pytest

from flowsim_amd import _abi as A
from flowsim_amd import _pack as P
from flowsim_amd.forcing import PoolSpec


def test_sample_tables():
    t, v = P.sample_tables([0, 10, 30], [1.0, 2.0, 4.0])
    assert t.dtype == v.dtype == np.float64 and t.flags.c_contiguous and v.flags.c_contiguous
    assert np.array_equal(t, [0.0, 10.0, 30.0]) and np.array_equal(v, [[1.0, 2.0, 4.0]])
    t, v = P.sample_tables(np.array([0.0, 1.0])[::1], np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]]).T[::, ::].T)
    assert v.shape == (3, 2) and v.flags.c_contiguous
    t, v = P.sample_tables([5.0], [7.0])
    assert t.shape == (1,) and v.shape == (1, 1)
    for times, values in (([0.0, 0.0], [1.0, 2.0]), ([1.0, 0.0], [1.0, 2.0]), ([0.0, np.nan], [1.0, 2.0]), ([0.0, 1.0], [1.0, 2.0, 3.0]),
                          ([], []), ([0.0, 1.0], [[1.0, 2.0, 3.0]])):
        with pytest.raises(ValueError):
            P.sample_tables(times, values)


def test_table_index():
    assert P.table_index(None, 2, 4) is None
    idx = P.table_index([0, 1, 1, 0], 2, 4)
    assert idx.dtype == np.int32 and np.array_equal(idx, [0, 1, 1, 0])
    assert np.array_equal(P.table_index(1, 2, 3), [1, 1, 1])
    for bad in ([0, 2, 0, 0], [-1, 0, 0, 0]):
        with pytest.raises(ValueError, match="table_of"):
            P.table_index(bad, 2, 4)
    with pytest.raises(ValueError):
        P.table_index([0, 1], 2, 4)                     # wrong length


def test_pool_descriptor():
    z, v, w = P.pool_descriptor([500.0, 600.0, 650.0], [1.0, 50.0, 90.0], [(2.0, 610.0, 620.0), (3.0, 640.0)])
    assert np.array_equal(z, [500.0, 600.0, 650.0]) and np.array_equal(v, [1.0, 50.0, 90.0])
    assert w.dtype == np.float64 and w.flags.c_contiguous
    assert np.array_equal(w, [[2.0, 610.0, 620.0, 0.0], [3.0, 640.0, 640.0, 0.0]])          # no ramp: the top is the crest
    assert P.pool_descriptor([0.0, 1.0], [0.0, 1.0], [])[2].shape == (0, 4)
    with pytest.raises(ValueError, match="same length"):
        P.pool_descriptor([0.0, 1.0], [0.0, 1.0, 2.0], [])
    with pytest.raises(ValueError, match="points"):
        P.pool_descriptor(np.arange(65.0), np.arange(65.0), [])                             # curve too long
    with pytest.raises(ValueError, match="points"):
        P.pool_descriptor([1.0], [1.0], [])
    with pytest.raises(ValueError, match="increasing"):
        P.pool_descriptor([0.0, 2.0, 2.0], [0.0, 1.0, 2.0], [])
    with pytest.raises(ValueError, match="weirs"):
        P.pool_descriptor([0.0, 1.0], [0.0, 1.0], [(1.0, 0.5)] * 9)                         # more than 8 weirs
    with pytest.raises(ValueError, match="a weir is"):
        P.pool_descriptor([0.0, 1.0], [0.0, 1.0], [(1.0,)])
    assert P.pool_descriptor(np.arange(64.0), np.arange(64.0), [(1.0, 0.5)] * 8)[2].shape == (8, 4)


def test_weir_scale():
    assert P.weir_scale(None, 3, 5) is None
    s = P.weir_scale([0.0, 1.0, 0.5], 3, 2)
    assert s.flags.c_contiguous and np.array_equal(s, [[0.0, 0.0], [1.0, 1.0], [0.5, 0.5]])
    full = np.arange(6.0).reshape(3, 2)
    assert np.array_equal(P.weir_scale(full, 3, 2), full)
    for bad in (np.ones(2), np.ones((2, 3)), np.ones((3, 3))):
        with pytest.raises(ValueError, match="weir_scale"):
            P.weir_scale(bad, 3, 2)


def test_pool_spec_rejections():
    ok = dict(curve_stage=[0.0, 1.0], curve_volume=[0.0, 1.0], weirs=[(1.0, 0.5)], base_flow=1.0, vol_scale=1e-6, z_lo=0.0, z_hi=1.0)
    PoolSpec(**ok)
    for change in (dict(z_lo=1.0), dict(z_lo=2.0), dict(vol_scale=0.0), dict(base_flow=-1.0), dict(curve_stage=[1.0, 0.0]),
                   dict(weirs=[(1.0, 0.5)] * 9), dict(curve_volume=[0.0, 1.0, 2.0])):
        with pytest.raises(ValueError):
            PoolSpec(**dict(ok, **change))


def test_pool_spec_of_the_case_is_its_constants():
    from cases.gerd_roseires import gerd_discharge as gd
    from cases.gerd_roseires import settings
    spec = gd.GerdHydrograph.pool_spec()
    curve = np.loadtxt(settings.gerd_volume_curve_path, delimiter=",")
    z, v, w = spec.arrays()
    assert np.array_equal(v, curve[:, 0]) and np.array_equal(z, curve[:, 1]) and 2 <= len(z) <= A.POOL_MAX_CURVE
    assert np.array_equal(w, [[gd.C_GATED, gd.CREST_GATED, gd.CREST_STEPPED, 0.0], [gd.C_STEPPED, gd.CREST_STEPPED, gd.CREST_STEPPED, 0.0],
                              [gd.C_EMERGENCY, gd.CREST_EMERGENCY, gd.CREST_EMERGENCY, 0.0]])
    assert (spec.base_flow, spec.vol_scale, spec.z_lo, spec.z_hi) == (gd.TURBINE_FLOW, 1e-6, 624.9, 645)
    # the capacity the spec describes is the one build() uses
    for level in (620.0, 624.9, 630.0, 640.0, 641.0, 644.5):
        q = spec.base_flow
        for c, crest, top, _ in w:
            ramp = 1.0 if top <= crest else min(max((level - crest) / (top - crest), 0.0), 1.0)
            q += c * max(0.0, level - crest) ** 1.5 * ramp
        assert abs(q - gd.outlet_capacity(level)) <= 1e-12 * q
    assert len(spec.without_weir(0).weirs) == 2
