"""The helpers of tests/kernel_harness.py that the kernel tests rest on, on the CPU, without the library: the error norm's floor, what
"the same bits" covers, the capacity of an entry and the ids the parametrised tests are collected under."""
import numpy as np
import pytest

import kernel_harness as H


def test_rel_err_applies_the_floor_and_takes_the_maximum():
    want = np.array([0.0, 1e-6, 2.0])
    got = want + np.array([2e-4, 5e-4, 1e-3])
    assert H.rel_err(got, want, 1e-3) == pytest.approx(0.5, rel=1e-9)            # 5e-4 / floor; the others: 0.2 and 5e-4
    assert H.rel_err(got[:1], want[:1], 1e-3) == pytest.approx(0.2, rel=1e-9)    # a want of 0 is measured against the floor
    assert H.rel_err(got[2:], want[2:], 1e-3) == pytest.approx(5e-4, rel=1e-9)   # above the floor: relative
    assert H.rel_err(want, want, 1e-3) == 0.0


def _snap():
    return dict(status=np.array([0, 2]), hyd=np.array([[1.0, np.nan], [3.0, 4.0]]), state=(np.array([1.0, np.nan]), np.array([5.0, 6.0])))


def test_same_bits_passes_with_nans_in_equal_places():
    H.assert_same_bits(_snap(), _snap())
    H.assert_same_bits(_snap(), _snap(), fields=("status", "hyd", "state", "hist"))      # hist: in neither, passed over


@pytest.mark.parametrize("field,edit", [("hyd", lambda s: s["hyd"].__setitem__((1, 0), np.nextafter(3.0, 4.0))),      # one ulp
                                        ("hyd", lambda s: s["hyd"].__setitem__((0, 1), 7.0)),                         # NaN against a number
                                        ("state", lambda s: s["state"][1].__setitem__(0, 5.5))],                      # an element of a tuple
                         ids=["one-ulp", "nan-against-a-number", "tuple-element"])
def test_same_bits_fails_on_a_difference_and_looks_only_where_asked(field, edit):
    a, b = _snap(), _snap()
    edit(b)
    for x, y in ((a, b), (b, a)):
        with pytest.raises(AssertionError):
            H.assert_same_bits(x, y)
        with pytest.raises(AssertionError):
            H.assert_same_bits(x, y, fields=(field,))
        H.assert_same_bits(x, y, fields=tuple(k for k in a if k != field))


def test_capacity():
    e = dict(cells_per_thread=16, waves_per_reach=4)
    assert H.capacity(e) == 4096 and H.capacity(dict(e, long_reach=0, team=0)) == 4096
    assert H.capacity(dict(e, long_reach=1)) == H.capacity(dict(e, team=1)) == 16 * 4096
    assert H.capacity(dict(cells_per_thread=8, waves_per_reach=4, long_reach=1)) == 16 * 2048
    assert H.capacity(dict(e, team=1), one_grid=True) == 4096


def test_entry_ids_are_the_collected_ones():
    e = dict(index=0, dtype=0, section_mode=0, cells_per_thread=2, waves_per_reach=1, full=0, boundary_class=0, diag=1, long_reach=0, tail=-1, team=0)
    assert H.entry_id(e) == "000-f64-rect-2x1-bc0"
    assert H.entry_id(dict(e, index=107, dtype=1, section_mode=2, cells_per_thread=4, waves_per_reach=4, boundary_class=-1, long_reach=1)) == "107-f32-table-4x4-bc-1-long"
    assert H.entry_id(dict(e, index=109, section_mode=2, boundary_class=8, diag=0, tail=1)) == "109-f64-table-2x1-bc8-nodiag-tail1"
    assert H.entry_id(dict(e, index=114, cells_per_thread=16, waves_per_reach=4, full=1, boundary_class=5, diag=0, team=1)) == "114-f64-rect-16x4-full-bc5-nodiag-team"
    assert H.entry_id(dict(e, index=100, section_mode=3, boundary_class=5, diag=0)) == "100-f64-irr-2x1-bc5-nodiag"
