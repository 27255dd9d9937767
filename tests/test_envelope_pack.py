"""The argument packing of PreissmannBatch.envelope / profile_bands (flowsim_amd/_pack.py: names to masks, threshold shapes, rows of
the envelope, quantile levels) on the CPU, and the new entry points of the C ABI answered without a device: a NULL handle is refused
with a text."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from flowsim_amd import _abi as A
from flowsim_amd import _pack as P


def header_enum(prefix, stop):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flowsim_abi.h")).read(), flags=re.S)
    body = text[text.index("enum { " + prefix):]
    return body[:body.index(stop)]


def test_the_header_and_the_binding_name_the_same_quantities_and_rows():
    bits = dict(re.findall(r"FS_ENV_([A-Z_]+) = (\d+)", header_enum("FS_ENV_DEPTH", "}")))
    assert [bits[n.upper().replace("FROUDE_NUMBER", "FROUDE")] for n in A.ENV_QUANTITIES] == [str(1 << i) for i in range(6)]
    assert int(bits["ALL"]) == A.ENV_ALL == 63 and int(bits["CROSSING"]) == A.ENV_CROSSING == 64
    stats = re.findall(r"FS_ENV_([A-Z_]+)", header_enum("FS_ENV_MAX = 0", "FS_ENV_NSTAT"))
    assert tuple(s.lower() for s in stats) == A.ENV_STATS
    rows = re.findall(r"FS_ENV_CROSS_([A-Z_]+)", header_enum("FS_ENV_CROSS_FIRST = 0", "FS_ENV_NCROSS"))
    assert tuple(s.lower() for s in rows) == A.ENV_CROSS_ROWS


def test_names_to_masks():
    assert P.envelope_mask(("stage",)) == (2, ("stage",))
    assert P.envelope_mask("depth") == (1, ("depth",))
    # the rows come out in bit order, whatever the order of the names
    assert P.envelope_mask(("top_width", "flow", "depth")) == (1 | 4 | 32, ("depth", "flow", "top_width"))
    assert P.envelope_mask(A.ENV_QUANTITIES) == (A.ENV_ALL, A.ENV_QUANTITIES)
    assert [P.envelope_quantity(n) for n in A.ENV_QUANTITIES] == [1, 2, 4, 8, 16, 32]
    with pytest.raises(ValueError, match="unknown envelope quantity 'level'"):
        P.envelope_mask(("stage", "level"))
    with pytest.raises(ValueError, match="given twice"):
        P.envelope_mask(("stage", "stage"))
    with pytest.raises(ValueError, match="no envelope quantity"):
        P.envelope_mask(())


def test_threshold_shapes():
    B, N = 3, 5
    assert P.envelope_threshold(None, B, N) == (None, 0)
    t, per = P.envelope_threshold(2.5, B, N)
    assert per == 0 and t.shape == (N,) and np.all(t == 2.5)
    t, per = P.envelope_threshold([1, 2, 3, 4, np.nan], B, N)
    assert per == 0 and t.dtype == np.float64 and t.flags.c_contiguous and np.isnan(t[4]) and t[3] == 4.0
    full = np.arange(15.0).reshape(B, N)
    t, per = P.envelope_threshold(full[:, ::-1], B, N)
    assert per == 1 and t.shape == (B, N) and t.flags.c_contiguous and np.array_equal(t, full[:, ::-1])
    for bad in (np.zeros(B), np.zeros((N, B)), np.zeros((1, N)), np.zeros((B, N, 1))):
        with pytest.raises(ValueError, match=r"threshold must be a scalar, \[N\] = \[5\] or \[B, N\] = \[3, 5\]"):
            P.envelope_threshold(bad, B, N)


def test_rows_of_the_envelope_on_the_handle():
    held = ("stage", "velocity")
    assert P.envelope_row("stage", "max", held, False) == (2, 0)
    assert P.envelope_row("velocity", "min_level", held, False) == (8, 3)
    assert P.envelope_row("crossing", "count", held, True) == (A.ENV_CROSSING, 2)
    with pytest.raises(ValueError, match="does not hold 'depth'"):
        P.envelope_row("depth", "max", held, True)
    with pytest.raises(ValueError, match="unknown envelope statistic 'mean'"):
        P.envelope_row("stage", "mean", held, True)
    with pytest.raises(ValueError, match="without a threshold"):
        P.envelope_row("crossing", "count", held, False)
    with pytest.raises(ValueError, match="unknown crossing row 'max'"):
        P.envelope_row("crossing", "max", held, True)
    with pytest.raises(ValueError, match="unknown envelope quantity"):
        P.envelope_row("amplitude", "max", held, True)


def test_quantile_levels():
    q = P.quantile_levels((0.05, 0.5, 0.95))
    assert q.dtype == np.float64 and q.tolist() == [0.05, 0.5, 0.95]
    assert P.quantile_levels(()).shape == (0,)
    assert len(P.quantile_levels(np.linspace(0, 1, 16))) == 16
    with pytest.raises(ValueError, match="at most 16"):
        P.quantile_levels(np.linspace(0, 1, 17))
    for bad in ([1.5], [-0.1], [np.nan]):
        with pytest.raises(ValueError, match=r"in \[0, 1\]"):
            P.quantile_levels(bad)


def test_every_new_entry_point_refuses_a_null_handle_with_a_text():
    lib = A.lib()
    out = np.zeros(8)
    cnt = np.zeros(4, dtype=np.int32)
    D, I = out.ctypes.data_as(A._D), cnt.ctypes.data_as(A._I)
    calls = {
        "fs_batch_envelope": lambda: lib.fs_batch_envelope(None, 0, 1, A.ENV_ALL, None, 0, 2, D, None, I),
        "fs_batch_envelope_device": lambda: lib.fs_batch_envelope_device(None, 0, 1, A.ENV_ALL, None, 0, 2),
        "fs_batch_profile_bands": lambda: lib.fs_batch_profile_bands(None, 2, 0, None, 0, D, None, None, I),
    }
    for name, call in calls.items():
        assert name in A.SIGNATURES
        lib.fs_batch_summarize(None, 0, 1, D)                 # (another text in the slot first)
        assert call() < 0, name
        assert "null handle" in A.last_error() and name.replace("_device", "") in A.last_error(), (name, A.last_error())
    lib.fs_batch_summarize(None, 0, 1, D)
    assert lib.fs_batch_envelope_device_ptr(None, 0) is None
    assert "fs_batch_envelope_device_ptr: null handle" in A.last_error()
    assert A.SIGNATURES["fs_batch_envelope_device_ptr"][0] is C.c_void_p
