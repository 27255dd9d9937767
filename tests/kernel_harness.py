"""What the kernel tests share: the parity bars and the error norm, the dispatch table (csrc/fs_entry_list.hpp, exported by the C ABI)
with its ids, lookups and capacities, a batch built for one entry, and snapshots of a batch compared bit for bit.  Importing this
module needs neither a GPU nor the built library and does not load it; the table itself (TABLE) and the recipes for its entries
are in tests/entry_recipes.py."""
import numpy as np

from fixture_batch import batch_from_problems
from flowsim_amd import _abi as A

TOL = 1e-8             # fp64 against the oracle
TOL_F32 = 5e-4         # fp32 against the fp64 answer


def rel_err(got, want, floor):
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), floor)))


def kernel_table():
    try:
        return A.kernel_table()
    except Exception:            # library not built: collection must not fail (the gpu run builds first)
        return []


def entry_id(e):
    sec = ("rect", "trap", "table", "irr")[e["section_mode"]]
    return (f"{e['index']:03d}-{'f64' if e['dtype'] == 0 else 'f32'}-{sec}-{e['cells_per_thread']}x{e['waves_per_reach']}"
            f"{'-full' if e['full'] else ''}-bc{e['boundary_class']}{'' if e['diag'] else '-nodiag'}{'-long' if e.get('long_reach') else ''}"
            f"{'-tail%d' % e['tail'] if e.get('tail', -1) >= 0 else ''}{'-team' if e.get('team') else ''}")


def find_entry(**attrs):
    """the first dispatch-table entry with these attributes (an attribute an entry does not carry counts as 0; tail: as -1)"""
    def value(e, key):
        return e.get("tail", -1) if key == "tail" else int(e.get(key) or 0)
    for e in kernel_table():
        if all(value(e, key) == want for key, want in attrs.items()):
            return e
    raise KeyError(attrs)


def f32_of(e):
    return e["dtype"] == A.F32


def entry_of(b):
    """the dispatch-table entry the batch's last launch ran"""
    return A.kernel_table()[b.kernel_index()]


def capacity(e, one_grid=False):
    """rows of the scalar system (N - 1 cells + the boundary row) that fit one lane grid of the entry, 64 M W; a multi-pass or team
    entry takes up to 64 / W grids of them (one_grid: the single grid of such an entry too)"""
    cap = 64 * e["cells_per_thread"] * e["waves_per_reach"]
    return cap * (64 // e["waves_per_reach"]) if (e.get("long_reach") or e.get("team")) and not one_grid else cap


def batch_for_entry(probs, e, mode, override=None, **kw):
    """fixture_batch.batch_from_problems with the entry's dtype; history: the entry's diag flag unless given"""
    kw.setdefault("history", bool(e["diag"]))
    return batch_from_problems(probs, mode=mode, dtype="f32" if f32_of(e) else "f64", n_main_override=override, **kw)


FIELDS = ("status", "iters", "hyd", "state", "hist")


def snapshot(b, nt, upto=None, fields=FIELDS):
    """the named fields of what a caller can read, as one dict; "hist" only where the batch keeps a history, and its rows only up to
    level `upto` (rows never written hold no promise)"""
    read = dict(status=lambda: b.status().copy(), iters=lambda: b.iterations(0, nt), hyd=lambda: b.hydrographs(0, nt), state=b.state, guess=b.guess,
                hist=lambda: tuple(a[:nt if upto is None else upto + 1] for a in b.history_arrays(0, nt)))
    return {k: read[k]() for k in fields if k != "hist" or b.history}


def assert_same_bits(a, b, fields=None, what=""):
    """bit for bit, NaN equal to NaN, on `fields` (None: those of a); a field neither snapshot holds is passed over"""
    for k in a if fields is None else fields:
        if k in a or k in b:
            x, y = (a[k], b[k]) if isinstance(a[k], tuple) else ((a[k],), (b[k],))
            assert all(np.array_equal(u, v, equal_nan=True) for u, v in zip(x, y)), (what, k)
