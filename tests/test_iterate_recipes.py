"""The iterate recipes of tests/iterate_recipes.py, checked on the numpy oracle alone, for every dispatch-table entry: the
capped levels end where and how they are meant to, from states that are positive and subcritical; the first update moves (nearly)
every node; the first iterate is sensitive to each Jacobian ingredient by at least 50 times the parity bar - so a kernel whose
T, dSe/dA, dSe/dQ or boundary-row derivative is off by 1e-4 cannot pass tests/test_gpu_newton_iterates.py - and the reference
itself is stable to rounding by a factor 1e4 below that bar.  These are conditions on the recipes, not measurements of a kernel."""
import numpy as np
import pytest

import iterate_recipes as IR
from oracle import preissmann_oracle as O

TABLE = IR.TABLE
IDS = [IR.entry_id(e) for e in TABLE]
BAR = 1e-8                 # the fp64 parity bar of the suite
EPS = 1e-4                 # the relative error of a Jacobian ingredient that must show
SENSITIVITY = 50 * BAR     # ... by at least this much in x1
STABILITY = BAR / 1e4      # what rounding noise on R and the Jacobian may move x1 by
NOISE = 4 * 2.0 ** -52
DRAWS = 8
FROUDE_MAX = 0.9


def moved(a, b):
    """the suite's error measure (depth floor 1e-3, flow floor 1.0) between two Newton vectors"""
    return max(IR.rel_err(a[0::2], b[0::2], 1e-3), IR.rel_err(a[1::2], b[1::2], 1.0))


def first_iterate(p):
    ref = O.newton_run(p, n_steps=1, max_iter_at={1: 1})
    assert ref["status"] == 1
    return ref["x_next"]


def froude(p, h, Q):
    t = O.node_terms(p.geo, h, Q)
    return float(np.max(np.abs(O.froude(t["top_width"], t["A"], Q))))


def test_the_library_is_built_and_every_entry_has_a_recipe():
    assert len(TABLE) > 100, "the dispatch table comes from the built library"
    for e in TABLE:
        probs, mode, _ = IR.iterate_case(e)
        assert len(probs) == IR.B and all(p.N == probs[0].N for p in probs)
        assert all(p.nt == 3 and p.tol == IR.ITER_TOL for p in probs)
        assert not np.array_equal(probs[0].h0, probs[1].h0) and not np.array_equal(probs[1].Q0, probs[2].Q0)
        for k in O.GEO_KEYS:        # one channel: a TABLE batch shares its geometry
            assert all(np.array_equal(p.geo[k], probs[0].geo[k]) for p in probs)


def test_the_offsets_reach_both_sides_of_bankfull_and_of_polyline_vertices():
    """compound fixtures: every one has nodes over bank at x0, and one of them (gerd) nodes on both sides of bankfull and nodes that
    change sides between the reaches of one launch or between x0 and x1; polyline fixtures: in every one the water levels of a node
    (three starts and their first iterates) straddle a vertex of its section"""
    compound, polyline = {}, {}
    for e in TABLE:
        probs, _, _ = IR.iterate_case(e)
        g = probs[0].geo
        firsts = [IR.unknowns(r[(1, 1)])[0] for r in IR.references(e)]
        levels = np.array([p.h0 for p in probs] + firsts)
        key = (probs[0].N, float(g["z_bed"][0]), probs[0].ds.kind)
        if "irr_npts" in g:
            straddled = 0
            for i in np.nonzero(g["irr_npts"] > 0)[0]:
                z = g["irr_z"][i, :int(g["irr_npts"][i])]
                lo, hi = z.min() + levels[:, i].min(), z.min() + levels[:, i].max()
                straddled += int(np.any((z > lo) & (z < hi)))
            polyline[key] = polyline.get(key, 0) + straddled
            continue
        comp = g["is_compound"] > 0.5
        if np.any(comp):
            over = (levels > g["h_bf"]) & comp
            compound.setdefault(key, []).append((bool(np.any(over[:IR.B])), bool(np.any(comp & ~over[:IR.B])), bool(np.any(over != over[0]))))
    print("compound (over bank, in bank, changes sides):", compound, " polyline nodes straddling a vertex:", polyline)
    assert len(compound) >= 2 and all(all(c[0] for c in v) for v in compound.values())
    assert any(all(c[1] and c[2] for c in v) for v in compound.values())
    assert len(polyline) >= 4 and all(v > 0 for v in polyline.values())


@pytest.mark.parametrize("e", TABLE, ids=IDS)
def test_exit_state_and_movement(e):
    probs, _, _ = IR.iterate_case(e)
    for r, (p, refs) in enumerate(zip(probs, IR.references(e))):
        vectors = [(p.h0, p.Q0)]
        for (lvl, m), ref in refs.items():
            assert ref["status"] == 1 and ref["fail_level"] == lvl and ref["iters"][lvl] == m, (r, lvl, m, ref["status"], ref["iters"])
            assert np.all(ref["iters"][1:lvl] > 0) and np.all(np.isfinite(ref["x_next"]))
            vectors.append(IR.unknowns(ref))
        lvl2 = refs[(2, 1)]
        vectors.append((lvl2["depth"][2], lvl2["flow"][2]))           # the start vector of level 2
        vectors.append((lvl2["depth"][1], lvl2["flow"][1]))           # and its old state
        assert not np.array_equal(lvl2["depth"][2], lvl2["depth"][1])         # (the time differences of level 2 are not degenerate)
        fr = max(froude(p, h, Q) for h, Q in vectors)
        hmin = min(float(np.min(h)) for h, _ in vectors)
        h1 = IR.unknowns(refs[(1, 1)])[0]
        frac = float(np.mean(np.abs(h1 - p.h0) / p.h0 > 1e-4))
        print(f"{IR.entry_id(e)} reach {r}: min depth {hmin:.3f}, max Froude {fr:.3f}, nodes moved by the first update {100 * frac:.2f} %, "
              f"level-1 counts ahead of the level-2 iterate {lvl2['iters'][1]}")
        assert hmin > 0 and fr < FROUDE_MAX
        assert frac >= 0.99


def _scaled_terms(key):
    plain = O.node_terms

    def terms(geo, h, Q):
        out = plain(geo, h, Q)
        out[key] = out[key] * (1 + EPS)
        return out
    return terms


def _scaled_row(side, slot):
    plain = O.boundary_eval

    def row(bc, geo_node, h, Q, k, dt, Q_old=None, store=None):
        out = list(plain(bc, geo_node, h, Q, k, dt, Q_old=Q_old, store=store))
        if (Q_old is not None) == (side == "ds"):          # (assemble hands Q_old to the downstream row only)
            out[slot] = out[slot] * (1 + EPS)
        return tuple(out)
    return row


@pytest.mark.parametrize("e", TABLE, ids=IDS)
def test_the_first_iterate_sees_every_jacobian_ingredient(e, monkeypatch):
    probs, _, _ = IR.iterate_case(e)
    for r, p in enumerate(probs):
        clean = first_iterate(p)
        for key in ("T", "dSe_dA", "dSe_dQ"):
            with monkeypatch.context() as m:
                m.setattr(O, "node_terms", _scaled_terms(key))
                got = moved(first_iterate(p), clean)
            print(f"{IR.entry_id(e)} reach {r}: {key} (1 + {EPS:g}) moves x1 by {got:.2e}")
            assert got >= SENSITIVITY, (key, got)
        rows = {"us": O.boundary_eval(p.us, O._one(p.geo, 0), p.h0[0], p.Q0[0], 1, p.dt),
                "ds": O.boundary_eval(p.ds, O._one(p.geo, p.N - 1), p.h0[-1], p.Q0[-1], 1, p.dt, Q_old=p.Q0[-1], store={"Y_prev": None})}
        for side, row in rows.items():
            for slot, name in ((1, "df/dh"), (2, "df/dQ")):
                if row[slot] == 0.0:                       # the kind has no such derivative
                    continue
                with monkeypatch.context() as m:
                    m.setattr(O, "boundary_eval", _scaled_row(side, slot))
                    got = moved(first_iterate(p), clean)
                print(f"{IR.entry_id(e)} reach {r}: {side} {getattr(p, side).kind} {name} (1 + {EPS:g}) moves x1 by {got:.2e}")
                assert got >= SENSITIVITY, (side, name, got)


@pytest.mark.parametrize("e", TABLE, ids=IDS)
def test_the_reference_iterate_is_stable_to_rounding(e, monkeypatch):
    probs, _, _ = IR.iterate_case(e)
    plain = O.assemble
    rng = np.random.default_rng(e["index"])

    def noisy(*args, **kw):
        R, data, new = plain(*args, **kw)
        return (R * (1 + NOISE * rng.uniform(-1, 1, R.shape)), data * (1 + NOISE * rng.uniform(-1, 1, data.shape)), new)
    for r, p in enumerate(probs):
        clean = first_iterate(p)
        with monkeypatch.context() as m:
            m.setattr(O, "assemble", noisy)
            worst = max(moved(first_iterate(p), clean) for _ in range(DRAWS))
        print(f"{IR.entry_id(e)} reach {r}: noise of {NOISE:.1e} on R and the Jacobian moves x1 by {worst:.2e}")
        assert worst < STABILITY, worst
