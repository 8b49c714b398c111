"""The host arithmetic of the planning entry points, without a GPU: `cfz_colloc_band_info` and `cfz_colloc_elimination_info` against
what the build before their restatement answered (tests/golden/planning_info_parent.json, recorded by
tests/golden/make_planning_info.py: shapes, pair lists and both eliminations, refused calls with their text), the band info as the
elimination info of the band elimination, the refusal texts of single defects, and the binding's one option helper."""
import json
import os

import pytest

from conflict_rez_amd import engine

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(HERE, "golden", "planning_info_parent.json")) as f:
        d = json.load(f)
    assert d["N_per_set"] == 5 and len(d["cases"]) > 300
    return d["cases"]


def _answer(f, case, **kw):
    try:
        r = f(case["n_sets"], n_obs=case["n_obs"], pairs=case["pairs"], has_final=case["has_final"], **kw)
    except RuntimeError as e:
        return {"error": str(e)}
    return list(r) if isinstance(r, tuple) else r


def test_info_functions_answer_what_the_parent_build_answered(recorded):
    """Every field of every case, as integers; a call the parent refused is refused with the same text."""
    grid = {(len(c["n_sets"]), max(c["n_sets"]), c["n_obs"], c["has_final"] is None, None if c["pairs"] is None else len(c["pairs"])) for c in recorded}
    assert {g[0] for g in grid} == {1, 2, 3, 4} and {g[1] for g in grid} >= {2, 3, 11, 52, 53} and {g[2] for g in grid} == {0, 4, 6, 8}
    assert {g[3] for g in grid} == {True, False} and {g[4] for g in grid} == {None, 0, 1}
    for c in recorded:
        key = {k: c[k] for k in ("n_sets", "has_final", "n_obs", "pairs")}
        assert _answer(engine.colloc_band_info, c) == c["band"], key
        for s in (0, 1):
            got = _answer(engine.colloc_elimination_info, c, structured=s)
            assert got == c["elim"][s], (key, s)
            assert "error" in got or all(type(v) is int for v in got.values())


def test_band_info_is_the_elimination_info_of_the_band_elimination(recorded):
    answered = 0
    for c in recorded:
        b, e = _answer(engine.colloc_band_info, c), _answer(engine.colloc_elimination_info, c, structured=0)
        if "error" in e:
            assert b == {"error": e["error"].replace("cfz_colloc_elimination_info", "cfz_colloc_band_info")}
        else:
            assert tuple(b) == (e["nk"], e["kb"], e["band_bytes"]), c
            answered += 1
    assert answered > 300


REFUSALS = [
    (dict(n_sets=[1]), "a plan needs at least two strategy steps"),
    (dict(n_sets=[3, 3], pairs=[(1, 0)]), "bad vehicle pair"),
    (dict(n_sets=[3], pairs=[(0, 1)]), "vehicle pairs need at least two vehicles"),
    (dict(n_sets=[3] * 5), "bad argument"),
    (dict(n_sets=[3], n_obs=9), "bad argument"),
    (dict(n_sets=[3], structured=2), "structured"),
    (dict(n_sets=[3] * 4, pairs=[(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3), (0, 1)]), "compiled limits"),
]


@pytest.mark.parametrize("kw,text", REFUSALS, ids=[t for _, t in REFUSALS])
def test_single_defects_are_refused_with_their_text(kw, text):
    with pytest.raises(RuntimeError, match=text):
        engine.colloc_elimination_info(**kw)
    if "structured" not in kw:
        with pytest.raises(RuntimeError, match=text):
            engine.colloc_band_info(**kw)


@pytest.mark.parametrize("struct,default_fn,what", [(engine._CPlanOptions, "cfz_default_plan_options", "plan"),
                                                    (engine._CCollocOptions, "cfz_default_colloc_options", "collocation"),
                                                    (engine._COptions, "cfz_default_options", "solver")])
def test_options_refuses_unknown_names(struct, default_fn, what):
    with pytest.raises(TypeError, match=f"unknown {what} option 'max_itr'"):
        engine._options(struct, default_fn, what, dict(max_itr=3))
    o = engine._options(struct, default_fn, what, dict(max_iter=7))
    assert isinstance(o, struct) and o.max_iter == 7


def test_options_assigns_arrays_element_wise():
    bounds = [float(i) - 3.5 for i in range(12)]
    o = engine._options(engine._CPlanOptions, "cfz_default_plan_options", "plan", dict(bounds=tuple(bounds), N=12))
    assert list(o.bounds) == bounds and o.N == 12 and o.dt == 0.1
