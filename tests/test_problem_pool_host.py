"""The problem pool of the closed loop (`cfz_problem_check`, `Engine.loop_set_problems`) without a GPU: the library loads without a
device (tests/test_abi.py), the check is host arithmetic; the Python argument handling; the replica construction of
examples/evaluate_strategies.py --dmin."""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import problem_pool_binding as pb  # noqa: E402


@pytest.fixture(scope="module")
def engine():
    import __graft_entry__ as g

    g.build()
    from conflict_rez_amd import engine

    engine.load_library()
    return engine


@pytest.fixture(scope="module")
def spec():
    from conflict_rez_amd import scenarios

    return scenarios.parking_lot_spec()


def test_check_accepts_what_a_problem_may_change(engine, spec):
    """dmin, bounds, weights and every option but carry_duals may differ from the handle's."""
    engine.problem_check(spec, spec)
    for item in pb.problems(spec):
        engine.problem_check(spec, pb.spec_of(item), **pb.options_of(item))
    engine.problem_check(spec, dataclasses.replace(spec, dmin=0.5, weights=np.arange(1.0, 7.0)), max_iter=20, tol=1e-3, mu_init=0.1, restoration=0,
                         vv_rows=0, filter_cap=8)
    # an engine created with other options: the overrides apply to those, as loop_set_problems applies them
    engine.problem_check(spec, spec, dict(carry_duals=0))
    engine.problem_check(spec, dataclasses.replace(spec, dmin=0.2), dict(carry_duals=0, max_iter=40), max_iter=5)
    with pytest.raises(ValueError, match="carry_duals"):
        engine.problem_check(spec, spec, dict(carry_duals=0), carry_duals=1)
    # NULL options on either side: the defaults, and the base's
    lib, cs = engine.load_library(), spec.to_c()
    assert lib.cfz_problem_check(C.byref(cs), None, C.byref(cs), None) == 0
    off = engine.default_options(carry_duals=0)
    assert lib.cfz_problem_check(C.byref(cs), C.byref(off), C.byref(cs), None) == 0  # opt NULL: base_opt, so nothing differs
    assert lib.cfz_problem_check(C.byref(cs), C.byref(off), C.byref(cs), C.byref(engine.default_options())) != 0
    assert b"carry_duals" in lib.cfz_last_error()


def test_check_names_the_field(engine, spec):
    """Every forbidden difference and every invalid value is refused with the field's name."""
    A, b = np.array(spec.A_obs), np.array(spec.b_obs)
    A2 = A.copy(); A2[4, 0] = A2[4, 0][::-1]
    b2 = b.copy(); b2[5, 3] += 1.0
    g2 = np.array(spec.g); g2[2] += 0.05
    rep = dataclasses.replace
    for other, text in ((rep(spec, N=24), "in N"), (rep(spec, A_obs=A[:4], b_obs=b[:4]), "in n_obs"), (rep(spec, n_nbr=2), "in n_nbr"),
                        (rep(spec, rk_substeps=2), "in rk_substeps"), (rep(spec, dt=0.05), "in dt"), (rep(spec, wb=2.4), "in wb"), (rep(spec, g=g2), "in g"),
                        (rep(spec, A_obs=A2), r"in A_obs\[4\]"), (rep(spec, b_obs=b2), r"in b_obs\[5\]"), (rep(spec, N=1), "N out of range"),
                        (rep(spec, n_nbr=-1), "n_obs / n_nbr out of range")):
        with pytest.raises(ValueError, match=text):
            engine.problem_check(spec, other)
    for i, name in enumerate(("x", "y", "v", "delta", "a", "w")):
        bd = np.array(spec.bounds, float)
        bd[2 * i], bd[2 * i + 1] = bd[2 * i + 1], bd[2 * i]
        with pytest.raises(ValueError, match=f"box of {name} has lo > hi"):
            engine.problem_check(spec, rep(spec, bounds=bd))
    bd = np.array(spec.bounds, float); bd[9] = np.inf
    with pytest.raises(ValueError, match="box of a .*not finite"):
        engine.problem_check(spec, rep(spec, bounds=bd))
    for opts, text in ((dict(carry_duals=0), "carry_duals"), (dict(filter_cap=0), "filter_cap"), (dict(filter_cap=33), "filter_cap"),
                       (dict(restoration=-1), "restoration"), (dict(reg_dual_rows=-1.0), "reg_dual_rows"), (dict(resto_first=float("nan")), "resto_first")):
        with pytest.raises(ValueError, match=text):
            engine.problem_check(spec, spec, **opts)
    # an obstacle that is no bounded quadrilateral is invalid on both sides: the difference is named first
    A3 = A.copy(); A3[0, 1] = A3[0, 0]
    with pytest.raises(ValueError, match=r"A_obs\[0\]"):
        engine.problem_check(spec, rep(spec, A_obs=A3))
    with pytest.raises(ValueError, match="bounded quadrilateral"):
        engine.problem_check(rep(spec, A_obs=A3), rep(spec, A_obs=A3))


def test_pack_problems(engine, spec):
    """A spec alone takes the engine's options, a (spec, overrides) pair changes them, None is the empty pool."""
    assert engine.pack_problems(None) == (0, None, None)
    base = dict(max_iter=77, tol=5e-3)
    P, specs, opts = engine.pack_problems([spec, (dataclasses.replace(spec, dmin=0.2), dict(max_iter=5)), (spec, {})], base)
    assert P == 3 and len(specs) == 3 and len(opts) == 3
    assert [o.max_iter for o in opts] == [77, 5, 77] and [o.tol for o in opts] == [5e-3] * 3
    assert [s.dmin for s in specs] == [spec.dmin, 0.2, spec.dmin]
    assert list(specs[1].bounds) == list(spec.bounds) and specs[1].n_obs == spec.n_obs
    dflt = engine.default_options()
    assert opts[1].mu_init == dflt.mu_init and opts[1].carry_duals == dflt.carry_duals
    P, _, opts = engine.pack_problems([spec])
    assert P == 1 and opts[0].max_iter == dflt.max_iter
    with pytest.raises(TypeError, match="unknown solver option"):
        engine.pack_problems([(spec, dict(no_such_option=1))])
    with pytest.raises(TypeError, match=r"problems\[1\]"):
        engine.pack_problems([spec, "B"])
    with pytest.raises(ValueError, match="at least one"):
        engine.pack_problems([])


def test_replicas_of_the_strategy_example():
    """examples/evaluate_strategies.py --dmin: blocks nest noise level, drop rate, clearance; every replica keeps its start's stream id."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from evaluate_strategies import replicate

    S0, V = 6, 4
    k0 = np.arange(10, 10 + S0, dtype=np.int32)
    noise = np.random.default_rng(0).normal(size=(S0, V, 5))
    tof = np.array([0, 0, 1, 1, 2, 2], np.int32)
    levels, rates, dmins = [0.0, 1.0], [0.0, 0.1, 0.3], [0.05, 0.1, 0.2, 0.4]
    r = replicate(k0, noise, tof, levels, rates, dmins)
    L, R, D = len(levels), len(rates), len(dmins)
    S = S0 * L * R * D
    assert all(len(r[k]) == S for k in r)
    i = np.arange(S)
    assert np.array_equal(r["stream"], i % S0) and r["stream"].dtype == np.uint32
    assert np.array_equal(r["k0"], k0[i % S0]) and np.array_equal(r["tof"], tof[i % S0]) and np.array_equal(r["noise"], noise[i % S0])
    assert np.array_equal(r["level"], np.asarray(levels)[(i // S0) % L])
    assert np.array_equal(r["drop"], np.asarray(rates)[(i // (S0 * L)) % R])
    assert np.array_equal(r["problem_of"], i // (S0 * L * R)) and r["problem_of"].dtype == np.int32
    # every (start, level, rate, problem) exactly once
    keys = set(zip(r["stream"].tolist(), r["level"].tolist(), r["drop"].tolist(), r["problem_of"].tolist()))
    assert len(keys) == S
    # an axis that is not given is absent, the others keep their nesting
    r = replicate(k0, noise, tof, None, None, dmins)
    assert r["level"] is None and r["drop"] is None and np.array_equal(r["problem_of"], np.arange(S0 * D) // S0)
    assert np.array_equal(r["stream"], np.arange(S0 * D) % S0)
    r = replicate(k0, noise, tof)
    assert r["problem_of"] is None and np.array_equal(r["k0"], k0) and np.array_equal(r["stream"], np.arange(S0))
