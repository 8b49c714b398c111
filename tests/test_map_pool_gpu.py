"""Per-scenario obstacle maps of the closed loop (`cfz_map_check`, `cfz_loop_set_maps`, `cfz_audit_maps`) on the GPU, through the C ABI.

With a pool of M maps and map_of[S], every solve of scenario s stands on the obstacles of map map_of[s] (rows, working set, stage-0
feasibility test, restoration) and the audit measures the scenario against that map; the setting composes with the problem pool.

The four test maps (tests/map_pool_binding.py) over the `parking_lot_spec()` handle, planned table, V = 4:
  A the handle's own | B every face moved out by 0.10 m | C by 0.20 m | D every obstacle shifted by (0.15, -0.15) m
tests/test_map_pool_host.py asserts from the host replay that the map moves the outcome of every scenario of the batch of
test_against_the_host_replay and that every map has converged solves there.  A plain engine created on a map
(`scenarios.map_spec`) is the parent's code path for that map: the mixed batch must equal it bit for bit.

What every per-scenario pool has is tests/loop_cases.py's, written against `POOL`; here: the numbered statement, that call, what is special.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audit_binding as ab  # noqa: E402
import disturbance_binding as db  # noqa: E402
import map_pool_binding as mb  # noqa: E402
import problem_pool_binding as pb  # noqa: E402
import loop_cases as lc  # noqa: E402
from loop_cases import orders as _orders, planned as _planned, run as _run, same as _same  # noqa: E402

SIG = db.SIGMA
SEED = 2024
S16, K6 = 16, 6
TOL = dict(pos_tol=0.3, psi_tol=0.1, v_tol=0.1)


def _plain(spec, m, max_batch):
    from conflict_rez_amd import engine, scenarios

    return engine.Engine(scenarios.map_spec(spec, *m), max_batch=max_batch)


POOL = lc.Pool(set=lambda e, maps, map_of: e.loop_set_maps(maps, map_of), off=lambda e: e.loop_set_maps(None), own=lambda e: e.spec,
               entries=mb.maps, plain=_plain, names=mb.NAMES)


@pytest.fixture(scope="module")
def eng():
    import __graft_entry__ as g

    g.build()
    from conflict_rez_amd import engine, scenarios

    e = engine.Engine(scenarios.parking_lot_spec(), max_batch=S16 * 4)
    yield e
    e.close()


@pytest.fixture(scope="module")
def maps(eng):
    return mb.maps(eng.spec)


@pytest.fixture(scope="module")
def plain_engines(eng, maps):
    """One plain engine per map, created with the handle's spec on that map: the parent's code path."""
    es = [POOL.plain(eng.spec, m, S16 * 4) for m in maps]
    yield es
    for e in es:
        e.close()


@pytest.mark.parametrize("exchange", ["jacobi", "sequential"])
@pytest.mark.parametrize("how", ["step", "run"])
def test_off_is_off(eng, how, exchange):
    """1. No call, M = 1 with the handle's own map, M = 3 identical copies under a random map_of, and set-then-unset give equal state,
    prediction, status, iterations and record, bit for bit.  S = 16, K = 6."""
    S, K, V = S16, K6, eng.spec.n_nbr + 1
    init = _planned(eng, S)
    order = _orders(S, V, 11) if exchange == "sequential" else None
    plain = lc.off_is_off(POOL, eng, init, K, how, order)
    assert (plain["rec_status"] == 0).mean() > 0.5
    _same(plain, _run(eng, init, K, how, order, lambda e: e.loop_set_maps([])), "an empty pool is off")


@pytest.mark.parametrize("exchange", ["jacobi", "sequential"])
@pytest.mark.parametrize("how", ["step", "run"])
def test_off_is_off_under_a_lossy_exchange(eng, how, exchange):
    """1, with loop_set_comm(p_drop 0.3) and no disturbance.  As under a problem pool, the pool kernels clip the applied input only while a
    disturbance is set and the persistent comm kernels without a pool clip to the handle's box under their zero sigma: the handle's own
    map equals no map pool as long as every applied input lies inside that box, which holds on the planned table
    (tests/test_problem_pool_gpu.py::test_off_is_off_under_a_lossy_exchange)."""
    S, K, V = S16, K6, eng.spec.n_nbr + 1
    init = _planned(eng, S)
    order = _orders(S, V, 11) if exchange == "sequential" else None
    plain = lc.off_is_off(POOL, eng, init, K, how, order, under=lambda e: e.loop_set_comm(SEED + 1, 0.3, max_age=3, compensate=True))
    assert not np.array_equal(plain["state"], _run(eng, init, K, how, order)["state"])  # the loss is felt


@pytest.mark.parametrize("disturbed", [False, True], ids=["exact", "noise+loss"])
@pytest.mark.parametrize("exchange", ["jacobi", "sequential"])
def test_mixed_batch_equals_separate_handles(eng, maps, plain_engines, exchange, disturbed):
    """2. S = 16, map_of[s] = s % 4, K = 6, stepped, in one launch and in a split launch: the rows of map m equal, bit for bit, what a plain
    engine created on map m gives for m's four scenarios alone; once more under noise and a lossy exchange (p_drop 0.3) with the
    sub-batch on the stream ids of its rows.  The rows of D differ from what the plain engine on map A gives for the same scenarios."""
    S, K, V = S16, K6, eng.spec.n_nbr + 1
    table, k0, noise = _planned(eng, S)
    order = _orders(S, V, 11) if exchange == "sequential" else None
    settings = lambda stream: lc.noise_and_loss(SIG, stream, SEED) if disturbed else None
    sel = np.flatnonzero(np.arange(S) % 4 == 3)
    for how, mixed in lc.mixed_batch_equals_separate_handles(POOL, eng, maps, plain_engines, (table, k0, noise), K, order, settings).items():
        on_a = _run(plain_engines[0], (table, k0[sel], noise[sel]), K, how, None if order is None else order[sel], settings(sel))
        assert not np.array_equal(mixed["state"][sel], on_a["state"]), (how, "the D rows equal the A engine's")


@pytest.mark.parametrize("exchange", ["jacobi", "sequential"])
def test_against_the_host_replay(eng, ospec, maps, exchange):
    """3. S = 8, two scenarios per map (map_of[s] = s % 4), K = 8: the port replayed with every scenario's own obstacles in its MpcSpec
    gives equal status and iterations solve for solve and states within 1e-6 (the tolerance of
    test_problem_pool_gpu.py::test_against_the_host_replay and test_disturbance_gpu.py::test_against_the_host_replay); at least one solve
    on map C ends with status 4 (the measured state inside the grown obstacles' clearance)."""
    from oracle.closed_loop import replay

    S, K, V = 8, 8, eng.spec.n_nbr + 1
    table, k0, noise = _planned(eng, S)
    mof = np.arange(S) % 4
    order = _orders(S, V, 5) if exchange == "sequential" else None
    eng.loop_init(table, k0, noise)
    if order is not None:
        eng.loop_set_order(order)
    eng.loop_set_maps(maps, mof)
    got = lc.stepwise(eng, K)
    osp = [mb.oracle_spec(ospec, maps[m]) for m in mof]
    worst, _ = lc.against_replay(got, replay(osp, table, k0, noise, K, dt=eng.spec.dt, wb=eng.spec.wb, order=order))
    status = np.stack([g["status"] for g in got])
    conv = {mb.NAMES[m]: int((status[:, mof == m] == 0).sum()) for m in range(4)}
    print(f"{exchange}: max |state - replay| {worst:.2e}; converged solves of 64 per map {conv}; "
          f"map C: {int((status[:, mof == 2] == 4).sum())} solves with status 4")
    assert worst < 1e-6
    assert (status[:, mof == 2] == 4).any()


def test_maps_and_problems_together(eng, maps):
    """4. problem_of[s] = s % 4 (the four problems of tests/problem_pool_binding.py) and map_of[s] = (s // 4) % 4 on S = 16, K = 6, one
    launch: the two call orders of the setters are equal bit for bit; every (problem, map) pair, one scenario each, equals a plain
    engine created with that problem's constants on that map; unsetting one setting leaves the other in force."""
    from conflict_rez_amd import engine, scenarios

    S, K = S16, K6
    table, k0, noise = _planned(eng, S)
    probs = pb.problems(eng.spec)
    pof, mof = np.arange(S) % 4, (np.arange(S) // 4) % 4

    def maps_first(e):
        e.loop_set_maps(maps, mof)
        e.loop_set_problems(probs, pof)

    def problems_first(e):
        e.loop_set_problems(probs, pof)
        e.loop_set_maps(maps, mof)

    both = _run(eng, (table, k0, noise), K, "run", None, maps_first)
    _same(both, _run(eng, (table, k0, noise), K, "run", None, problems_first), "the two call orders")
    _same(both, _run(eng, (table, k0, noise), K, "step", None, problems_first), "stepped")
    for s in range(S):
        p, m = probs[pof[s]], maps[mof[s]]
        pe = engine.Engine(scenarios.map_spec(pb.spec_of(p), *m), max_batch=4, **pb.options_of(p))
        alone = _run(pe, (table, k0[s : s + 1], noise[s : s + 1]), K, "run")
        pe.close()
        _same(lc.rows(both, [s]), alone, (pb.NAMES[pof[s]], mb.NAMES[mof[s]]))
    only_maps = _run(eng, (table, k0, noise), K, "run", None, lambda e: e.loop_set_maps(maps, mof))
    only_probs = _run(eng, (table, k0, noise), K, "run", None, lambda e: e.loop_set_problems(probs, pof))
    assert not np.array_equal(only_maps["state"], both["state"]) and not np.array_equal(only_probs["state"], both["state"])

    def then(first, unset):
        def f(e):
            first(e)
            unset(e)
        return f

    for first in (maps_first, problems_first):
        _same(only_maps, _run(eng, (table, k0, noise), K, "run", None, then(first, lambda e: e.loop_set_problems(None))), "problems unset: the maps stay")
        _same(only_probs, _run(eng, (table, k0, noise), K, "run", None, then(first, lambda e: e.loop_set_maps(None))), "maps unset: the problems stay")


@pytest.mark.parametrize("exchange", ["jacobi", "sequential"])
def test_mapping_changes_between_calls(eng, maps, exchange):
    """5. loop_run(3), another map_of, loop_run(3) equals the same sequence stepped, bit for bit; the change matters."""
    S, K, V = S16, K6, eng.spec.n_nbr + 1
    order = _orders(S, V, 11) if exchange == "sequential" else None
    lc.mapping_changes_between_calls(POOL, eng, maps, _planned(eng, S), K, order)


def test_audit_follows_the_map(eng, maps, plain_engines):
    """6. S = 16, map_of[s] = s % 4, K = 6 in one launch.  loop_audit() equals, row for row and bit for bit, the audits of the four plain
    engines of the same record, and Engine.audit(history, goal, maps, map_of).  Both agree with the CPU build of the kernel's source
    (audit_binding.emu_audit, called per scenario with that scenario's obstacle vertices) as tests/test_audit_geometry.py asserts the
    emulation against the numpy statement: where, first_contact and arrive equal, clear within 1e-12.  The vehicle-vehicle column does
    not depend on the map; the vehicle-obstacle column does."""
    S, K = S16, K6
    table, k0, noise = _planned(eng, S)
    mof = np.arange(S) % 4
    _run(eng, (table, k0, noise), K, "run", None, lambda e: e.loop_set_maps(maps, mof))
    traj = eng.loop_history()["traj"]
    goals = lc.goals(table, S)
    a = eng.loop_audit(**TOL)
    assert np.isfinite(a["clear"]).all()
    _same(a, eng.audit(traj, goals, maps, mof, **TOL), "loop_audit against audit of the history on the same maps")
    for m, pe in enumerate(plain_engines):
        sel = np.flatnonzero(mof == m)
        _same(lc.rows(a, sel), pe.audit(traj[:, sel], goals[sel], **TOL), ("the plain engine on map", mb.NAMES[m]))
    for s in range(S):
        emu = ab.emu_audit(traj[:, s : s + 1], goals[s : s + 1], mb.vertices(*maps[mof[s]]), eng.spec.g, TOL["pos_tol"], TOL["psi_tol"], TOL["v_tol"])
        for k in ("where", "first_contact", "arrive"):
            assert np.array_equal(a[k][s], emu[k][0]), (s, k, a[k][s], emu[k][0])
        assert np.abs(a["clear"][s] - emu["clear"][0]).max() <= 1e-12, s
    on_a = eng.audit(traj, goals, **TOL)  # the same record against the handle's map
    assert np.array_equal(on_a["clear"][:, 0], a["clear"][:, 0]) and np.array_equal(on_a["where"][:, :3], a["where"][:, :3])
    assert np.array_equal(on_a["arrive"], a["arrive"])
    assert np.array_equal(on_a["clear"][mof == 0, 1], a["clear"][mof == 0, 1])
    assert (on_a["clear"][mof > 0, 1] != a["clear"][mof > 0, 1]).all()
    # the mapping in force when the audit is called
    eng.loop_set_maps(maps, np.zeros(S, int))
    _same(on_a, eng.loop_audit(**TOL), "after the mapping changed to map A")
    eng.loop_set_maps(None)
    _same(on_a, eng.loop_audit(**TOL), "after the maps were switched off")


def test_refusals(eng, maps):
    """7. Refused by the host before any launch, with a cfz_last_error text, the loop's state and the setting in force unchanged (the next
    steps give the bits they would have given): a call before loop_init, M < 0, map_of out of range, a map with an unbounded obstacle or
    a NaN; the same for cfz_audit_maps.  loop_init switches the maps off."""
    import ctypes as C

    from conflict_rez_amd import engine

    S, K = S16, 4
    init = _planned(eng, S)
    mof = np.arange(S) % 4
    fresh = engine.Engine(eng.spec, max_batch=4)
    with pytest.raises(RuntimeError, match="cfz_loop_init has not been called"):
        fresh.loop_set_maps(maps, np.zeros(1, int))
    fresh.close()
    A, b = engine.pack_maps(eng.spec, maps)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)

    def refused(eng):
        assert eng.lib.cfz_loop_set_maps(eng._h, -1, ptr(A), ptr(b), ptr(mof.astype(np.int32))) != 0
        assert b"M must not be negative" in eng.lib.cfz_last_error()
        for bad in (np.where(mof == 3, 4, mof), np.where(mof == 0, -1, mof)):
            with pytest.raises(RuntimeError, match="map_of"):
                eng.loop_set_maps(maps, bad)
        strip_A, strip_b = np.array(maps[1][0]), np.array(maps[1][1])
        strip_A[2, 1:], strip_b[2, 1:] = strip_A[2, 0], strip_b[2, 0]  # obstacle 2: one row four times, a half-plane
        nan_b = np.array(maps[2][1]); nan_b[5, 3] = np.nan
        for pool, text in (([maps[0], (strip_A, strip_b)], "map 1: obstacle 2 is not a bounded quadrilateral"),
                           ([maps[0], maps[1], (maps[2][0], nan_b)], "map 2: obstacle 5 has an entry that is not finite")):
            with pytest.raises(RuntimeError, match=text):
                eng.loop_set_maps(pool, np.zeros(S, int))
            with pytest.raises(RuntimeError, match=text):
                eng.audit(np.zeros((2, S, 4, 7)), np.zeros((S, 4, 3)), pool, np.zeros(S, int))
        with pytest.raises(RuntimeError, match="map_of"):
            eng.audit(np.zeros((2, S, 4, 7)), np.zeros((S, 4, 3)), maps, np.where(mof == 3, 4, mof))

    lc.refusals_change_nothing(POOL, eng, maps, init, K, refused, rest=("step", K - 3))
