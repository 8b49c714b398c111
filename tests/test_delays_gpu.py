"""The delay search over a conflict map on the GPU (cfz_delay_search / cfz_plan_delays / cfz_loop_plan_delays, delay_kernel over
csrc/cfz_delay.inl): every integer equal to the CPU build of the same source and to the numpy statement, the clearance the same double, the
same arrays on every call, the map searched where it was computed equal to the map searched after a round trip, the answers measured
again as delayed tables, and without effect on the closed loop.  No solver kernel runs but in the one test about the loop."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conflict_binding as cb  # noqa: E402
import delay_binding as db  # noqa: E402

ALL = db.OUT + ("clear",)


@pytest.fixture(scope="module")
def eng():
    import __graft_entry__ as g

    g.build()
    from conflict_rez_amd import engine, scenarios

    e = engine.Engine(scenarios.parking_lot_spec(), max_batch=1024)
    yield e
    e.close()


def _equal(a, b):
    """All five outputs, the clearance as bits (NaN where it is not written on either side)."""
    for k in ALL:
        assert np.array_equal(a[k], b[k], equal_nan=k == "clear"), (k, a[k].tolist(), b[k].tolist())
    return True


@pytest.mark.parametrize("name", list(db.CASES))
def test_delay_search_cases(eng, name):
    """The cases of the host tests on the device (V from 1 to 8 on the 4-vehicle engine): D = 0, rows of one and of several words, shells
    below one round of the lanes and of many rounds, a cap of 0, 28 pairs."""
    count, clear, slack, cap, ref = db.case(name)
    out = eng.delay_search(dict(count=count, clear=clear), slack, cap)
    assert out["delays"].dtype == np.int32 and out["found"].dtype == bool and out["delays"].shape == ref["delays"].shape
    assert _equal(out, ref) and _equal(out, db.emu_delays(count, clear, slack, cap))
    assert _equal(out, eng.delay_search(dict(count=count, clear=clear), slack, cap))
    bare = eng.delay_search(dict(count=count), slack, cap)  # no clearances: the same integers, nothing written to clear
    assert db.same(bare, ref) and np.isnan(bare["clear"]).all()


def test_a_cap_per_vehicle_is_the_cap_of_every_set(eng):
    count, clear, slack, cap, ref = db.case("iid_4_5_cap")
    full = np.broadcast_to(np.asarray(cap), (16, 4)).copy()
    assert _equal(eng.delay_search(dict(count=count, clear=clear), slack, full), ref)
    full[3] = (5, 5, 5, 0)  # and a cap of one set's own
    out = eng.delay_search(dict(count=count, clear=clear), slack, full)
    assert _equal(out, db.search(count, clear, slack, full))
    assert (out["delays"][np.arange(16) != 3, 1] <= 0).all() and out["delays"][3, 3] <= 0 and out["found"].any()


def test_a_clearance_that_is_not_finite_is_not_free(eng):
    count = np.zeros((1, 1, 5), np.int32)
    for hole in (np.nan, np.inf):
        out = eng.delay_search(dict(count=count, clear=np.array([[[0.5, 0.4, hole, 0.3, 0.2]]])))
        assert out["delays"].tolist() == [[0, 1]] and out["clear"][0] == 0.3
    assert eng.delay_search(dict(count=count))["delays"].tolist() == [[0, 0]]
    assert not eng.delay_search(dict(count=count), slack=3)["found"][0]  # r > D: a result, not an error


def test_plan_delays_on_the_packaged_pool(eng):
    """The map searched on the device where it was computed equals the map read back and searched: all outputs, bit for bit.  Set 0 is
    resolved by (0, 0, 2, 0), with one sample of slack by (2, 0, 3, 0), sets 1 and 2 are not; the delayed tables of the answer are
    conflict-free on the device at every lag within the slack, and their clearance at lag 0 is the answer's."""
    from conflict_rez_amd import scenarios

    pool, D = cb.packaged_pool(), 12
    cm = eng.plan_conflicts(pool, D)
    for slack, want, rclear in ((0, [0, 0, 2, 0], 0.05371650552136141), (1, [2, 0, 3, 0], 0.09801251021964312)):
        out = eng.plan_delays(pool, D, slack=slack)
        assert _equal(out, eng.delay_search(cm, slack=slack)) and _equal(out, eng.plan_delays(pool, D, slack=slack))
        assert db.same(out, db.search(cm["count"], cm["clear"], slack))
        assert out["found"].tolist() == [True, False, False] and out["delays"][0].tolist() == want and abs(out["clear"][0] - rclear) <= 1e-12
        assert (out["delays"][1:] == -1).all() and (out["clear"][1:] == -np.inf).all()
        again = eng.plan_conflicts(scenarios.delay_tables(pool[0], out["delays"][0]), slack)
        assert (again["count"] == 0).all() and abs(again["clear"][..., slack].min() - out["clear"][0]) <= 1e-12
    # one set [V, T, 7] is P = 1; a cap that keeps vehicle 2 on time moves the delay to the others; another margin, another map
    one = eng.plan_delays(pool[0], D, cap=[12, 12, 0, 12])
    assert _equal(one, eng.delay_search(eng.plan_conflicts(pool[0], D), cap=[12, 12, 0, 12])) and one["delays"].shape == (1, 4)
    assert one["delays"][0, 2] <= 0 and one["delays"][0].tolist() != [0, 0, 2, 0]
    wide = eng.plan_conflicts(pool, D, margin=0.3)
    assert (wide["count"] != cm["count"]).any() and _equal(eng.plan_delays(pool, D, margin=0.3), eng.delay_search(wide))


def test_loop_plan_delays_leaves_the_loop_alone(eng):
    """From the pool that loop_init put on the device: equal to plan_delays on the host's copy; the loop's state is the same before
    and after, and it steps (state, clock) as it does without the call."""
    from conflict_rez_amd import scenarios

    pool, D, S = cb.packaged_pool(), 12, 6
    k0, noise = scenarios.sample_scenarios(S, pool[1], seed=5, spec=eng.spec)
    tof = (np.arange(S) % 3).astype(np.int32)
    eng.loop_init(pool, k0, noise, table_of=tof)
    eng.loop_step(); eng.loop_step()
    plain = eng.loop_get()
    eng.loop_init(pool, k0, noise, table_of=tof)
    eng.loop_step()
    before = eng.loop_get()
    for slack, cap in ((0, None), (1, None), (0, np.array([[12, 0, 12, 12]] * 3))):
        assert _equal(eng.loop_plan_delays(D, slack=slack, cap=cap), eng.plan_delays(pool, D, slack=slack, cap=cap))
    after = eng.loop_get()
    eng.loop_step()
    stepped = eng.loop_get()
    for k in plain:
        assert np.array_equal(before[k], after[k]) and np.array_equal(plain[k], stepped[k]), k
    eng.loop_init(pool[1], k0, noise)  # a single table is a pool of one
    one = eng.loop_plan_delays(D, margin=0.0)
    assert one["delays"].shape == (1, 4) and _equal(one, eng.plan_delays(pool[1], D, margin=0.0))


def test_refusals_and_what_is_served(eng):
    """Every refusal that needs no handle, with a handle: -1, its text, the outputs unwritten; what passes is served.  The loop form
    before any loop_init; V = 1 and NULL info / rclear are served, not refused."""
    from conflict_rez_amd import engine

    fresh = engine.Engine(eng.spec, max_batch=8)
    try:
        assert db.check_refusals(fresh.lib, fresh._h) == 2
        with pytest.raises(RuntimeError, match="cfz_loop_plan_delays: cfz_loop_init has not been called"):
            fresh.loop_plan_delays(3)
        with pytest.raises(RuntimeError, match="cfz_plan_delays: margin"):
            fresh.plan_delays(cb.synthetic(1, 2, 5), 3, margin=float("inf"))
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
        count, clear, slack, cap, ref = db.case("band_3_6_r1")
        count, clear = np.ascontiguousarray(count), np.ascontiguousarray(clear)
        delays, info, rclear = np.full((16, 3), 7, np.int32), np.full((16, 3), 7, np.int32), np.full(16, 7.0)
        assert fresh.lib.cfz_delay_search(fresh._h, 16, 3, 6, p(count), p(clear), 1, None, p(delays), None, None) == 0
        assert np.array_equal(delays, ref["delays"]) and (info == 7).all() and (rclear == 7.0).all()
        assert fresh.lib.cfz_delay_search(fresh._h, 16, 3, 6, p(count), None, 1, None, p(delays), p(info), p(rclear)) == 0
        assert np.array_equal(info[:, 1], ref["span"]) and (rclear == 7.0).all()  # no clearances: rclear is not written
        # V = 1: found, delay 0, +inf where clearances are given
        one, inf1 = np.full((16, 1), 7, np.int32), np.full((16, 3), 7, np.int32)
        empty_n, empty_c = np.zeros((16, 0, 7), np.int32), np.zeros((16, 0, 7))
        assert fresh.lib.cfz_delay_search(fresh._h, 16, 1, 3, p(empty_n), None, 0, None, p(one), p(inf1), p(rclear)) == 0
        assert (one == 0).all() and (inf1 == (1, 0, 0)).all() and (rclear == 7.0).all()
        assert fresh.lib.cfz_delay_search(fresh._h, 16, 1, 3, p(empty_n), p(empty_c), 0, None, p(one), None, p(rclear)) == 0 and (rclear == np.inf).all()
        out = fresh.plan_delays(cb.synthetic(2, 1, 5), 3)
        assert (out["delays"] == 0).all() and out["found"].all() and (out["clear"] == np.inf).all() and (out["span"] == 0).all()
    finally:
        fresh.close()
