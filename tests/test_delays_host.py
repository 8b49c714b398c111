"""The delay search over a conflict map on the host: the CPU build of the kernel source (csrc/cfz_delay.inl through
tests/emu/cfz_delay_emu.cpp) against an independent numpy statement of its definitions, at several lane counts, on hand-made maps and on
the packaged plans (where the answer is turned back into delayed tables and measured again); and the argument handling of the Python
layer and the C entry points (which refuse on the host, before any launch)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conflict_binding as cb  # noqa: E402
import delay_binding as db  # noqa: E402


@pytest.mark.parametrize("name", list(db.CASES))
def test_cpu_build_matches_the_numpy_statement(name):
    """All integers equal and the clearance the same double, with 1, 4 and 64 lanes: the dealing must not matter.  Without `clear`
    the integers are the same (every clearance of clear_map is finite) and the clearance is not written."""
    count, clear, slack, cap, ref = db.case(name)
    P, V = ref["delays"].shape
    assert V == db.CASES[name][1][1] and P == db.CASES[name][1][0]
    for lanes in (1, 4, 64):
        out = db.emu_delays(count, clear, slack, cap, lanes=lanes)
        assert db.same(out, ref) and np.array_equal(out["clear"], ref["clear"]), lanes
    bare = db.emu_delays(count, None, slack, cap)
    assert db.same(bare, ref) and np.isnan(bare["clear"]).all()


@pytest.mark.parametrize("name", list(db.CASES))
def test_the_answer_has_a_zero_respects_the_caps_and_is_free(name):
    count, clear, slack, cap, ref = db.case(name)
    out = db.emu_delays(count, clear, slack, cap)
    P, V = out["delays"].shape
    D = count.shape[2] // 2
    caps = np.broadcast_to(np.full(V, D) if cap is None else np.asarray(cap), (P, V))
    f = out["found"]
    assert (out["delays"][~f] == -1).all() and (out["span"][~f] == -1).all() and (out["total"][~f] == -1).all() and (out["clear"][~f] == -np.inf).all()
    d = out["delays"][f]
    assert (d.min(1) == 0).all() and (d <= caps[f]).all() and np.array_equal(d.max(1), out["span"][f]) and np.array_equal(d.sum(1), out["total"][f])
    for p in np.flatnonzero(f):
        at = [(q, out["delays"][p, w] - out["delays"][p, u] + D) for q, (u, w) in enumerate(db.pairs(V))]
        for q, j in at:
            assert slack <= j <= 2 * D - slack and (count[p, q, j - slack : j + slack + 1] == 0).all()
        assert out["clear"][p] == min([clear[p, q, j] for q, j in at], default=np.inf)  # the map's entry itself, ==


def test_the_cases_cover_what_they_are_for():
    """Tuple-rule decisions, several feasible vectors at the span, the stated spans of the smallest cases."""
    assert db.case("iid_2_0")[4]["span"].tolist().count(0) == 7 and db.case("iid_2_0")[4]["span"].tolist().count(-1) == 9
    assert set(db.case("iid_2_1")[4]["span"].tolist()) == {-1, 0, 1}
    assert db.case("iid_2_1")[4]["delays"][2].tolist() == [0, 1] and (db.case("iid_2_1")[0][2, 0] == 0).tolist() == [True, False, True]
    ref = db.case("iid_4_5_cap")[4]
    assert not ref["found"][0] and ref["found"][1:].all() and (ref["delays"][1:, 1] == 0).all() and ref["span"][1:].min() >= 1
    assert db.case("iid_8_1")[4]["span"].tolist() == [1, 1, 1, -1]
    assert db.case("band_4_10_r2")[4]["found"].sum() == 8 and db.case("band_4_10")[4]["span"].max() == 8
    one = db.case("iid_1_3")[4]
    assert one["found"].all() and (one["delays"] == 0).all() and one["delays"].shape == (16, 1) and (one["clear"] == np.inf).all()


def test_hand_made_maps():
    free = np.zeros((2, 6, 9), np.int32)
    out = db.emu_delays(free)
    assert (out["delays"] == 0).all() and out["found"].all() and (out["span"] == 0).all() and (out["total"] == 0).all()
    # V = 2, only the lags -1 and +1 free: (0, 1) and (1, 0) have the same span and total, the tuple rule takes (0, 1)
    count = np.array([[[0, 3, 0]]], np.int32)
    for out in (db.emu_delays(count), db.search(count)):
        assert out["delays"].tolist() == [[0, 1]] and out["span"].tolist() == [1] and out["total"].tolist() == [1]
    # a cap of 0 on vehicle 1 leaves (1, 0)
    for out in (db.emu_delays(count, cap=(1, 0)), db.search(count, cap=(1, 0))):
        assert out["delays"].tolist() == [[1, 0]]
    assert not db.emu_delays(count, cap=(0, 0))["found"][0]
    # a clearance that is not finite at the otherwise winning lag: the pair is not free there; without `clear` it is
    count = np.zeros((1, 1, 5), np.int32)
    for hole in (np.nan, np.inf, -np.inf):
        clear = np.array([[[0.5, 0.4, hole, 0.3, 0.2]]])
        for out in (db.emu_delays(count, clear), db.search(count, clear)):
            assert out["delays"].tolist() == [[0, 1]] and out["clear"][0] == 0.3
        assert db.emu_delays(count)["delays"].tolist() == [[0, 0]]
    # with slack 1 the window around the lag must be free as well, and inside the map: lag 0 is blocked, so the lags -2 and 2 are left
    count = np.array([[[0, 0, 0, 7, 0, 0, 0]]], np.int32)
    assert db.emu_delays(count)["delays"].tolist() == [[0, 1]]
    for out in (db.emu_delays(count, slack=1), db.search(count, slack=1)):
        assert out["delays"].tolist() == [[0, 2]]
    for out in (db.emu_delays(count, slack=2), db.search(count, slack=2)):
        assert not out["found"][0]


def test_a_slack_wider_than_the_window_finds_nothing():
    for V, D in ((2, 0), (3, 2), (4, 3)):
        free = np.zeros((2, V * (V - 1) // 2, 2 * D + 1), np.int32)
        assert db.emu_delays(free, slack=D)["found"].all() and (db.emu_delays(free, slack=D)["delays"] == 0).all()
        for out in (db.emu_delays(free, slack=D + 1), db.search(free, slack=D + 1), db.emu_delays(free, slack=10 ** 9)):
            assert not out["found"].any() and (out["delays"] == -1).all()


def test_packaged_pool_resolved_and_measured_again():
    """The CPU build of the map on the packaged pool, D = 12: set 0 is resolved by (0, 0, 2, 0), with one sample of slack by
    (2, 0, 3, 0); sets 1 and 2 have no solution inside the window.  The delayed tables of the answer are conflict-free at every lag
    within the slack, and their smallest clearance at lag 0 is the entry of the original map, the same double."""
    from conflict_rez_amd import scenarios

    pool, D = cb.packaged_pool(), 12
    cm = cb.emu_conflicts(pool, D)
    for slack, want, rclear in ((0, [0, 0, 2, 0], 0.05371650552136141), (1, [2, 0, 3, 0], 0.09801251021964312)):
        out = db.emu_delays(cm["count"], cm["clear"], slack)
        assert db.same(out, db.search(cm["count"], cm["clear"], slack))
        assert out["found"].tolist() == [True, False, False] and out["delays"][0].tolist() == want and out["clear"][0] == rclear
        again = cb.emu_conflicts(scenarios.delay_tables(pool[0], out["delays"][0]), slack)
        assert (again["count"] == 0).all() and again["clear"][..., slack].min() == out["clear"][0]  # (index slack: lag 0 of the delayed tables)


# ---- arguments ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from conflict_rez_amd import engine

    return engine.load_library()


def test_python_side_refusals(lib):
    """An Engine without a handle (no GPU needed): slack and cap are refused by the Python layer, and what passes it reaches the library,
    which refuses the null handle last."""
    from conflict_rez_amd import engine, scenarios

    e = engine.Engine.__new__(engine.Engine)
    e.lib, e.spec, e._h, e._S, e._V, e._P = lib, scenarios.parking_lot_spec(), None, 0, 0, 0
    cmap = dict(count=np.zeros((3, 6, 9), np.int32))
    tab = cb.synthetic(3, 4, 64)
    for call in (lambda **k: e.delay_search(cmap, **k), lambda **k: e.plan_delays(tab, 4, **k)):
        for bad in (-1, 1.5):
            with pytest.raises(ValueError, match="slack"):
                call(slack=bad)
        for bad in ([4, 4, 4], np.zeros((2, 4)), np.zeros((3, 4, 1)), 3):
            with pytest.raises(ValueError, match="cap of shape"):
                call(cap=bad)
        for bad in ([0, 5, 0, 0], [0, -1, 0, 0], [0, 0.5, 0, 0], np.full((3, 4), 9)):
            with pytest.raises(ValueError, match="cap must hold whole numbers"):
                call(cap=bad)
    with pytest.raises(ValueError, match="slack"):
        e.loop_plan_delays(4, slack=-2)
    with pytest.raises(ValueError, match="max_lag"):
        e.plan_delays(tab, -1)
    for bad in (np.zeros((3, 6, 8), np.int32), np.zeros((6, 9), np.int32), np.zeros((3, 5, 9), np.int32)):
        with pytest.raises(ValueError, match="count of shape|pairs are not"):
            e.delay_search(dict(count=bad))
    with pytest.raises(ValueError, match="clear of the shape"):
        e.delay_search(dict(cmap, clear=np.zeros((3, 6, 8))))
    for call, name in ((lambda: e.delay_search(cmap, slack=2, cap=[4, 0, 4, 4]), "cfz_delay_search"), (lambda: e.plan_delays(tab, 4, cap=np.full((3, 4), 4)), "cfz_plan_delays")):
        with pytest.raises(RuntimeError, match=name + ": null handle"):
            call()
    with pytest.raises(RuntimeError, match="cfz_loop_plan_delays: cfz_loop_init has not been called"):
        e.loop_plan_delays(4)
    r, c = engine._delay_args(np.int64(2), [1, 0, 2, 2], 3, 4, 2)
    assert r == 2 and c.dtype == np.int32 and c.flags.c_contiguous and c.tolist() == [[1, 0, 2, 2]] * 3
    assert engine._delay_args(0, None, 3, 4, 2) == (0, None)


def test_library_refusals_come_before_the_handle(lib):
    """Every refusal of the C entry points that needs no handle, by its text, with a null handle, which is refused last; the outputs stay
    unwritten."""
    assert db.check_refusals(lib, None) == 0
