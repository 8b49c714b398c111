"""The coordination diagrams and the hold-point schedules without a GPU: the CPU build of the kernel sources (tests/emu/cfz_schedule_emu.cpp)
against the independent statements of tests/schedule_binding.py, against an exhaustive enumeration, against the conflict map and the
delay search, and the helpers of conflict_rez_amd/scenarios.py that go with them."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conflict_binding as cb  # noqa: E402
import delay_binding as db  # noqa: E402
import schedule_binding as sb  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from conflict_rez_amd import engine

    return engine.load_library()


@pytest.mark.parametrize("name", list(sb.CASES))
def test_cpu_build_matches_the_statements(name):
    """The diagram equal except where the statement's distance lies within 1e-12 of the margin, of which there is none; both sides
    transposes of each other; every integer of the schedules equal, however the orders are dealt out; the result is what it promises."""
    tables, hold, length, H, slack, orders, B, near, ref = sb.case(name)
    sides = sb.emu_diagram(tables, sb.MARGIN, length)
    assert int(near.sum()) == 0
    assert np.array_equal(sides[:, :, 0], B) and np.array_equal(sides[:, :, 1], B.transpose(0, 1, 3, 2))
    for waves in (4, 1, 3):
        assert sb.same(sb.emu_schedule_diagram(sides, hold, H, slack, orders, length, waves), ref)
    assert sb.check_schedules(ref, B, hold, H, slack, length)


def test_the_cases_cover_what_they_are_for():
    found = np.concatenate([sb.case(n)[8]["found"] for n in sb.CASES])
    waits = np.concatenate([sb.case(n)[8]["waits"].ravel() for n in sb.CASES])
    assert found.any() and (~found).any() and (waits > 0).any()
    assert sb.case("t65_lds_edge")[3] == sb.lds_edge() == sb.case("t65_global")[3] - 1 and sb.history_in_lds(4, 301, 365)
    late = [n for n in sb.CASES if (sb.case(n)[8]["order"] > 0).any()]
    inner = [n for n in sb.CASES if any((s[:a][np.diff(s[: a + 1]) == 0] > 0).any() for r in [sb.case(n)[8]] for p in np.flatnonzero(r["found"])
                                        for s, a in zip(r["schedule"][p], r["arrival"][p]))]
    assert late and inner, (late, inner)  # an answer that is not the first order; a wait that is not at the first sample


def test_crafted_sets():
    """A goal that is free, then blocked, then free again: the arrival is the start of the last run; an answer found only under the last
    order of the list; a start that is blocked: nothing feasible; a batch with both."""
    tab, length, hold = sb.crafted()
    B, near, ref = sb.crafted_reference()
    assert int(near.sum()) == 0
    goal = ~B[0, 0, :, 12]  # vehicle 1 at its goal against vehicle 0's samples: free, blocked, free
    runs = np.flatnonzero(np.diff(goal.astype(int)))
    assert goal[12] and len(runs) == 2 and not goal[runs[0] + 1]
    out = sb.emu_schedule(tab, hold, 77, length=length)
    assert sb.same(out, ref) and sb.check_schedules(out, B, hold, 77, 0, length)
    assert out["found"].tolist() == [True, False, True] and out["order"].tolist() == [0, -1, 0] and out["feasible_orders"].tolist() == [1, 0, 2]
    assert out["arrival"][0, 1] > runs[1] and out["waits"][0].tolist() == [0, out["arrival"][0, 1] - 12] and (out["waits"][2] == 0).all()
    assert B[1, 0, 0, 0] and (out["schedule"][1] == -1).all() and (out["arrival"][1] == -1).all()
    rev = sb.emu_schedule(tab, hold, 77, length=length, orders=[[1, 0], [0, 1]])  # the same answer, late in the list
    assert rev["order"].tolist() == [1, -1, 0] and sb.same(rev, out, ("schedule", "arrival", "waits", "found", "makespan", "total"))
    assert sb.same(rev, sb.schedule(B, hold, 77, 0, [[1, 0], [0, 1]], length))


@pytest.mark.parametrize("V", [2, 3])
def test_exhaustive_enumeration(V):
    """Random diagrams and holds, T <= 5, H <= 9: for the last vehicle of the winning order every schedule is enumerated; its arrival is
    the smallest of the feasible ones and its schedule their pointwise maximum.  Statement and CPU build agree on everything."""
    rng = np.random.default_rng(V)
    npair, seen = V * (V - 1) // 2, 0
    for trial in range(160):
        T = int(rng.integers(1, 6))
        H = int(rng.integers(T, 10))
        slack = int(rng.integers(0, 2))
        length = rng.integers(1, T + 1, (1, V)).astype(np.int32)
        B = rng.random((1, npair, T, T)) < 0.15
        for q, (u, w) in enumerate(sb.pairs(V)):
            B[0, q, length[0, u]:, :] = False
            B[0, q, :, length[0, w]:] = False
        hold = (rng.random((1, V, T)) < 0.5).astype(np.uint8)
        sides = np.stack([B, B.transpose(0, 1, 3, 2)], 2)
        out = sb.emu_schedule_diagram(sides, hold, H, slack, None, length)
        ref = sb.schedule(B, hold, H, slack, None, length)
        assert sb.same(out, ref) and sb.check_schedules(out, B, hold, H, slack, length)
        if not out["found"][0]:
            continue
        pi = sb.all_orders(V)[out["order"][0]]
        v, g, s = int(pi[-1]), int(length[0, pi[-1]]) - 1, out["schedule"][0]
        feas = []
        for steps in itertools.product((0, 1), repeat=H - 1):
            c = np.concatenate([[0], np.cumsum(steps, dtype=int)]).astype(int)
            if c[-1] != g or any(st == 0 and not (hold[0, v, c[t]] or c[t] == g) for t, st in enumerate(steps)):
                continue
            ok = True
            for e in pi[:-1]:
                for d in range(-slack, slack + 1):
                    tt = np.clip(np.arange(H) + d, 0, H - 1)
                    Bq = B[0, sb.pairs(V).index((min(v, e), max(v, e)))]
                    hit = (Bq[c, s[e, tt]] | Bq[c[tt], s[e]]) if v < e else (Bq[s[e, tt], c] | Bq[s[e], c[tt]])
                    ok &= not hit.any()
            if ok:
                feas.append(c)
        assert feas and min(int(np.argmax(c == g)) for c in feas) == out["arrival"][0, v]
        assert np.array_equal(np.max(feas, axis=0), s[v])
        seen += 1
    assert seen >= 40


@pytest.mark.parametrize("shape", [(2, 3, 33, 7), (1, 4, 65, 12)])
def test_the_conflict_map_is_the_diagrams_diagonal_sums(shape):
    P, V, T, D = shape
    tables = cb.synthetic(P, V, T, sb.SEED)
    sides, cm = sb.emu_diagram(tables), cb.emu_conflicts(tables, D)
    for tau in range(-D, D + 1):
        iu, iw = cb.lag_indices(T, tau)
        assert np.array_equal(sides[:, :, 0][:, :, iu, iw].sum(-1), cm["count"][:, :, tau + D]), tau
    assert cm["count"].any()


def test_start_only_holds_are_the_delay_search():
    """V = 2, equal lengths, slack 0, holds at sample 0 only: the waits are the delays of the delay search over the conflict map,
    wherever that finds an answer inside its window (H = T + D gives the schedule the same room)."""
    P, T, D = 24, 33, 12
    tables = sb.crossing(P, 2, T, sb.SEED)
    hold = np.zeros((P, 2, T), np.uint8)
    hold[:, :, 0] = 1
    out = sb.emu_schedule(tables, hold, T + D)
    dl = db.search(cb.emu_conflicts(tables, D)["count"])
    f = dl["found"]
    assert f.sum() >= 8 and (dl["span"][f] > 0).sum() >= 3 and out["found"][f].all()
    assert np.array_equal(out["waits"][f], dl["delays"][f])


def test_packaged_pool_start_only_and_rest_sample_holds():
    """The packaged pool, horizon T + 64.  Holds at the start only: set 0 gives the delay search's answers, (0, 0, 2, 0) and with one
    sample of slack (2, 0, 3, 0); sets 1 and 2 have no feasible order.  With holds at the rest samples sets 1 and 2 are resolved under
    order (1, 2, 0, 3) by two waits at cusps, without a longer makespan.  CPU build and statement agree on every integer."""
    from conflict_rez_amd import scenarios

    pool = cb.packaged_pool()
    T, H = pool.shape[2], pool.shape[2] + 64
    length = scenarios.plan_lengths(pool)
    assert length[1].tolist() == [158, 79, 95, 104] and length[2].tolist() == [138, 59, 75, 84]
    full = scenarios.hold_points(pool, 0.1, length)
    start = np.zeros_like(full)
    start[:, :, 0] = 1
    B, near = sb.diagram(pool, sb.MARGIN, length)
    sides = sb.emu_diagram(pool, sb.MARGIN, length)
    assert int(near.sum()) == 0 and np.array_equal(sides[:, :, 0], B)
    for slack, want in ((0, [0, 0, 2, 0]), (1, [2, 0, 3, 0])):
        out = sb.emu_schedule_diagram(sides, start, H, slack, None, length)
        assert out["found"].tolist() == [True, False, False] and out["waits"][0].tolist() == want and (out["feasible_orders"][1:] == 0).all()
        assert sb.same({k: v[:1] for k, v in out.items()}, sb.schedule(B[:1], start[:1], H, slack, None, length[:1]))
    out = sb.emu_schedule_diagram(sides, full, H, 0, None, length)
    assert sb.same(out, sb.schedule(B, full, H, 0, None, length)) and sb.check_schedules(out, B, full, H, 0, length)
    assert out["found"].all() and out["order"][1:].tolist() == [8, 8] and sb.all_orders(4)[8].tolist() == [1, 2, 0, 3]
    assert out["waits"][1:].tolist() == [[1, 0, 0, 16]] * 2 and out["makespan"][1:].tolist() == [158, 138]
    for p, at in ((1, (24, 44)), (2, (4, 24))):
        s = out["schedule"][p]
        for v, i in zip((0, 3), at):
            rest = s[v, :-1][(np.diff(s[v]) == 0) & (s[v, :-1] < length[p, v] - 1)]
            assert set(rest.tolist()) == {i} and abs(pool[p, v, i, 3]) <= 0.1
    # the scheduled tables are conflict-free at lag 0 in the CPU build of the conflict map
    again = cb.emu_conflicts(scenarios.schedule_tables(pool, out["schedule"]), 0)
    assert (again["count"] == 0).all()


def test_schedule_tables_is_delay_tables_for_a_start_delay():
    from conflict_rez_amd import scenarios

    pool = cb.packaged_pool()
    P, V, T = pool.shape[:3]
    rng = np.random.default_rng(5)
    d = rng.integers(0, 9, (P, V))
    H = T + int(d.max()) + 5
    s = np.clip(np.arange(H)[None, None, :] - d[:, :, None], 0, T - 1)
    a, b = scenarios.schedule_tables(pool, s), scenarios.delay_tables(pool, d)
    assert a.shape == (P, V, H, 7) and np.array_equal(a[:, :, : b.shape[2]].view(np.uint64), b.view(np.uint64))
    assert np.array_equal(a[:, :, b.shape[2]:], np.repeat(pool[:, :, -1:], H - b.shape[2], axis=2))
    one = scenarios.schedule_tables(pool[1], s[1])
    assert one.shape == (V, H, 7) and np.array_equal(one, a[1])
    # a wait in the middle: the pose and the steering angle are kept, v = a = w = 0; the row that leaves the sample is a copy
    s2 = np.minimum(np.array([[0, 1, 2, 2, 2, 3, 4, 5]]), 4)
    t2 = scenarios.schedule_tables(pool[1, :1, :5], s2)
    assert np.array_equal(t2[0, 2:4, :3], pool[1, 0, [2, 2], :3]) and (t2[0, 2:4][:, [3, 5, 6]] == 0).all() and t2[0, 2, 4] == pool[1, 0, 2, 4]
    assert np.array_equal(t2[0, 4], pool[1, 0, 2]) and np.array_equal(t2[0, 6:], pool[1, 0, [4, 4]])
    for bad in (s[:, :, ::-1], s - 1, s.astype(float), s[:, :2]):
        with pytest.raises(ValueError):
            scenarios.schedule_tables(pool, bad)


def test_hold_points_and_plan_lengths_on_a_padded_table():
    from conflict_rez_amd import scenarios

    tab = np.zeros((2, 9, 7))
    tab[0, :, 0] = [0, 1, 2, 3, 3, 4, 5, 5, 5]          # drives, rests at sample 3-4 (same pose), arrives at sample 6, padded
    tab[0, :, 3] = [0.05, 1, 1, 0.0, 0.08, -1, -0.5, 0.3, 0.3]
    tab[1, :, 2] = 0.5                                  # never moves: length 1
    tab[1, :, 3] = 1.0
    assert scenarios.plan_lengths(tab).tolist() == [7, 1] and scenarios.plan_lengths(tab).dtype == np.int32
    assert scenarios.plan_lengths(tab[None]).tolist() == [[7, 1]]
    h = scenarios.hold_points(tab)
    assert h.dtype == np.uint8 and h.shape == (2, 9)
    assert h[0].tolist() == [1, 0, 0, 1, 1, 0, 1, 1, 1] and h[1].tolist() == [1] * 9
    assert scenarios.hold_points(tab, v_tol=0.01)[0].tolist() == [1, 0, 0, 1, 0, 0, 1, 1, 1]
    assert scenarios.hold_points(tab, length=[9, 9])[0].tolist() == [1, 0, 0, 1, 1, 0, 0, 0, 1]
    full = np.arange(6.0)[None, :, None] * np.ones((1, 6, 7))
    assert scenarios.plan_lengths(full).tolist() == [6]


def test_python_side_refusals(lib):
    """An Engine without a handle (no GPU needed): what the Python layer refuses, and what passes it reaches the library, which refuses
    the null handle last."""
    from conflict_rez_amd import engine, scenarios

    e = engine.Engine.__new__(engine.Engine)
    e.lib, e.spec, e._h, e._S, e._V, e._P, e._T = lib, scenarios.parking_lot_spec(), None, 0, 0, 0, 0
    tab, hold = cb.synthetic(2, 3, 40, sb.SEED), sb.random_hold(2, 3, 40)
    for kw, text in ((dict(hold=hold[:, :2]), "expected hold"), (dict(slack=-1), "slack"), (dict(slack=0.5), "slack"),
                     (dict(horizon=50.5), "horizon"), (dict(orders=[[0, 1]]), "orders"), (dict(orders=[[0.0, 1.0, 2.0]]), "orders"),
                     (dict(length=[40, 40]), "length"), (dict(length=[40.0] * 3), "length")):
        with pytest.raises(ValueError, match=text):
            e.plan_schedule(tab, **{"hold": hold, **kw})
    with pytest.raises(ValueError, match="orders is required"):
        e.plan_schedule(cb.synthetic(1, 5, 8, sb.SEED), np.ones((5, 8)))
    with pytest.raises(ValueError, match="expected tables"):
        e.plan_coordination(np.zeros((3, 4)))
    for call, name in ((lambda: e.plan_schedule(tab, hold), "cfz_plan_schedule"), (lambda: e.plan_schedule(tab[0], hold[0], orders=[2, 1, 0]), "cfz_plan_schedule"),
                       (lambda: e.plan_coordination(tab, length=[40, 30, 20]), "cfz_plan_coordination")):
        with pytest.raises(RuntimeError, match=name + ": null handle"):
            call()
    with pytest.raises(RuntimeError, match="cfz_plan_schedule: an order is not a permutation"):
        e.plan_schedule(tab, hold, orders=[[0, 1, 1]])
    with pytest.raises(RuntimeError, match="cfz_plan_schedule: H must not be below T"):
        e.plan_schedule(tab, hold, horizon=39)
    with pytest.raises(RuntimeError, match="cfz_loop_plan_schedule: cfz_loop_init has not been called"):
        e.loop_plan_schedule(hold)


def test_library_refusals_come_before_the_handle(lib):
    assert sb.check_refusals(lib, None) == 0
