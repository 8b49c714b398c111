"""The conflict map of a plan pool on the GPU (cfz_plan_conflicts / cfz_loop_plan_conflicts, conflict_kernel over
csrc/cfz_conflict.inl): within 1e-12 of the numpy statement and of the CPU build of the same source with every integer equal and
nothing exempted, the same bits on every call and from the loop's own pool, consistent with the existing audit, and without effect on
the closed loop."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conflict_binding as cb  # noqa: E402

KEYS = ("clear",) + cb.INTS


@pytest.fixture(scope="module")
def eng():
    import __graft_entry__ as g

    g.build()
    from conflict_rez_amd import engine, scenarios

    e = engine.Engine(scenarios.parking_lot_spec(), max_batch=1024)
    yield e
    e.close()


def _same(a, b):
    for k in KEYS + ("pairs", "lags"):
        assert np.array_equal(a[k], b[k]), k


def _against_cpu(out, cpu):
    assert np.abs(out["clear"] - cpu["clear"]).max(initial=0.0) <= 1e-12
    for n in cb.INTS:
        assert np.array_equal(out[n], cpu[n]), n


@pytest.mark.parametrize("P", cb.PS)
@pytest.mark.parametrize("V,T,D", cb.SHAPES)
def test_synthetic_plans(eng, P, V, T, D):
    """The shapes of the host tests on the device (V = 2 and V = 3 on the 4-vehicle engine): no lag, a window wider than the plan, steps
    no multiple of 64, lags no multiple of 4."""
    assert tuple(eng.spec.g) == cb.G and eng.spec.dmin == cb.MARGIN
    tab = cb.synthetic(P, V, T)
    out = eng.plan_conflicts(tab, D)
    assert out["clear"].shape == (P, V * (V - 1) // 2, 2 * D + 1) and out["pairs"].tolist() == [list(q) for q in cb.pairs(V)]
    assert out["lags"].tolist() == list(range(-D, D + 1))
    assert cb.check_against_statement(out, cb.synthetic_reference(P, V, T, D)) == 0
    _against_cpu(out, cb.emu_conflicts(tab, D))


def test_five_vehicles_one_vehicle_and_one_set(eng):
    """V = 5 (ten pairs) on the 4-vehicle engine; a [V, T, 7] table is P = 1; V = 1 has no pairs; another margin."""
    tab = cb.synthetic(2, 5, 33)
    ref = cb.conflicts(tab, 5, margin=0.4)
    out = eng.plan_conflicts(tab, 5, margin=0.4)
    assert cb.check_against_statement(out, ref) == 0 and (out["count"] != eng.plan_conflicts(tab, 5)["count"]).any()
    _against_cpu(out, cb.emu_conflicts(tab, 5, margin=0.4))
    one = eng.plan_conflicts(tab[1], 5, margin=0.4)
    for k in KEYS:
        assert np.array_equal(one[k][0], out[k][1]), k
    none = eng.plan_conflicts(tab[:, :1], 5)
    assert all(none[k].shape == (2, 0, 11) for k in KEYS) and none["pairs"].shape == (0, 2)


def test_packaged_pool(eng):
    """Three packaged plan sets over 81 lags: against the numpy statement; the same bits when called again; the same bits from the
    pool that loop_init put on the device; and the closed loop steps as it does without the call."""
    from conflict_rez_amd import scenarios

    pool, D = cb.packaged_pool(), 40
    out = eng.plan_conflicts(pool, D)
    assert cb.check_against_statement(out, cb.packaged_reference(D)) == 0
    _same(out, eng.plan_conflicts(pool, D))
    S = 6
    k0, noise = scenarios.sample_scenarios(S, pool[1], seed=5, spec=eng.spec)
    tof = (np.arange(S) % 3).astype(np.int32)
    eng.loop_init(pool, k0, noise, table_of=tof)
    eng.loop_step()
    plain = eng.loop_get()
    eng.loop_init(pool, k0, noise, table_of=tof)
    _same(out, eng.loop_plan_conflicts(D))
    eng.loop_step()
    after = eng.loop_get()
    _same(out, eng.loop_plan_conflicts(D))
    for k in plain:
        assert np.array_equal(plain[k], after[k]), k
    # a single table is a pool of one
    eng.loop_init(pool[1], k0, noise)
    one = eng.loop_plan_conflicts(D, margin=0.0)
    assert one["clear"].shape == (1, 6, 81) and np.array_equal(one["clear"][0], out["clear"][1]) and np.array_equal(one["when"][0], out["when"][1])


def test_against_the_audit(eng):
    """Every (pair, lag) as a two-vehicle scenario of the existing audit: the index sequences of the definition, written out as a
    trajectory (the last step repeated up to the longest), give the audit's vehicle-vehicle clearance and its step."""
    from conflict_rez_amd import scenarios

    pl, _ = scenarios.load_reference_table(kind="planned")
    T, D, lags = pl.shape[1], 40, (-40, -1, 0, 1, 23, 40)
    out = eng.plan_conflicts(pl, D, margin=0.0)
    prs = cb.pairs(4)
    K, S = T + D, len(prs) * len(lags)
    traj = np.zeros((K, S, 2, 7))
    pick = []
    for q, (u, w) in enumerate(prs):
        for tau in lags:
            iu, iw = cb.lag_indices(T, tau)
            iu, iw = (np.concatenate([i, np.full(K - len(i), i[-1])]) for i in (iu, iw))
            traj[:, len(pick), 0], traj[:, len(pick), 1] = pl[u, iu], pl[w, iw]
            pick.append((0, q, tau + D))
    pick = tuple(np.array(pick).T)
    aud = eng.audit(traj, np.zeros((S, 2, 3)))
    assert np.abs(aud["clear"][:, 0] - out["clear"][pick]).max() <= 1e-12
    assert np.array_equal(aud["where"][:, 0], out["when"][pick])
    assert (aud["where"][:, 1:3] == (0, 1)).all()
    off = aud["clear"][:, 1] > 0  # no contact with an obstacle: the audit's first contact is the pair's
    assert off.sum() > S // 2 and (out["first"][pick][off] >= 0).any() and (out["first"][pick][off] < 0).any()
    assert np.array_equal(aud["first_contact"][off], out["first"][pick][off])


def test_plans_longer_than_the_staging_bound(eng):
    """The smallest T whose columns are read from global memory instead of LDS."""
    T = cb.lds_t() + 1
    tab = cb.synthetic(1, 2, T)
    out = eng.plan_conflicts(tab, 1)
    _against_cpu(out, cb.emu_conflicts(tab, 1))
    assert cb.check_against_statement(out, cb.conflicts(tab, 1)) == 0
    assert (out["when"] > 0).all() and (out["count"] > 0).all()
    # and the largest that is staged
    tab = cb.synthetic(1, 2, T - 1)
    assert cb.check_against_statement(eng.plan_conflicts(tab, 1), cb.conflicts(tab, 1)) == 0


def test_device_refusals(eng):
    """What needs the handle: the loop form before any loop_init; V = 1 and NULL outputs are served, not refused."""
    from conflict_rez_amd import engine

    fresh = engine.Engine(eng.spec, max_batch=8)
    try:
        with pytest.raises(RuntimeError, match="cfz_loop_plan_conflicts: cfz_loop_init has not been called"):
            fresh.loop_plan_conflicts(3)
        with pytest.raises(RuntimeError, match="cfz_plan_conflicts: margin"):
            fresh.plan_conflicts(cb.synthetic(1, 2, 5), 3, margin=float("inf"))
        tab = np.ascontiguousarray(cb.synthetic(1, 3, 70))
        ref = fresh.plan_conflicts(tab, 7)
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
        clear, info = np.zeros((1, 3, 15)), np.zeros((1, 3, 15, 3), np.int32)
        assert fresh.lib.cfz_plan_conflicts(fresh._h, 1, 3, 70, p(tab), 7, 0.05, p(clear), None) == 0 and np.array_equal(clear, ref["clear"])
        assert fresh.lib.cfz_plan_conflicts(fresh._h, 1, 3, 70, p(tab), 7, 0.05, None, p(info)) == 0 and np.array_equal(info[..., 2], ref["count"])
        clear[:] = 7.0
        assert fresh.lib.cfz_plan_conflicts(fresh._h, 1, 1, 70, p(tab), 7, 0.05, p(clear), None) == 0 and (clear == 7.0).all()
    finally:
        fresh.close()
