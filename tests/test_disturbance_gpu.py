"""Disturbances of the closed loop (`cfz_loop_set_disturbance`, `cfz_loop_disturbance`; csrc/cfz_disturb.inl) on the GPU.

A disturbed step of (scenario s, vehicle v) at step t, d = level[s] * sigma * z(seed, stream[s], v, t): the solver is pinned to the
measurement state + d[0:5]; the applied input is clip((a0, w0) + d[5:7]) to the input box; the new true state is the plant from the true
state with that input, plus d[7:12]; the record keeps the true state and the applied input.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import disturbance_binding as db  # noqa: E402
from loop_cases import against_replay, orders as _orders, planned as _planned, run as _run, same as _same, stepwise  # noqa: E402

SIG = db.SIGMA
SEED = 2024


@pytest.fixture(scope="module")
def eng():
    import __graft_entry__ as g

    g.build()
    from conflict_rez_amd import engine, scenarios

    e = engine.Engine(scenarios.parking_lot_spec(), max_batch=1024)
    yield e
    e.close()


@pytest.mark.parametrize("exchange", ["jacobi", "sequential"])
@pytest.mark.parametrize("how", ["step", "run"])
def test_off_is_off(eng, how, exchange):
    """(5) No disturbance call, a disturbance with every sigma zero (the disturbed kernels run) and set-then-unset give equal state,
    prediction, status, iterations and record, bit for bit.  S = 64, planned table, feasible starts, K = 6."""
    S, K, V = 64, 6, eng.spec.n_nbr + 1
    table, k0, noise = _planned(eng, S)
    init = ((table, k0, noise), {})
    order = _orders(S, V, 11) if exchange == "sequential" else None
    zero = np.zeros(5)

    def zeros(e):
        e.loop_set_disturbance(SEED, meas=zero, act=zero[:2], proc=zero)
        assert not e.loop_disturbance(0, K).any()

    def set_unset(e):
        e.loop_set_disturbance(SEED, **SIG)
        e.loop_set_disturbance(SEED)
        with pytest.raises(RuntimeError, match="no disturbance is set"):
            e.loop_disturbance(0, 1)

    plain = _run(eng, init, K, how, order)
    assert (plain["rec_status"] == 0).mean() > 0.5
    _same(plain, _run(eng, init, K, how, order, zeros), "all sigmas zero")
    _same(plain, _run(eng, init, K, how, order, set_unset), "set, then unset")


@pytest.mark.parametrize("exchange", ["jacobi", "sequential"])
def test_stepwise_equals_persistent_under_noise(eng, exchange):
    """(6) With the base sigmas on, K x loop_step, loop_run(K) and loop_run(3); loop_run(K - 3) give the same record, state, predictions,
    status and iterations, bit for bit; the state is not the undisturbed run's."""
    S, K, V = 64, 6, eng.spec.n_nbr + 1
    table, k0, noise = _planned(eng, S)
    init = ((table, k0, noise), {})
    order = _orders(S, V, 11) if exchange == "sequential" else None
    on = lambda e: e.loop_set_disturbance(SEED, **SIG)
    step = _run(eng, init, K, "step", order, on)
    _same(step, _run(eng, init, K, "run", order, on), "one launch")
    _same(step, _run(eng, init, K, (3, K - 3), order, on), "split launch")
    plain = _run(eng, init, K, "run", order)
    moved = np.abs(step["state"] - plain["state"]).max(-1)
    print(f"{exchange}: final states moved by up to {moved.max():.3f} m against the undisturbed run; "
          f"{int((step['rec_status'] == 0).sum())} of {step['rec_status'].size} disturbed solves converged")
    assert (moved > 0).all()


def test_export_is_the_loops_noise(eng):
    """(7) loop_disturbance equals the numpy statement within 1e-13 x level x sigma; it scales exactly with the level; a level-0 scenario
    inside a disturbed batch equals its undisturbed run bit for bit; running the loop does not change it."""
    S, K, V = 16, 5, eng.spec.n_nbr + 1
    table, k0, noise = _planned(eng, S)
    init = ((table, k0, noise), {})
    sig = db.sigma12(**SIG)
    level = np.array([0.0, 1.0, 0.5, 2.0, 0.25, 4.0, 1.7, 0.3] * 2)
    stream = np.array([5] * 6 + [6, 7] + list(range(100, 108)), np.uint32)  # scenarios 0..5 share one stream
    plain = _run(eng, init, K, "run")
    got = {}

    def on(e):
        e.loop_set_disturbance(SEED, level=level, stream=stream, **SIG)
        got["before"] = e.loop_disturbance(0, K + 3)

    dist = _run(eng, init, K, "run", None, on)
    d = eng.loop_disturbance(0, K + 3)
    assert np.array_equal(d, got["before"]) and np.array_equal(d[2:4], eng.loop_disturbance(2, 2))
    assert d.shape == (K + 3, S, V, 12)
    ref = db.disturbance(SEED, sig, level, stream, V, 0, K + 3)
    err = np.abs(d - ref) / np.maximum(level[None, :, None, None] * sig, 1e-300)
    print(f"largest |d - numpy| / (level sigma) = {err.max():.2e}")
    assert (np.abs(d - ref) <= 1e-13 * level[None, :, None, None] * sig).all()
    for s in (2, 3, 4, 5):  # powers of two: the products are exact multiples of scenario 1's
        assert np.array_equal(d[:, s], level[s] * d[:, 1]), s
    assert not d[:, 0].any() and d[:, 1][..., sig > 0].all() and not d[..., sig == 0].any()
    for k, val in dist.items():  # scenario 0 has level 0
        assert np.array_equal(val[:, 0] if k.startswith("rec_") else val[0], plain[k][:, 0] if k.startswith("rec_") else plain[k][0]), k
    assert not np.array_equal(dist["state"][1], plain["state"][1])
    # default level and stream: 1 and s
    eng.loop_set_disturbance(SEED, **SIG)
    d1 = eng.loop_disturbance(4, 2)
    assert (np.abs(d1 - db.disturbance(SEED, sig, np.ones(S), np.arange(S), V, 4, 2)) <= 1e-13 * sig).all()


def test_streams_belong_to_scenarios(eng):
    """(8) A subset of a mixed pool's scenarios, run alone with `stream=` their ids in the full batch, equals its rows of the full run
    bit for bit, persistent and stepwise.  Two replicas of one scenario with equal stream ids are equal, with different ids not."""
    from conflict_rez_amd import scenarios
    from test_scenario_loop_gpu import _three_tables

    tabs, pool = _three_tables()
    S, K = 24, 6
    tof = np.random.default_rng(3).integers(0, 3, S).astype(np.int32)
    k0, noise = scenarios.sample_scenarios(S, tabs[2], seed=9, spec=eng.spec)
    sel = np.array([1, 4, 5, 11, 17, 22])
    assert len(set(tof[sel])) == 3
    full_init = ((pool, k0, noise), dict(table_of=tof))
    sub_init = ((pool, k0[sel], noise[sel]), dict(table_of=tof[sel]))
    for how in ("run", "step"):
        full = _run(eng, full_init, K, how, None, lambda e: e.loop_set_disturbance(SEED, **SIG))
        sub = _run(eng, sub_init, K, how, None, lambda e: e.loop_set_disturbance(SEED, stream=sel, **SIG))
        _same(full, sub, how, rows=sel)
        wrong = _run(eng, sub_init, K, how, None, lambda e: e.loop_set_disturbance(SEED, **SIG))  # streams 0..5 instead
        assert not np.array_equal(wrong["state"], sub["state"])
    rep = np.array([7, 7, 7])
    rep_init = ((pool, k0[rep], noise[rep]), dict(table_of=tof[rep]))
    r = _run(eng, rep_init, K, "run", None, lambda e: e.loop_set_disturbance(SEED, stream=np.array([40, 40, 41]), **SIG))
    for k, val in r.items():
        x = np.moveaxis(val, 1, 0) if k.startswith("rec_") else val  # scenarios first
        assert np.array_equal(x[0], x[1]), k
    assert not np.array_equal(r["state"][0], r["state"][2])


def test_each_group_does_what_it_says(eng):
    """(9) Stepwise, one group of the base sigmas on at a time, d from the export.
    act: recorded input = clip(prediction's first input + d[5:7]) exactly, inside the input box; with a large sigma some sit on it.
    proc: recorded state - plant(previous recorded state, recorded input) = d[7:12] within 1e-12 (test_record's tolerance).
    meas: the true state obeys the plant (1e-12); a converged prediction starts at previous state + d[0:5] within constr_viol_tol."""
    from conflict_rez_amd import engine
    from oracle.dynamics import plant_step

    S, K, V = 16, 6, eng.spec.n_nbr + 1
    table, k0, noise = _planned(eng, S)
    box = np.asarray(eng.spec.bounds, float).reshape(6, 2)[4:6]  # a, w
    tol = engine.default_options().constr_viol_tol

    def loop(**groups):
        eng.loop_init(table, k0, noise)
        eng.loop_set_disturbance(SEED, **groups)
        eng.loop_record(K)
        start = eng.loop_get()["state"]
        preds = []
        for _ in range(K):
            eng.loop_step()
            preds.append(eng.loop_get()["pred"])
        h = eng.loop_history()
        prev = np.concatenate([start[None], h["traj"][:-1, ..., :5]])
        return h, np.stack(preds), prev, eng.loop_disturbance(0, K)

    def defect(h, prev):
        return h["traj"][..., :5] - plant_step(prev, h["traj"][..., 5:7], eng.spec.dt, eng.spec.wb)

    # act
    for scale, clipped in ((1.0, False), (40.0, True)):
        h, pred, prev, d = loop(act=np.asarray(SIG["act"]) * scale)
        want = np.clip(pred[:, :, :, 5:7, 0] + d[..., 5:7], box[:, 0], box[:, 1])
        assert np.array_equal(h["traj"][..., 5:7], want)
        assert (h["traj"][..., 5:7] >= box[:, 0]).all() and (h["traj"][..., 5:7] <= box[:, 1]).all()
        on_bound = int(((h["traj"][..., 5:7] == box[:, 0]) | (h["traj"][..., 5:7] == box[:, 1])).sum())
        print(f"act x {scale:g}: {on_bound} of {want.size} applied inputs on the box; plant defect {np.abs(defect(h, prev)).max():.1e}")
        assert not clipped or on_bound > 0
        assert d[..., 5:7].all() and not d[..., :5].any() and not d[..., 7:].any()
        assert np.abs(defect(h, prev)).max() < 1e-12
    # proc
    h, pred, prev, d = loop(proc=SIG["proc"])
    assert np.array_equal(h["traj"][..., 5:7], pred[:, :, :, 5:7, 0])  # the input is untouched
    worst = float(np.abs(defect(h, prev) - d[..., 7:12]).max())
    print(f"proc: |state - plant - d| <= {worst:.1e}; |d| up to {np.abs(d).max():.3f}")
    assert worst < 1e-12 and np.abs(d[..., 7:11]).min() > 0
    # meas
    h, pred, prev, d = loop(meas=SIG["meas"])
    assert np.abs(defect(h, prev)).max() < 1e-12
    conv = h["status"] == 0
    dev = np.abs(pred[:, :, :, :5, 0] - (prev + d[..., :5]))[conv]
    print(f"meas: {int(conv.sum())} of {conv.size} solves converged; their predictions start within {dev.max():.1e} of the measurement")
    assert conv.mean() > 0.5 and dev.max() <= tol
    assert np.abs(pred[:, :, :, :2, 0] - prev[..., :2])[conv].max() > 1e-3  # ... and not at the true state
    # the setting may change between calls; the step count keeps running
    eng.loop_init(table, k0, noise)
    eng.loop_record(K)
    eng.loop_set_disturbance(SEED, proc=SIG["proc"])
    eng.loop_run(2)
    eng.loop_set_disturbance(SEED + 1, proc=np.asarray(SIG["proc"]) * 2, stream=np.arange(S)[::-1].copy())
    d2 = eng.loop_disturbance(0, K)
    eng.loop_run(K - 2)
    h = eng.loop_history()
    df = defect(h, np.concatenate([h["traj"][:1, ..., :5], h["traj"][:-1, ..., :5]]))
    assert np.abs(df[2:] - d2[2:, ..., 7:12]).max() < 1e-12 and np.abs(df[1] - d2[1, ..., 7:12]).max() > 1e-4


@pytest.mark.parametrize("S,exchange", [(8, "jacobi"), (4, "sequential")])
def test_against_the_host_replay(eng, ospec, S, exchange):
    """(10) S scenarios of the planned table (sample_scenarios(S, table, seed=3, spec)), 10 steps, base sigmas, noise seed 2024, against
    the host replay (oracle/closed_loop.replay) with d downloaded from the device: status and iterations equal solve for solve, states within 1e-6 (the tolerances
    of test_pool_matches_oracle_replay); at least 85 % of the replay's solves converge."""
    from conflict_rez_amd import scenarios
    from oracle.closed_loop import replay

    table, _ = scenarios.load_reference_table(kind="planned")
    k0, noise = scenarios.sample_scenarios(S, table, seed=3, spec=eng.spec)
    steps, V = 10, table.shape[0]
    box = np.asarray(eng.spec.bounds, float).reshape(6, 2)[4:6]  # a, w
    order = _orders(S, V, 5) if exchange == "sequential" else None
    eng.loop_init(table, k0, noise)
    if order is not None:
        eng.loop_set_order(order)
    eng.loop_set_disturbance(SEED, **SIG)
    d = eng.loop_disturbance(0, steps)
    got = stepwise(eng, steps)
    plain = _run(eng, ((table, k0, noise), {}), steps, "step", order, record=False)
    worst, n_conv = against_replay(got, replay(ospec, table, k0, noise, steps, dt=eng.spec.dt, wb=eng.spec.wb, order=order, d=d, box=box))
    moved = float(np.abs(got[-1]["state"] - plain["state"]).max())
    print(f"{exchange}: {n_conv} of {S * V * steps} replayed solves converge; max |state - replay| {worst:.2e}; final states moved by up to "
          f"{moved:.2f} against the undisturbed loop")
    assert worst < 1e-6
    assert n_conv >= 0.85 * S * V * steps
    assert moved > 1e-2


def test_refusals(eng):
    """(11) Refused with a cfz_last_error text, the loop's state and the setting in force unchanged: a call before loop_init, a negative
    or non-finite sigma or level; loop_disturbance with nothing set.  loop_init switches the disturbance off and restarts the count."""
    import ctypes as C

    from conflict_rez_amd import engine

    S, V = 8, eng.spec.n_nbr + 1
    table, k0, noise = _planned(eng, S)
    fresh = engine.Engine(eng.spec, max_batch=S * V)
    with pytest.raises(RuntimeError, match="cfz_loop_init has not been called"):
        fresh.loop_set_disturbance(1, **SIG)
    with pytest.raises(RuntimeError, match="cfz_loop_init has not been called"):
        fresh.loop_disturbance(0, 1)
    fresh.close()
    eng.loop_init(table, k0, noise)
    with pytest.raises(RuntimeError, match="no disturbance is set"):
        eng.loop_disturbance(0, 1)
    eng.loop_set_disturbance(SEED, **SIG)
    eng.loop_run(2)
    before, d = eng.loop_get(), eng.loop_disturbance(0, 4)
    bad_level = np.ones(S); bad_level[3] = -0.5
    nan_level = np.ones(S); nan_level[5] = np.nan
    for kw, text in ((dict(meas=[0.02, -0.02, 0, 0, 0]), "sigma"), (dict(act=[np.nan, 0.0]), "sigma"), (dict(proc=[0, 0, 0, np.inf, 0]), "sigma"),
                     (dict(level=bad_level, **SIG), "level"), (dict(level=nan_level, **SIG), "level")):
        with pytest.raises(RuntimeError, match=text):
            eng.loop_set_disturbance(7, **kw)
    for kw in (dict(meas=[0.1] * 4), dict(level=np.ones(S + 1), **SIG), dict(stream=np.arange(S) - 1, **SIG), dict(stream=np.ones(S), **SIG)):
        with pytest.raises(ValueError):
            eng.loop_set_disturbance(7, **kw)
    neg = (C.c_double * 2)(-1.0, 0.0)
    assert eng.lib.cfz_loop_set_disturbance(eng._h, C.c_uint64(7), None, neg, None, None, None) != 0
    assert b"sigma" in eng.lib.cfz_last_error()
    with pytest.raises(RuntimeError, match="t0"):
        eng.loop_disturbance(-1, 2)
    with pytest.raises(RuntimeError, match="K"):
        eng.loop_disturbance(0, 0)
    after = eng.loop_get()
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    assert np.array_equal(eng.loop_disturbance(0, 4), d)  # the setting in force stayed
    # the loop goes on under it: the same as a run that was never interrupted
    eng.loop_run(2)
    end = eng.loop_get()
    ref = _run(eng, ((table, k0, noise), {}), 4, "run", None, lambda e: e.loop_set_disturbance(SEED, **SIG), record=False)
    _same(ref, end, "after the refusals")
    # loop_init: off, count from 0 (ref ran after a loop_init of its own)
    eng.loop_init(table, k0, noise)
    with pytest.raises(RuntimeError, match="no disturbance is set"):
        eng.loop_disturbance(0, 1)
    eng.loop_run(4)
    plain = eng.loop_get()
    assert not np.array_equal(plain["state"], end["state"])
    _same(plain, _run(eng, ((table, k0, noise), {}), 4, "run", record=False), "loop_init switches the disturbance off")
