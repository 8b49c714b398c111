"""The lossy prediction exchange of the closed loop (`cfz_loop_set_comm`, `cfz_loop_comm`; csrc/cfz_comm.inl) on the GPU.

Message tau of vehicle u is its prediction after iteration tau.  Vehicle v receives it if u1 > p_drop[s] at the Philox draw with counter
(stream[s], v, tau + 1, 8 + u); it plans against the newest message that arrived among the last max_age + 1 it could want (the oldest of
them, or the one history started at, always counts as arrived), advanced by its age (compensate) or as if it were new.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import comm_binding as cb  # noqa: E402
import disturbance_binding as db  # noqa: E402
from loop_cases import against_replay, orders as _orders, planned as _planned, run as _run, same as _same, stepwise  # noqa: E402
from oracle.closed_loop import replay  # noqa: E402

SIG = db.SIGMA
SEED = 2024  # the comm seed of every test; test_against_the_host_replay's conditions were checked with it on the host


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
    """(1) No call, p_drop = 0 everywhere (the comm kernels and the ring run; max_age 1 and 6) and set-then-unset give equal state,
    prediction, status, iterations and record, bit for bit.  S = 64, K = 6."""
    S, K, V = 64, 6, eng.spec.n_nbr + 1
    init = _planned(eng, S)
    order = _orders(S, V, 11) if exchange == "sequential" else None

    def set_unset(e):
        e.loop_set_comm(SEED, 0.5, max_age=2)
        e.loop_set_comm(SEED)
        with pytest.raises(RuntimeError, match="no lossy exchange is set"):
            e.loop_comm(0, 1)

    plain = _run(eng, init, K, how, order)
    assert (plain["rec_status"] == 0).mean() > 0.5
    for max_age in (1, 6):
        def lossless(e):
            e.loop_set_comm(SEED, 0.0, max_age=max_age)
            assert e.loop_comm(0, K).all()

        _same(plain, _run(eng, init, K, how, order, lossless), f"p_drop = 0, max_age {max_age}")
    _same(plain, _run(eng, init, K, how, order, set_unset), "set, then unset")


@pytest.mark.parametrize("exchange", ["jacobi", "sequential"])
@pytest.mark.parametrize("compensate", [False, True])
def test_stepwise_equals_persistent(eng, exchange, compensate):
    """(2) p_drop = 0.3, max_age = 3: K x loop_step, loop_run(K) and loop_run(3); loop_run(K - 3) are equal bit for bit, and once more with
    the base noise sigmas on; the state is not the lossless run's."""
    S, K, V = 64, 6, eng.spec.n_nbr + 1
    init = _planned(eng, S)
    order = _orders(S, V, 11) if exchange == "sequential" else None
    on = lambda e: e.loop_set_comm(SEED, 0.3, max_age=3, compensate=compensate)

    def noisy(e):
        e.loop_set_disturbance(7, **SIG)
        on(e)

    step = _run(eng, init, K, "step", order, on)
    _same(step, _run(eng, init, K, "run", order, on), "one launch")
    _same(step, _run(eng, init, K, (3, K - 3), order, on), "split launch")
    plain = _run(eng, init, K, "run", order)
    moved = np.abs(step["state"] - plain["state"]).reshape(S, -1).max(-1)
    print(f"{exchange}, compensate {compensate}: {int((moved > 0).sum())} of {S} scenarios moved, by up to {moved.max():.3f}; "
          f"{int((step['rec_status'] == 0).sum())} of {step['rec_status'].size} solves converged")
    assert (moved > 0).mean() > 0.5
    if compensate:
        nstep = _run(eng, init, K, "step", order, noisy)
        _same(nstep, _run(eng, init, K, "run", order, noisy), "one launch, noise on")
        _same(nstep, _run(eng, init, K, (3, K - 3), order, noisy), "split launch, noise on")
        assert not np.array_equal(nstep["state"], step["state"])


@pytest.mark.parametrize("exchange,A", [("jacobi", 1), ("jacobi", 3), ("sequential", 3)])
def test_everything_dropped(eng, ospec, exchange, A):
    """(3) p_drop = 1, max_age = A: every age is min(A, iterations since the call) (one more for a vehicle ranked before, whose wanted
    message is this iteration's), and the run, stepwise and persistent, equals the host replay with exactly that age, solve for solve.
    K = 2 A + 3 steps (D = A + 2): every slot of the ring is reused and the history limit binds in the first A iterations."""
    S, V = 2, eng.spec.n_nbr + 1
    K = 2 * A + 3
    table, k0, noise = _planned(eng, S, seed=3)
    order = _orders(S, V, 5) if exchange == "sequential" else None
    fixed = cb.Setting(A, True, -1, age=lambda t, s, v, u, earlier: min(A, cb.want(t, earlier) + 1))
    ref = list(replay(ospec, table, k0, noise, K, dt=eng.spec.dt, wb=eng.spec.wb, order=order, comm=lambda t: fixed))
    lossless = list(replay(ospec, table, k0, noise, K, dt=eng.spec.dt, wb=eng.spec.wb, order=order))
    assert max(float(np.abs(a[0] - b[0]).max()) for a, b in zip(ref, lossless)) > 1e-4  # the ages matter to what is compared below
    # the same ages from the rule over the downloaded bits
    eng.loop_init(table, k0, noise)
    eng.loop_set_comm(SEED, 1.0, max_age=A)
    bits = eng.loop_comm(0, K)
    assert not bits[:, :, ~np.eye(V, dtype=bool)].any()
    ruled = cb.Setting(A, True, -1, bits=bits)
    for t in range(K):
        for earlier in (False, True):
            assert ruled.age_of(t, 0, 0, 1, earlier) == fixed.age_of(t, 0, 0, 1, earlier)
    for how in ("step", "run"):
        eng.loop_init(table, k0, noise)
        if order is not None:
            eng.loop_set_order(order)
        eng.loop_set_comm(SEED, 1.0, max_age=A)
        eng.loop_record(K)
        if how == "step":
            for _ in range(K):
                eng.loop_step()
        else:
            eng.loop_run(K)
        worst, n_conv = against_replay(eng.loop_history(), ref, how)
        print(f"{exchange}, A = {A}, {how}: max |state - replay| {worst:.2e}; {n_conv} of {K * S * V} converge")
        assert worst < 1e-6


def test_export(eng):
    """(4) loop_comm equals the numpy statement exactly and is unchanged by running the loop; it depends on the stream id and not on S: a
    subset of a batch, run alone with `stream=` its ids, equals its rows of the full run bit for bit, persistent and stepwise; a scenario
    with p_drop = 0 inside a lossy batch equals its lossless run bit for bit."""
    S, K, V = 16, 6, eng.spec.n_nbr + 1
    init = _planned(eng, S)
    p = np.array([0.0, 0.3, 0.3, 1.0, 0.5, 0.1, 0.9, 0.3] * 2)
    stream = np.array([5, 5, 6, 7] + [2 ** 32 - 1] + list(range(100, 111)), np.uint32)
    got = {}

    def on(e):
        e.loop_set_comm(SEED, p, max_age=3, stream=stream)
        got["before"] = e.loop_comm(0, K + 3)

    plain = _run(eng, init, K, "run")
    full = {how: _run(eng, init, K, how, None, on) for how in ("run", "step")}
    bits = eng.loop_comm(0, K + 3)
    assert bits.dtype == bool and bits.shape == (K + 3, S, V, V)
    assert np.array_equal(bits, got["before"]) and np.array_equal(bits[2:4], eng.loop_comm(2, 2))
    assert np.array_equal(bits, cb.delivered(SEED, p, stream, V, 0, K + 3))
    assert bits[:, 0].all() and not bits[:, 3][:, ~np.eye(V, dtype=bool)].any()
    _same(full["run"], full["step"], "stepwise against persistent")
    for k, val in full["run"].items():  # scenario 0 loses nothing
        assert np.array_equal(val[:, 0] if k.startswith("rec_") else val[0], plain[k][:, 0] if k.startswith("rec_") else plain[k][0]), k
    assert not np.array_equal(full["run"]["state"][1], plain["state"][1])
    sel = np.array([1, 4, 6, 11, 15])
    sub_init = (init[0], init[1][sel], init[2][sel])
    for how in ("run", "step"):
        sub = _run(eng, sub_init, K, how, None, lambda e: e.loop_set_comm(SEED, p[sel], max_age=3, stream=stream[sel]))
        _same(full[how], sub, how, rows=sel)
        assert np.array_equal(eng.loop_comm(0, K), bits[:K, sel])
    wrong = _run(eng, sub_init, K, "run", None, lambda e: e.loop_set_comm(SEED, p[sel], max_age=3))  # streams 0..4 instead
    assert not np.array_equal(wrong["state"], sub["state"])
    # default stream: s; a scalar rate broadcasts
    eng.loop_set_comm(SEED + 1, 0.4)
    assert np.array_equal(eng.loop_comm(4, 2), cb.delivered(SEED + 1, np.full(len(sel), 0.4), np.arange(len(sel)), V, 4, 2))


@pytest.mark.parametrize("S,exchange,compensate", [(8, "jacobi", True), (4, "sequential", False)])
def test_against_the_host_replay(eng, ospec, S, exchange, compensate):
    """(5) S scenarios of the planned table (sample_scenarios(S, table, seed=3, spec)), 10 steps at p_drop = 0.3, max_age = 3, comm seed
    2024, against the host replay with message history (oracle/closed_loop.replay with comm_binding.Setting) over the bits downloaded by loop_comm: status and iterations
    equal solve for solve, states within 1e-6 (test_disturbance_gpu's tolerance against its replay).  Not vacuous: at least half of the
    replayed solves converge and at least one neighbour read has age >= 2 (with seed 2024 the replay alone gives 315 of 320 converged
    and 64 such reads under Jacobi, 152 of 160 and 31 under the sequential exchange)."""
    from conflict_rez_amd import scenarios

    table, _ = scenarios.load_reference_table(kind="planned")
    k0, noise = scenarios.sample_scenarios(S, table, seed=3, spec=eng.spec)
    steps, V = 10, table.shape[0]
    order = _orders(S, V, 5) if exchange == "sequential" else None
    eng.loop_init(table, k0, noise)
    if order is not None:
        eng.loop_set_order(order)
    eng.loop_set_comm(SEED, 0.3, max_age=3, compensate=compensate)
    setting = cb.Setting(3, compensate, -1, bits=eng.loop_comm(0, steps))
    got = stepwise(eng, steps)
    ages = []
    worst, n_conv = against_replay(got, replay(ospec, table, k0, noise, steps, dt=eng.spec.dt, wb=eng.spec.wb, order=order,
                                               comm=lambda t: setting, ages=ages))
    old = sum(a >= 2 for *_, a in ages)
    print(f"{exchange}: {n_conv} of {S * V * steps} replayed solves converge; {old} of {len(ages)} neighbour reads have age >= 2; "
          f"max |state - replay| {worst:.2e}")
    assert worst < 1e-6
    assert n_conv >= 0.5 * S * V * steps and old >= 1


def test_setting_at_a_step_boundary(eng, ospec):
    """(6) loop_run(2), loop_set_comm, loop_run(3), loop_set_comm with another rate, loop_run(3) equals the host replay whose history
    starts at message 1, and anew at message 4: a changed setting restarts history."""
    S, V = 4, eng.spec.n_nbr + 1
    table, k0, noise = _planned(eng, S, seed=3)
    K, cuts = 8, (2, 5)
    eng.loop_init(table, k0, noise)
    eng.loop_record(K)
    eng.loop_run(cuts[0])
    eng.loop_set_comm(SEED, 0.6, max_age=3, compensate=True)
    first = cb.Setting(3, True, cuts[0] - 1, bits=eng.loop_comm(0, K))
    eng.loop_run(cuts[1] - cuts[0])
    eng.loop_set_comm(SEED, 0.9, max_age=2, compensate=False)
    second = cb.Setting(2, False, cuts[1] - 1, bits=eng.loop_comm(0, K))
    eng.loop_run(K - cuts[1])
    h = eng.loop_history()
    ages = []
    comm = lambda t: None if t < cuts[0] else (first if t < cuts[1] else second)
    worst, _ = against_replay(h, replay(ospec, table, k0, noise, K, dt=eng.spec.dt, wb=eng.spec.wb, comm=comm, ages=ages))
    by_t = {t: max(a for tt, *_, a in ages if tt == t) for t in range(cuts[0], K)}
    print(f"max |state - replay| {worst:.2e}; largest age per iteration {by_t}")
    assert worst < 1e-6
    assert by_t[cuts[0]] == 0 and by_t[cuts[1]] == 0 and by_t[cuts[1] - 1] >= 2 and by_t[K - 1] == 2


def test_refusals(eng):
    """(7) Refused with a cfz_last_error text, the loop's state and the setting in force unchanged: a call before loop_init, a p_drop outside
    [0, 1] or not finite, max_age outside 1..6, compensate other than 0 or 1; shape and dtype errors raise ValueError before the library is
    called.  The loop then goes on as a run that was never interrupted; loop_init switches the setting off."""
    import ctypes as C

    from conflict_rez_amd import engine

    S, V = 8, eng.spec.n_nbr + 1
    table, k0, noise = _planned(eng, S)
    fresh = engine.Engine(eng.spec, max_batch=S * V)
    with pytest.raises(RuntimeError, match="cfz_loop_init has not been called"):
        fresh.loop_set_comm(1, 0.3)
    with pytest.raises(RuntimeError, match="cfz_loop_init has not been called"):
        fresh.loop_comm(0, 1)
    fresh.close()
    eng.loop_init(table, k0, noise)
    with pytest.raises(RuntimeError, match="no lossy exchange is set"):
        eng.loop_comm(0, 1)
    on = lambda e: e.loop_set_comm(SEED, 0.3, max_age=3)
    on(eng)
    eng.loop_run(2)
    before, bits = eng.loop_get(), eng.loop_comm(0, 6)
    high = np.full(S, 0.3); high[3] = 1.5
    neg = np.full(S, 0.3); neg[0] = -0.1
    nan = np.full(S, 0.3); nan[5] = np.nan
    for kw, text in ((dict(p_drop=high), "p_drop"), (dict(p_drop=neg), "p_drop"), (dict(p_drop=nan), "p_drop"), (dict(p_drop=np.inf), "p_drop"),
                     (dict(p_drop=0.5, max_age=0), "max_age"), (dict(p_drop=0.5, max_age=7), "max_age"), (dict(p_drop=0.5, compensate=2), "compensate"),
                     (dict(p_drop=0.5, compensate=-1), "compensate")):
        with pytest.raises(RuntimeError, match=text):
            eng.loop_set_comm(7, **kw)
    for kw in (dict(p_drop=np.full(S + 1, 0.3)), dict(p_drop=np.full((S, 1), 0.3)), dict(p_drop="0.3"), dict(p_drop=0.3, max_age=2.5),
               dict(p_drop=0.3, stream=np.arange(S) - 1), dict(p_drop=0.3, stream=np.ones(S)), dict(p_drop=0.3, stream=np.arange(S + 1))):
        with pytest.raises(ValueError):
            eng.loop_set_comm(7, **kw)
    bad = (C.c_double * S)(*([2.0] * S))
    assert eng.lib.cfz_loop_set_comm(eng._h, C.c_uint64(7), bad, 3, 1, None) != 0
    assert b"p_drop" in eng.lib.cfz_last_error()
    with pytest.raises(RuntimeError, match="tau0"):
        eng.loop_comm(-1, 2)
    with pytest.raises(RuntimeError, match="K"):
        eng.loop_comm(0, 0)
    after = eng.loop_get()
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    assert np.array_equal(eng.loop_comm(0, 6), bits)  # the setting in force stayed
    # the loop goes on under it, history included: the same as a run that was never interrupted
    eng.loop_run(2)
    end = eng.loop_get()
    _same(_run(eng, (table, k0, noise), 4, "run", None, on, record=False), end, "after the refusals")
    # loop_init: off
    eng.loop_init(table, k0, noise)
    with pytest.raises(RuntimeError, match="no lossy exchange is set"):
        eng.loop_comm(0, 1)
    eng.loop_run(4)
    plain = eng.loop_get()
    assert not np.array_equal(plain["state"], end["state"])
    _same(plain, _run(eng, (table, k0, noise), 4, "run", record=False), "loop_init switches the lossy exchange off")
