"""Per-scenario problem constants of the closed loop (`cfz_problem_check`, `cfz_loop_set_problems`) on the GPU, through the C ABI.

With a pool of P problems (cfz_spec, cfz_options) and problem_of[S], every solve of scenario s uses problem problem_of[s]: its dmin, bounds,
weights, options, the constants derived from them and the stage-0 feasibility test; the clip of a disturbed input uses its input box.
Geometry, time base and carry_duals stay the handle's.

The four test problems (tests/problem_pool_binding.py) over the `parking_lot_spec()` handle, planned table, V = 4:
  A the handle's own | B dmin 0.2 | C v in [-1.8, 1.8], a in [-0.8, 0.8], w in [-0.5, 0.5] | D weights (20, 20, 50, 2, 2, 5), max_iter 5
chosen under two conditions:
  (i)  the problem moves the outcome: replayed on the host (oracle/closed_loop.replay with every scenario's own MpcSpec
       and options), every scenario of B, C and D of the batches below ends in other final states than under problem A (checked on the host
       before the first GPU run: the smallest difference is 8e-6 m, scenario 9 of the 16, the others 5e-3 .. 0.5 m; in the batch of 8,
       3.5e-6 m for scenario 1 under B, the others 7e-3 .. 0.5 m);
  (ii) a plain handle created with the problem's constants agrees with the host replay in status and iterations: that is
       test_mixed_batch_equals_separate_handles (plain handles equal the mixed rows bit for bit) together with test_against_the_host_replay.

What every per-scenario pool has is tests/loop_cases.py's, written against `POOL`; here: the numbered statement, that call, what is special.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import disturbance_binding as db  # noqa: E402
import problem_pool_binding as pb  # noqa: E402
import loop_cases as lc  # noqa: E402
from loop_cases import orders as _orders, planned as _planned, run as _run, same as _same  # noqa: E402

SIG = db.SIGMA
SEED = 2024
S16, K6 = 16, 6


def _plain(spec, p, max_batch):
    from conflict_rez_amd import engine

    return engine.Engine(pb.spec_of(p), max_batch=max_batch, **pb.options_of(p))


POOL = lc.Pool(set=lambda e, probs, problem_of: e.loop_set_problems(probs, problem_of), off=lambda e: e.loop_set_problems(None),
               own=lambda e: e.spec, entries=pb.problems, plain=_plain, names=pb.NAMES)


@pytest.fixture(scope="module")
def eng():
    import __graft_entry__ as g

    g.build()
    from conflict_rez_amd import engine, scenarios

    e = engine.Engine(scenarios.parking_lot_spec(), max_batch=S16 * 4)
    yield e
    e.close()


@pytest.fixture(scope="module")
def probs(eng):
    return pb.problems(eng.spec)


@pytest.fixture(scope="module")
def plain_engines(eng, probs):
    """One plain engine per problem, created with that problem's spec and options: the parent's code path."""
    es = [POOL.plain(eng.spec, p, S16 * 4) for p in probs]
    yield es
    for e in es:
        e.close()


@pytest.mark.parametrize("exchange", ["jacobi", "sequential"])
@pytest.mark.parametrize("how", ["step", "run"])
def test_off_is_off(eng, how, exchange):
    """1. No call, P = 1 with the handle's own problem, P = 3 identical copies under a random problem_of, and set-then-unset give equal
    state, prediction, status, iterations and record, bit for bit.  S = 16, K = 6."""
    S, K, V = S16, K6, eng.spec.n_nbr + 1
    order = _orders(S, V, 11) if exchange == "sequential" else None
    plain = lc.off_is_off(POOL, eng, _planned(eng, S), K, how, order)
    assert (plain["rec_status"] == 0).mean() > 0.5


@pytest.mark.parametrize("exchange", ["jacobi", "sequential"])
@pytest.mark.parametrize("how", ["step", "run"])
def test_off_is_off_under_a_lossy_exchange(eng, how, exchange):
    """1, with loop_set_comm(p_drop 0.3) and no disturbance.  The persistent comm kernels without a pool clip the applied input to the
    handle's box under their zero sigma; the pool kernels and the stepwise path clip only while a disturbance is set.  The handle's own
    problem therefore equals no pool as long as every applied input lies inside the handle's box, which holds on the planned table."""
    S, K, V = S16, K6, eng.spec.n_nbr + 1
    init = _planned(eng, S)
    order = _orders(S, V, 11) if exchange == "sequential" else None
    plain = lc.off_is_off(POOL, eng, init, K, how, order, under=lambda e: e.loop_set_comm(SEED + 1, 0.3, max_age=3, compensate=True))
    assert not np.array_equal(plain["state"], _run(eng, init, K, how, order)["state"])  # the loss is felt


@pytest.mark.parametrize("disturbed", [False, True], ids=["exact", "noise+loss"])
@pytest.mark.parametrize("exchange", ["jacobi", "sequential"])
def test_mixed_batch_equals_separate_handles(eng, probs, plain_engines, exchange, disturbed):
    """2. S = 16, problem_of[s] = s % 4, K = 6, stepped, in one launch and in a split launch: the rows of problem p equal, bit for bit, what
    a plain engine created with p's spec and options gives for p's four scenarios alone; once more under noise and a lossy exchange
    (p_drop 0.3) with the sub-batch on the stream ids of its rows.  The rows of B, C and D differ from a plain run of the whole batch."""
    S, K, V = S16, K6, eng.spec.n_nbr + 1
    init = _planned(eng, S)
    pof = np.arange(S) % 4
    order = _orders(S, V, 11) if exchange == "sequential" else None
    settings = lambda stream: lc.noise_and_loss(SIG, stream, SEED) if disturbed else None
    whole = _run(eng, init, K, "run", order, settings(np.arange(S)))
    for how, mixed in lc.mixed_batch_equals_separate_handles(POOL, eng, probs, plain_engines, init, K, order, settings).items():
        for p in range(4):
            sel = np.flatnonzero(pof == p)
            differs = not np.array_equal(mixed["state"][sel], whole["state"][sel])
            assert differs == (p > 0), (how, pb.NAMES[p])
            if p > 0:  # every scenario of the problem, not just one of them
                assert (np.abs(mixed["state"][sel] - whole["state"][sel]).max((1, 2)) > 0).all(), (how, pb.NAMES[p])


@pytest.mark.parametrize("exchange", ["jacobi", "sequential"])
def test_against_the_host_replay(eng, ospec, probs, exchange):
    """3. S = 8, two scenarios per problem, K = 8: the port replayed with every scenario's own MpcSpec and options gives
    equal status and iterations solve for solve and states within 1e-6 (the tolerance of test_pool_matches_oracle_replay and
    test_disturbance_gpu.py::test_against_the_host_replay); at least one solve of problem D ends with status 1.
    problem_of[s] = s % 4, chosen on the host replay alone: every problem then has converged and failed solves among its 64 (status 4 and
    5; status 2 under A; status 1 under D), C 55 converged.  With problem_of[s] = s // 2 both starts
    of C are faster than C's speed box allows and none of its 64 solves converges, which compares statuses and fallbacks only."""
    from oracle.closed_loop import replay

    S, K, V = 8, 8, eng.spec.n_nbr + 1
    table, k0, noise = _planned(eng, S)
    pof = np.arange(S) % 4
    order = _orders(S, V, 5) if exchange == "sequential" else None
    eng.loop_init(table, k0, noise)
    if order is not None:
        eng.loop_set_order(order)
    eng.loop_set_problems(probs, pof)
    got = lc.stepwise(eng, K)
    osp, opt = zip(*(pb.oracle_problem(ospec, probs[p]) for p in pof))
    worst, _ = lc.against_replay(got, replay(osp, table, k0, noise, K, dt=eng.spec.dt, wb=eng.spec.wb, opt=opt, order=order))
    status = np.stack([g["status"] for g in got])
    conv = {pb.NAMES[p]: float((status[:, pof == p] == 0).mean()) for p in range(4)}
    print(f"{exchange}: max |state - replay| {worst:.2e}; converged share per problem {conv}; "
          f"problem D: {int((status[:, pof == 3] == 1).sum())} solves at the iteration limit")
    assert worst < 1e-6
    assert (status[:, pof == 3] == 1).any()


@pytest.mark.parametrize("exchange", ["jacobi", "sequential"])
def test_mapping_changes_between_calls(eng, probs, exchange):
    """4. loop_run(3), another problem_of, loop_run(3) equals the same sequence stepped, bit for bit; the change matters."""
    S, K, V = S16, K6, eng.spec.n_nbr + 1
    order = _orders(S, V, 11) if exchange == "sequential" else None
    lc.mapping_changes_between_calls(POOL, eng, probs, _planned(eng, S), K, order)


@pytest.mark.parametrize("how", ["step", "run"])
def test_disturbed_input_is_clipped_to_the_scenarios_box(eng, probs, how):
    """5. Problems A and C alternate under actuator noise of 40 x the base sigma: the recorded inputs of C's scenarios stay inside C's
    input box and reach its edge; those of A's scenarios stay inside A's box and exceed C's somewhere."""
    S, K = S16, K6
    init = _planned(eng, S)
    pof = np.arange(S) % 2
    pool = [probs[0], probs[2]]
    box = [np.asarray(pb.spec_of(p).bounds, float).reshape(6, 2)[4:6] for p in pool]  # (a, w) x (lo, hi)

    def setup(e):
        e.loop_set_disturbance(SEED, act=np.asarray(SIG["act"]) * 40)
        e.loop_set_problems(pool, pof)

    u = _run(eng, init, K, how, None, setup)["rec_traj"][..., 5:7]
    for p in (0, 1):
        up = u[:, pof == p]
        assert (up >= box[p][:, 0]).all() and (up <= box[p][:, 1]).all(), p
        assert ((up == box[p][:, 0]) | (up == box[p][:, 1])).any(), p
    ua = u[:, pof == 0]
    assert ((ua < box[1][:, 0]) | (ua > box[1][:, 1])).any()


def test_audit_and_record_under_a_pool(eng, probs, plain_engines):
    """6. loop_audit() equals audit(loop_history(), goals) under a pool; the audit of that record does not depend on the pool's dmin (it
    measures signed distance, not the constraint): the same after the pool is changed to all-B, and from an engine created with dmin 0.2."""
    S, K = S16, K6
    table, k0, noise = _planned(eng, S)
    _run(eng, (table, k0, noise), K, "run", None, lambda e: e.loop_set_problems(probs, np.arange(S) % 4))
    traj = eng.loop_history()["traj"]
    goals = lc.goals(table, S)
    a = eng.loop_audit()
    _same(a, eng.audit(traj, goals), "loop_audit against audit of the history")
    eng.loop_set_problems([probs[1]], np.zeros(S, int))
    _same(a, eng.loop_audit(), "after the pool changed")
    _same(a, plain_engines[1].audit(traj, goals), "from an engine created with dmin 0.2")
    assert np.isfinite(a["clear"]).all()


def test_refusals(eng, probs):
    """7. Refused with a cfz_last_error text, the loop's state and the setting in force unchanged: a call before loop_init, P < 0,
    problem_of out of range, an entry differing in N, n_obs, an obstacle row, g, dt, wb or carry_duals, a box with lo > hi.  loop_init
    switches the pool off."""
    import ctypes as C
    import dataclasses

    from conflict_rez_amd import engine

    S, K = S16, 4
    init = _planned(eng, S)
    pof = np.arange(S) % 4
    sp = eng.spec
    fresh = engine.Engine(sp, max_batch=4)
    with pytest.raises(RuntimeError, match="cfz_loop_init has not been called"):
        fresh.loop_set_problems(probs, pof)
    fresh.close()
    _, specs, opts = engine.pack_problems(probs)

    def refused(eng):
        assert eng.lib.cfz_loop_set_problems(eng._h, -1, specs, opts, pof.astype(np.int32).ctypes.data_as(C.c_void_p)) != 0
        assert b"P must not be negative" in eng.lib.cfz_last_error()
        for bad in (np.where(pof == 3, 4, pof), np.where(pof == 0, -1, pof)):
            with pytest.raises(RuntimeError, match="problem_of"):
                eng.loop_set_problems(probs, bad)
        A2, b2, g2 = np.array(sp.A_obs), np.array(sp.b_obs), np.array(sp.g)
        b2[2, 1] += 0.25
        g2[0] += 0.1
        lo_hi = np.array(sp.bounds, float); lo_hi[8], lo_hi[9] = 0.5, -0.5
        for entry, text in ((dataclasses.replace(sp, N=sp.N - 2), " N"), (dataclasses.replace(sp, A_obs=A2[:5], b_obs=np.array(sp.b_obs)[:5]), "n_obs"),
                            (dataclasses.replace(sp, b_obs=b2), r"b_obs\[2\]"), (dataclasses.replace(sp, g=g2), " g"),
                            (dataclasses.replace(sp, dt=0.2), " dt"), (dataclasses.replace(sp, wb=2.6), " wb"), ((sp, dict(carry_duals=0)), "carry_duals"),
                            (dataclasses.replace(sp, bounds=lo_hi), "lo > hi")):
            with pytest.raises(RuntimeError, match="problem 1: .*" + text):
                eng.loop_set_problems([sp, entry], np.zeros(S, int))

    lc.refusals_change_nothing(POOL, eng, probs, init, K, refused, rest=(K - 2,))
