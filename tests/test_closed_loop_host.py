"""oracle/closed_loop.py without a GPU: `replay`'s options against its plain form, and `replay` against `step_inputs`, the one host
statement of what a solve of the closed loop is fed (2 scenarios x 3 steps of the planned table, feasible starts); and `replay` with one
problem per scenario against the one-scenario replays (3 scenarios on the test maps and problems of the pool modules)."""
import numpy as np
import pytest

from oracle import closed_loop, port

S, STEPS = 2, 3


@pytest.fixture(scope="module")
def case():
    from conflict_rez_amd import scenarios
    from oracle.mpc_nlp import MpcSpec

    spec = scenarios.parking_lot_spec()
    table, _ = scenarios.load_reference_table(kind="planned")
    ospec = MpcSpec(N=spec.N, dt=spec.dt, A_obs=spec.A_obs, b_obs=spec.b_obs, n_nbr=spec.n_nbr)
    k0, noise = scenarios.sample_scenarios(S, table, seed=0, spec=spec)
    box = np.asarray(spec.bounds, float).reshape(6, 2)[4:6]  # a, w
    return spec, ospec, table, k0, noise, box


def test_zero_disturbance_is_the_plain_replay(case):
    """replay(order=None, d=None) and replay(d=zeros) yield equal state, prediction, status and iterations, bit for bit: the three
    injections and the clip to the input box are on the second run's path and change nothing."""
    spec, ospec, table, k0, noise, box = case
    V = table.shape[0]
    plain = list(closed_loop.replay(ospec, table, k0, noise, STEPS, dt=spec.dt, wb=spec.wb, order=None, d=None))
    zeros = list(closed_loop.replay(ospec, table, k0, noise, STEPS, dt=spec.dt, wb=spec.wb, d=np.zeros((STEPS, S, V, 12)), box=box))
    assert len(plain) == len(zeros) == STEPS
    for t, (a, b) in enumerate(zip(plain, zeros)):
        for name, x, y in zip(("state", "pred", "status", "iters"), a, b):
            assert np.array_equal(x, y), (t, name)
    assert (plain[-1][2] == 0).any()


def test_replay_feeds_every_solve_what_step_inputs_returns(case, monkeypatch):
    """Under an order, every call of `port.solve` receives exactly `step_inputs` of the state and predictions before the step, this
    step's predictions so far and the vehicles ranked before it (the calls are recorded as test_sequential_exchange_host._record_solves
    records the stand-in's)."""
    spec, ospec, table, k0, noise, _ = case
    V, N = table.shape[0], ospec.N
    order = np.array([[2, 0, 3, 1], [3, 2, 1, 0]])
    calls = []
    orig = port.solve

    def solve(osp, x0, ref, nbr, zu, **kw):
        calls.append(dict(x0=np.array(x0), ref=np.array(ref), nbr=np.array(nbr), zu=np.array(zu), carry=kw.get("carry")))
        return orig(osp, x0, ref, nbr, zu, **kw)

    monkeypatch.setattr(port, "solve", solve)
    state, pred = closed_loop.seed(table, k0, noise, N)
    n_unshifted = 0
    for t, (state1, pred1, status, _) in enumerate(closed_loop.replay(ospec, table, k0, noise, STEPS, dt=spec.dt, wb=spec.wb, order=order)):
        assert len(calls) == (t + 1) * S * V
        for s in range(S):
            for r, v in enumerate(order[s]):
                c = calls[(t * S + s) * V + r]
                x0, ref, nbr, warm = closed_loop.step_inputs(table, k0[s] + t, state[s], pred[s], v, pred1[s], order[s][:r])
                assert np.array_equal(c["x0"], x0) and np.array_equal(c["ref"], ref), (t, s, v)
                assert np.array_equal(c["nbr"], nbr) and np.array_equal(c["zu"], warm.T), (t, s, v)
                assert (c["carry"] is None) == (t == 0), (t, s, v)
                # the rule itself, spelled out once more: ranks before v as they stand after the step, the others shifted
                others = [u for u in range(V) if u != v]
                adv = np.minimum(np.arange(N) + 1, N - 1)
                want = np.stack([pred1[s, u, :3] if u in order[s][:r] else pred[s, u, :3][:, adv] for u in others])
                assert np.array_equal(nbr, want), (t, s, v)
                n_unshifted += sum(u in order[s][:r] for u in others)
        state, pred = state1, pred1
    assert n_unshifted == STEPS * S * V * (V - 1) // 2



def _pool_case(case, which):
    """(table, k0, noise, specs, options) of three scenarios (seed 2024) of the planned table on the maps [A, B, D] of map_pool_binding or
    the problems [A, D, B] of problem_pool_binding; specs[0] is the handle's own."""
    import map_pool_binding as mb
    import problem_pool_binding as pb
    from conflict_rez_amd import scenarios

    spec, ospec, table = case[:3]
    k0, noise = scenarios.sample_scenarios(3, table, seed=2024, spec=spec)
    if which == "maps":
        return table, k0, noise, [mb.oracle_spec(ospec, mb.maps(spec)[m]) for m in (0, 1, 3)], [None] * 3
    specs, opts = zip(*(pb.oracle_problem(ospec, pb.problems(spec)[p]) for p in (0, 3, 1)))
    return table, k0, noise, specs, opts


def _same_bits(a, b, what, s=None):
    """The replays a and b are equal bit for bit at every step; s: scenario s of a against b, a replay of that scenario alone."""
    assert len(a) == len(b) == STEPS
    for t, (x, y) in enumerate(zip(a, b)):
        for name, p, q in zip(("state", "pred", "status", "iters"), x, y):
            assert np.array_equal(p if s is None else p[s : s + 1], q), (what, s, t, name)


@pytest.mark.parametrize("exchange", ["jacobi", "sequential"])
@pytest.mark.parametrize("which", ["maps", "problems"])
def test_per_scenario_problems_are_the_separate_replays(case, which, exchange):
    """replay with one MpcSpec (and IpmOptions) per scenario equals, bit for bit in state, prediction, status and iterations, the three
    one-scenario replays with those specs, under Jacobi and under a sequential order.  Not vacuous: scenarios 1 and 2 end in other
    states than under the handle's own problem, scenario 0 (on it) does not."""
    table, k0, noise, specs, opts = _pool_case(case, which)
    order = np.array([[2, 0, 3, 1], [3, 2, 1, 0], [1, 3, 0, 2]]) if exchange == "sequential" else None
    kw = dict(dt=case[0].dt, wb=case[0].wb)
    joint = list(closed_loop.replay(specs, table, k0, noise, STEPS, opt=opts, order=order, **kw))
    for s in range(3):
        one = slice(s, s + 1)
        _same_bits(joint, list(closed_loop.replay(specs[s], table, k0[one], noise[one], STEPS, opt=opts[s], order=None if order is None else order[one], **kw)), which, s)
    under_a = list(closed_loop.replay(specs[0], table, k0, noise, STEPS, opt=opts[0], order=order, **kw))
    assert [not np.array_equal(joint[-1][0][s], under_a[-1][0][s]) for s in range(3)] == [False, True, True]


def test_one_problem_is_the_same_problem_for_every_scenario(case):
    """A single MpcSpec and the same spec repeated per scenario give equal bits; a wrong count and specs that differ in N are refused."""
    import dataclasses

    ospec = case[1]
    table, k0, noise, _, _ = _pool_case(case, "maps")
    kw = dict(dt=case[0].dt, wb=case[0].wb)
    one = list(closed_loop.replay(ospec, table, k0, noise, STEPS, **kw))
    _same_bits(one, list(closed_loop.replay([ospec] * 3, table, k0, noise, STEPS, opt=[None] * 3, **kw)), "the spec three times")
    for bad in ([ospec, dataclasses.replace(ospec, N=ospec.N - 2), ospec], [ospec] * 2):
        with pytest.raises(ValueError, match="N and n_nbr"):
            next(closed_loop.replay(bad, table, k0, noise, STEPS, **kw))
