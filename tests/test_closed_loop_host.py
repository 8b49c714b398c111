"""oracle/closed_loop.py without a GPU: `replay`'s options against its plain form, and `replay` against `step_inputs`, the one host
statement of what a solve of the closed loop is fed.  2 scenarios x 3 steps of the planned table, feasible starts."""
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
