"""The sequential exchange on the reference surface (`VehicleFollower.prepare_step(current=...)`,
`MultiDistributedFollower.solve(order=...)`) without a GPU: the C port behind the `OracleEngine` stand-in of test_follower_host."""
import numpy as np
import pytest

from conflict_rez_amd import strategy as strat
from conflict_rez_amd.control.vehicle_follower import MultiDistributedFollower
from conflict_rez_amd.pytypes import VehicleState
from test_follower_host import OracleEngine, _references, follower_setup  # noqa: F401  (follower_setup: the fixture)

import audit_binding as ab

NAMES = [f"vehicle_{i}" for i in range(4)]


def _setup(path, monkeypatch):
    import conflict_rez_amd.control.vehicle_follower as vf

    strat.write_strategy(path, strat.generate_strategy(4))
    mdf = MultiDistributedFollower(path, {a: True for a in NAMES}, {a: {"front": (1, 0, 0), "back": (0, 1, 0)} for a in NAMES},
                                   {a: VehicleState() for a in NAMES}, {a: None for a in NAMES})
    monkeypatch.setattr(vf, "Engine", lambda spec, max_batch, **kw: OracleEngine(spec))
    mdf.setup_multi_vehicles(references=_references())
    return mdf


def _xyp(p):
    return np.stack([np.asarray(p.x), np.asarray(p.y), np.asarray(p.psi)])


def _record_solves(mdf):
    """Wraps the stand-in's solve: per call (slot, carry, nbr, every vehicle's prediction (x, y, psi) at the time of the call)."""
    calls = []
    orig = mdf.engine.solve

    def solve(x0, ref, nbr, zu, want_duals=True, carry=None, slots=None):
        calls.append(dict(B=len(x0), slots=None if slots is None else list(slots), carry=None if carry is None else list(carry),
                          nbr=np.array(nbr), preds={v.agent: _xyp(v.pred) for v in mdf.vehicles}))
        return orig(x0, ref, nbr, zu, want_duals=want_duals, carry=carry, slots=slots)

    mdf.engine.solve = solve
    return calls


def test_prepare_step_current_rows_unshifted(follower_setup):
    mdf = follower_setup
    mdf.solve(num_iter=2, dump=False)  # predictions that are no longer the plan
    v = mdf.vehicles[1]
    v.get_others_pred(mdf.vehicles)
    _, _, nbr_all, zu_all = v.prepare_step()
    _, _, nbr, zu = v.prepare_step(current=("vehicle_2",))
    assert v.others == ["vehicle_0", "vehicle_2", "vehicle_3"]
    for o, other in enumerate(v.others):
        p = v.others_pred[other]
        adv = np.stack([v._adv_onestep(p.x), v._adv_onestep(p.y), v._adv_onestep(p.psi)])
        want = _xyp(p) if other == "vehicle_2" else adv
        assert np.array_equal(nbr[o], want), other
        assert np.array_equal(nbr_all[o], adv), other
    assert not np.array_equal(nbr[1], nbr_all[1])
    assert np.array_equal(zu, zu_all)  # the warm start is the vehicle's own prediction, advanced, either way


def test_sequential_solve_call_pattern_and_inputs(follower_setup):
    """One solve per vehicle per iteration, in the given order, each a batch of one in the vehicle's own slot; every nbr the
    stand-in receives is the rule's, rebuilt from the followers' predictions at the time of the call."""
    mdf = follower_setup
    order = ["vehicle_2", "vehicle_0", "vehicle_3", "vehicle_1"]
    calls = _record_solves(mdf)
    n_iter = 3
    mdf.solve(num_iter=n_iter, dump=False, order=order)
    slot = {v.agent: v.slot for v in mdf.vehicles}
    assert len(calls) == 4 * n_iter
    for i, c in enumerate(calls):
        a = order[i % 4]
        assert c["B"] == 1 and c["slots"] == [slot[a]] and c["carry"] == [int(i >= 4)]
        earlier = order[: i % 4]
        others = [o for o in NAMES if o != a]
        adv = np.minimum(np.arange(30) + 1, 29)
        want = np.stack([c["preds"][o] if o in earlier else c["preds"][o][:, adv] for o in others])
        assert np.array_equal(c["nbr"][0], want), (i, a)
    with pytest.raises(ValueError):
        mdf.solve(num_iter=1, dump=False, order=["vehicle_0", "vehicle_1", "vehicle_2"])


def test_order_none_is_the_jacobi_loop(tmp_path, monkeypatch):
    a = _setup(str(tmp_path / "a"), monkeypatch)
    b = _setup(str(tmp_path / "b"), monkeypatch)
    ca, cb = _record_solves(a), _record_solves(b)
    a.solve(num_iter=5, dump=False)
    b.solve(num_iter=5, dump=False, order=None)
    assert len(ca) == len(cb) == 5 and all(c["B"] == 4 for c in ca + cb)
    for va, vb in zip(a.vehicles, b.vehicles):
        assert va.status == vb.status and va.back_up_steps == vb.back_up_steps
        for key in ("x", "y", "psi", "v", "u_a", "u_steer_dot"):
            assert np.array_equal(getattr(va.final_traj, key), getattr(vb.final_traj, key)), key
    assert [c["nbr"].tolist() for c in ca] == [c["nbr"].tolist() for c in cb]
    assert a.engine.calls == b.engine.calls and a.engine.carried == b.engine.carried


def test_clearance_against_earlier_ranks(follower_setup):
    """4 vehicles, 20 iterations in the strategy's planning priority: every converged solve's prediction keeps dmin - constr_viol_tol
    (less the working set's 1 mm hysteresis) from the predictions of the vehicles stepped before it, at stages 1..N-1."""
    mdf = follower_setup
    order = [NAMES[i] for i in strat.DEFAULT_ORDER]
    log = []
    for v in mdf.vehicles:
        def wrapped(out, b=0, solve_time=None, _v=v, _orig=v.finish_step):
            _orig(out, b, solve_time=solve_time)
            log.append((_v.agent, _v.status, _xyp(_v.pred)))
        v.finish_step = wrapped
    n_iter = 20
    mdf.solve(num_iter=n_iter, dump=False, order=order)
    spec = mdf.vehicles[0].spec
    thr = spec.dmin - 1e-2 - 1e-3  # constr_viol_tol of the default options
    n = 0
    for i in range(n_iter):
        it = log[4 * i: 4 * i + 4]
        assert [a for a, _, _ in it] == order
        for r, (a, st, p) in enumerate(it):
            if st != 0:
                continue
            for _, _, q in it[:r]:
                d = ab.signed_distance(ab.body(spec.g, p[0, 1:], p[1, 1:], p[2, 1:]), ab.body(spec.g, q[0, 1:], q[1, 1:], q[2, 1:]))
                assert d.min() >= thr, (i, a, r, float(d.min()))
                n += 1
    assert n >= 6 * n_iter * 3 // 4
