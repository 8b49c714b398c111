"""The closed loop over per-scenario plans (cfz_loop_init_tables), the record of the realised trajectory (cfz_loop_record /
cfz_loop_history), its audit (cfz_loop_audit / cfz_audit, csrc/cfz_audit.inl) and the batched planning chain
(scenarios.plan_scenarios) on the GPU."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audit_binding as ab  # noqa: E402
from loop_cases import against_replay, stepwise as _stepwise  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = dict(pos_tol=0.3, psi_tol=0.1, v_tol=0.1)


@pytest.fixture(scope="module")
def eng():
    import __graft_entry__ as g

    g.build()
    from conflict_rez_amd import engine, scenarios

    e = engine.Engine(scenarios.parking_lot_spec(), max_batch=1024)
    yield e
    e.close()


def _hold(table, T):
    """table [V, T0, 7] extended to T samples by repeating its last sample (the loop clamps at T - 1: the same reference)."""
    return np.concatenate([table, np.repeat(table[:, -1:], T - table.shape[1], axis=1)], 1) if T > table.shape[1] else table


def _check_against_numpy(out, traj, goal, obs, g, tol=1e-12):
    """The audit `out` against the numpy statement: first contact and arrivals equal; both minima within `tol`; the reported
    (step, index) is one whose numpy distance is within `tol` of the minimum, and THE one where no other item comes that close (near
    ties are decided by the last bits of sin / cos, which the device and numpy need not share).  Returns the number of near ties."""
    ref = ab.audit(traj, goal, obs, g, **TOL)
    assert np.array_equal(out["first_contact"], ref["first_contact"]) and np.array_equal(out["arrive"], ref["arrive"])
    assert np.abs(out["clear"] - ref["clear"]).max() <= tol
    K, S, V = traj.shape[:3]
    W = ab.body(g, traj[..., 0], traj[..., 1], traj[..., 2])
    pairs = [(u, w) for u in range(V) for w in range(u + 1, V)]
    ties = 0
    for s in range(S):
        Dvv = np.stack([ab.signed_distance(W[:, s, u], W[:, s, w]) for u, w in pairs], 1)  # [K, npair]
        t, u, w = out["where"][s, :3]
        assert abs(Dvv[t, pairs.index((u, w))] - Dvv.min()) <= tol, s
        near = int((Dvv <= Dvv.min() + tol).sum())
        ties += near > 1
        if near == 1:
            assert out["where"][s, :3].tolist() == ref["where"][s, :3].tolist(), s
        if len(obs):
            Dvo = ab.signed_distance(W[:, s, :, None], np.asarray(obs)[None, None])  # [K, V, n_obs]
            t, v, j = out["where"][s, 3:]
            assert abs(Dvo[t, v, j] - Dvo.min()) <= tol, s
            near = int((Dvo <= Dvo.min() + tol).sum())
            ties += near > 1
            if near == 1:
                assert out["where"][s, 3:].tolist() == ref["where"][s, 3:].tolist(), s
    return ties


def _three_tables():
    from conflict_rez_amd import scenarios

    ws, _ = scenarios.load_reference_table(kind="state_ws")
    pl, _ = scenarios.load_reference_table(kind="planned")
    tabs = [ws, pl, pl[:, 20:]]
    T = max(t.shape[1] for t in tabs)
    return tabs, np.stack([_hold(t, T) for t in tabs])


def test_pool_of_one_equals_loop_init(eng):
    """(a) A pool with P = 1 and every scenario on it is cfz_loop_init, bit for bit, stepwise and persistent."""
    from conflict_rez_amd import scenarios

    table, _ = scenarios.load_reference_table(kind="planned")
    k0, noise = scenarios.sample_scenarios(64, table, seed=5)
    for tof in (None, np.zeros(64, np.int32)):
        eng.loop_init(table, k0, noise)
        a = _stepwise(eng, 3)
        eng.loop_init(table[None], k0, noise, table_of=tof if tof is not None else np.zeros(64, np.int32))
        b = _stepwise(eng, 3)
        for x, y in zip(a, b):
            for k in ("state", "pred", "status", "iters"):
                assert np.array_equal(x[k], y[k]), k
        eng.loop_init(table, k0, noise)
        eng.loop_run(4)
        x = eng.loop_get()
        eng.loop_init(table[None], k0, noise, table_of=np.zeros(64, np.int32))
        eng.loop_run(4)
        y = eng.loop_get()
        for k in ("state", "pred", "status", "iters"):
            assert np.array_equal(x[k], y[k]), k


def test_mixed_pool_equals_each_table_alone(eng):
    """(b) Three plan sets (state_ws, planned, planned 20 samples later) mixed over 24 scenarios: every scenario equals the run of its
    own table through cfz_loop_init, bit for bit, persistent and stepwise."""
    from conflict_rez_amd import scenarios

    tabs, pool = _three_tables()
    S = 24
    rng = np.random.default_rng(3)
    tof = rng.integers(0, 3, S).astype(np.int32)
    k0, noise = scenarios.sample_scenarios(S, tabs[2], seed=9, spec=eng.spec)
    K = 6
    eng.loop_init(pool, k0, noise, table_of=tof)
    eng.loop_run(K)
    mixed = eng.loop_get()
    eng.loop_init(pool, k0, noise, table_of=tof)
    mixed_steps = _stepwise(eng, K)[-1]
    for p in range(3):
        sel = np.flatnonzero(tof == p)
        assert len(sel)
        eng.loop_init(tabs[p], k0[sel], noise[sel])
        eng.loop_run(K)
        alone = eng.loop_get()
        for k in ("state", "pred", "status", "iters"):
            assert np.array_equal(mixed[k][sel], alone[k]), (p, k)
            assert np.array_equal(mixed_steps[k][sel], alone[k]), (p, k)
    # the three tables really differ in what they make the vehicles do
    assert not np.array_equal(mixed["state"][tof == 1][:1], mixed["state"][tof == 2][:1])
    # NULL table_of: scenario s follows set s (P == S)
    eng.loop_init(pool, k0[:3], noise[:3])
    eng.loop_run(2)
    a = eng.loop_get()
    eng.loop_init(pool, k0[:3], noise[:3], table_of=np.arange(3, dtype=np.int32))
    eng.loop_run(2)
    b = eng.loop_get()
    assert np.array_equal(a["state"], b["state"])


def test_pool_validation(eng):
    from conflict_rez_amd import scenarios

    _, pool = _three_tables()
    k0, noise = scenarios.sample_scenarios(4, pool[2], seed=1)
    with pytest.raises(RuntimeError, match="table_of"):
        eng.loop_init(pool, k0, noise, table_of=np.array([0, 1, 3, 0], np.int32))
    with pytest.raises(RuntimeError, match="table_of"):
        eng.loop_init(pool, k0, noise, table_of=np.array([0, -1, 2, 0], np.int32))
    with pytest.raises(RuntimeError, match="P == S"):
        eng.loop_init(pool, k0, noise)  # P = 3 != S = 4 without table_of
    with pytest.raises(RuntimeError, match="max_batch"):
        eng.loop_init(pool, np.zeros(257, np.int32), None, table_of=np.zeros(257, np.int32))
    lib = eng.lib
    assert lib.cfz_loop_init_tables(eng._h, 4, 0, pool.shape[2], pool.ctypes.data, None, k0.ctypes.data, None) != 0
    assert b"P >= 1" in lib.cfz_last_error()
    assert lib.cfz_loop_init_tables(eng._h, 4, 3, pool.shape[2], None, np.zeros(4, np.int32).ctypes.data, k0.ctypes.data, None) != 0


def test_pool_matches_oracle_replay(eng, ospec):
    """(c) Six scenarios on three tables x 5 steps against the host replay of the oracle with each scenario's own table: equal status and
    iteration counts, states within 1e-6 (as test_gpu_parity's closed-loop test)."""
    from conflict_rez_amd import scenarios
    from oracle.closed_loop import replay

    tabs, pool = _three_tables()
    S, steps = 6, 5
    tof = np.array([0, 1, 2, 2, 1, 0], np.int32)
    k0, noise = scenarios.sample_scenarios(S, tabs[2], seed=3)
    eng.loop_init(pool, k0, noise, table_of=tof)
    got = _stepwise(eng, steps)
    worst, _ = against_replay(got, replay(ospec, pool, k0, noise, steps, dt=eng.spec.dt, wb=eng.spec.wb, table_of=tof))
    assert worst < 1e-6


def test_record(eng):
    """(d) The record: K x loop_step and loop_run(K) write the same record; its last step is loop_get's state; the plant on the recorded
    inputs reproduces the next recorded state; its status counts are loop_last_status_counts; overflowing it is refused before
    anything runs."""
    from conflict_rez_amd import scenarios
    from oracle.dynamics import plant_step

    table, _ = scenarios.load_reference_table(kind="planned")
    S, K = 32, 7
    k0, noise = scenarios.sample_scenarios(S, table, seed=2024, spec=eng.spec)
    eng.loop_init(table, k0, noise)
    eng.loop_record(K)
    for _ in range(K):
        eng.loop_step()
    a = eng.loop_history()
    last_step = eng.loop_get()
    eng.loop_init(table, k0, noise)
    eng.loop_record(K)
    eng.loop_run(3); eng.loop_run(K - 3)
    b = eng.loop_history()
    g = eng.loop_get()
    counts = eng.loop_last_status_counts()
    for k in ("traj", "status", "iters"):
        assert np.array_equal(a[k], b[k]), k
    assert a["traj"].shape == (K, S, 4, 7)
    assert np.array_equal(b["traj"][-1, ..., :5], g["state"]) and np.array_equal(b["status"][-1], g["status"])
    assert np.array_equal(b["iters"][-1], g["iters"]) and np.array_equal(a["traj"][-1, ..., :5], last_step["state"])
    # the last run covered steps 3..K-1 of the record
    assert np.array_equal(np.bincount(b["status"][3:].ravel(), minlength=6)[:6], counts)
    # a window of the record
    w = eng.loop_history(2, 3)
    assert np.array_equal(w["traj"], b["traj"][2:5])
    # plant: state after step t from state after step t-1 and the inputs applied at step t
    worst = 0.0
    for t in range(1, K):
        for s in range(0, S, 4):
            for v in range(4):
                z = plant_step(b["traj"][t - 1, s, v, :5], b["traj"][t, s, v, 5:7], eng.spec.dt, eng.spec.wb)
                worst = max(worst, float(np.abs(z - b["traj"][t, s, v, :5]).max()))
    assert worst < 1e-12, worst
    # overflow: refused, state untouched; then K = 0 switches recording off and the loop runs on
    with pytest.raises(RuntimeError, match="overflow"):
        eng.loop_run(1)
    with pytest.raises(RuntimeError, match="overflow"):
        eng.loop_step()
    assert np.array_equal(eng.loop_get()["state"], g["state"])
    with pytest.raises(RuntimeError, match="not in the record"):
        eng.loop_history(K - 1, 2)
    eng.loop_record(0)
    eng.loop_run(1)
    with pytest.raises(RuntimeError, match="not in the record"):
        eng.loop_history(0, 1)


def test_audit_of_the_bench_workload(eng):
    """(e) 256 scenarios of the bench sampler x 25 steps of the planned table, recorded by one persistent launch: the device audit equals
    cfz_audit on the host copy and the numpy statement (integers equal, distances within 1e-12); contact between vehicles is found in
    exactly the scenarios where the separating-axis bound of tools/closed_loop_separation.py is negative at some step."""
    import importlib.util

    from conflict_rez_amd import scenarios

    sp_ = importlib.util.spec_from_file_location("closed_loop_separation", os.path.join(ROOT, "tools", "closed_loop_separation.py"))
    cls = importlib.util.module_from_spec(sp_)
    sp_.loader.exec_module(cls)
    table, _ = scenarios.load_reference_table(kind="planned")
    S, K = 256, 25
    k0, noise = scenarios.sample_scenarios(S, table, seed=2024, spec=eng.spec)
    eng.loop_init(table, k0, noise)
    eng.loop_record(K)
    eng.loop_run(K)
    dev = eng.loop_audit(**TOL)
    h = eng.loop_history()
    goal = np.repeat(table[None, :, -1, :3], S, 0)
    host = eng.audit(h["traj"], goal, **TOL)
    spec = eng.spec
    obs = np.stack([ab.obstacle_vertices(spec.A_obs[j], spec.b_obs[j]) for j in range(spec.n_obs)])
    for k in ("where", "first_contact", "arrive", "clear"):
        assert np.array_equal(dev[k], host[k]), k
    _check_against_numpy(dev, h["traj"], goal, obs, spec.g)
    # against the separating-axis bound on the same states
    pol = cls.body_polygons(h["traj"][..., :5])  # [K, S, 4, 4, 2]
    sep = np.full((K, S), np.inf)
    for a in range(4):
        for b in range(a + 1, 4):
            sep = np.minimum(sep, cls.separation(pol[:, :, a].reshape(-1, 4, 2), pol[:, :, b].reshape(-1, 4, 2)).reshape(K, S))
    vv_contact = (sep < 0).any(0)
    assert np.array_equal(dev["clear"][:, 0] < 0, vv_contact)
    assert np.array_equal(dev["first_contact"] >= 0, vv_contact | (dev["clear"][:, 1] < 0))
    assert vv_contact.any()  # the Jacobi exchange lets bodies overlap on this workload (tests/test_determinism_gpu.py)
    fc = dev["first_contact"]
    for s in np.flatnonzero(fc >= 0):  # no contact between vehicles before the first one reported
        assert not (sep[: fc[s], s] < 0).any()
    # deterministic
    again = eng.loop_audit(**TOL)
    for k in dev:
        assert np.array_equal(dev[k], again[k]), k


def test_audit_known_answers(eng):
    """(f) cfz_audit on synthetic records: a head-on approach, a body inside an obstacle from step 3, arrivals at known steps."""
    spec = eng.spec
    obs = np.stack([ab.obstacle_vertices(spec.A_obs[j], spec.b_obs[j]) for j in range(spec.n_obs)])
    K = 9
    traj = np.zeros((K, 3, 2, 7))
    goal = np.zeros((3, 2, 3))
    t = np.arange(K, dtype=float)
    # scenario 0: head-on along y = 17.5 (the lane), fronts 13.4 - 2t apart; overlapping from step 7, by more than the 1.8 m width at 8
    traj[:, 0, 0, :4] = np.stack([5.0 + t, np.full(K, 17.5), np.zeros(K), np.ones(K)], 1)
    traj[:, 0, 1, :4] = np.stack([25.0 - t, np.full(K, 17.5), np.full(K, np.pi), np.ones(K)], 1)
    goal[0] = [[30.0, 17.5, 0.0], [0.0, 17.5, np.pi]]
    # scenario 1: vehicle 1 parked inside obstacle 0 from step 3; vehicle 0 drives down the lane and stops at (12, 17.5) at step 4
    c0 = obs[0].mean(0)
    traj[:, 1, 1, :3] = [15.0, 17.5, 0.0]
    traj[3:, 1, 1, :2] = c0
    traj[:, 1, 0, :4] = np.stack([np.minimum(8.0 + t, 12.0), np.full(K, 17.5), np.zeros(K), np.where(t < 4, 1.0, 0.0)], 1)
    goal[1] = [[12.0, 17.5, 0.0], [0.0, 0.0, 0.0]]
    # scenario 2: two vehicles far apart, both on their goals from step 2 and 5
    traj[:, 2, 0, :3] = [8.0, 16.0, 0.0]; traj[:, 2, 1, :3] = [26.0, 19.0, np.pi]
    traj[:2, 2, 0, 3] = 0.5; traj[:5, 2, 1, 3] = -0.4
    goal[2] = [[8.0, 16.1, 0.0], [26.0, 19.0, -np.pi + 0.01]]
    out = eng.audit(traj, goal, **TOL)
    _check_against_numpy(out, traj, goal, obs, spec.g)
    assert out["first_contact"][0] == 7 and out["where"][0, :3].tolist() == [8, 0, 1]
    assert out["clear"][0, 0] == pytest.approx(-1.8, abs=1e-9)
    assert out["first_contact"][1] == 3 and out["where"][1, 3:].tolist()[1:] == [1, 0] and out["where"][1, 3] >= 3
    assert out["clear"][1, 1] < -0.5
    assert out["arrive"].tolist() == [[-1, -1], [4, -1], [2, 5]]
    assert out["first_contact"][2] == -1 and out["clear"][2, 0] > 10


def _default_followers(fn, hist, offsets):
    from conflict_rez_amd.control.compute_sets import interp_along_sets
    from conflict_rez_amd.control.vehicle_follower import VehicleFollower
    from conflict_rez_amd.pytypes import VehicleState
    from conflict_rez_amd.vehicle_types import VehicleBody

    paths = interp_along_sets(fn, VehicleBody(), 30)
    out = []
    for i, a in enumerate(sorted(hist)):
        off = VehicleState()
        off.x.x, off.x.y, off.e.psi = (float(c) for c in offsets[i])
        out.append(VehicleFollower(rl_file_name=fn, agent=a, color={"front": (1, 0, 0), "back": (0, 1, 0)}, init_offset=off,
                                   final_heading=float(paths[a][-1, 2]), printer=lambda *_: None))
    return out


def test_plan_scenarios(tmp_path):
    """(g) The batched chain: the default strategy with zero offsets is planned_reference_table() exactly; on 4 strategies x 2 start
    offsets every plan equals plan_single_path(strict=True) of that vehicle (or fails where it raises)."""
    from itertools import permutations

    from conflict_rez_amd import scenarios
    from conflict_rez_amd import strategy as strat

    table, lengths, _ = scenarios.planned_reference_table()
    r = scenarios.plan_scenarios([strat.generate_strategy(4)])
    assert r["ok"].all() and (r["ws_status"] == 0).all() and (r["colloc_status"] == 0).all()
    assert np.array_equal(r["tables"][0], table) and np.array_equal(r["lengths"][0], lengths)
    strategies, keys = [], set()
    for order in permutations(range(4)):
        try:
            h = strat.generate_strategy(4, list(order), [0, 0, 0, 0])
        except RuntimeError:
            continue
        k = repr(sorted((a, [sorted(c.items()) for c in h[a]]) for a in h))
        if k not in keys:
            keys.add(k); strategies.append(h)
        if len(strategies) == 4:
            break
    assert len(strategies) == 4
    offs = [np.zeros((4, 3)), np.tile([0.1, -0.05, 0.02], (4, 1))]
    P = [(h, o) for h in strategies for o in offs]
    r = scenarios.plan_scenarios([h for h, _ in P], init_offsets=np.stack([o for _, o in P]))
    assert r["tables"].shape[:2] == (8, 4)
    n_ok = 0
    for p, (h, o) in enumerate(P):
        fn = str(tmp_path / f"s{p}")
        strat.write_strategy(fn, h)
        for i, v in enumerate(_default_followers(fn, h, o)):
            try:
                v.plan_single_path(spline_ws=True, strict=True)
            except RuntimeError:
                assert r["colloc_status"][p, i] != 0 and not r["ok"][p], (p, i)
                continue
            assert r["ws_status"][p, i] == 0 and r["colloc_status"][p, i] == 0, (p, i)
            tt = np.arange(0.0, float(v.reference_traj.t[-1]) + 0.05, 0.1)
            s_ = v.interpolate_states(tt)
            tr = np.stack([s_.x, s_.y, s_.psi, s_.v, s_.u_steer, s_.u_a, s_.u_steer_dot], 1)
            assert r["lengths"][p, i] == len(tr) and np.array_equal(r["tables"][p, i, : len(tr)], tr), (p, i)
            n_ok += 1
    assert n_ok >= 24
