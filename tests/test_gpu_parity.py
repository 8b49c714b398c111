"""GPU parity tests (`pytest -m gpu`): the HIP path, called through the C ABI, against the oracle.

Tolerances (fp64 everywhere): the kernel and the oracle run the same algorithm, so trajectories
agree to rounding (1e-7 absolute allows for different summation order and libm sin/cos); against
the reference's CasADi/IPOPT solutions the claim is the one its own stopping rule supports
(tol = constr_viol_tol = 1e-2, vehicle_follower.py:362-363): 5e-2 m, 5e-2 rad, 1e-1 in inputs --
unpinned, see DESIGN.md.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-7  # states x, y, psi, v, delta
TOL_U = 1e-5  # inputs a, w: w is almost undetermined where v ~ 0 ((v w)^2 is its only cost), rounding shows there


@pytest.fixture(scope="module")
def eng():
    from conflict_rez_amd import engine, scenarios

    e = engine.Engine(scenarios.parking_lot_spec(), max_batch=4096)
    yield e
    e.close()


def test_golden_vectors(eng, golden):
    """Committed fixtures: inputs + full-KKT numpy oracle solutions (tests/golden/make_fixtures.py)."""
    out = eng.solve(golden["x0"], golden["ref"], golden["nbr"], golden["zu"])
    meta = golden["meta"]
    assert out["status"].tolist() == meta[:, 0].astype(int).tolist()
    ok = out["status"] == 0
    assert out["iters"][ok].tolist() == meta[ok, 1].astype(int).tolist()
    assert np.abs(out["zu"][ok][:, :5] - golden["sol"][ok][:, :5]).max() < TOL
    assert np.abs(out["zu"][ok][:, 5:] - golden["sol"][ok][:, 5:]).max() < TOL_U
    assert np.allclose(out["cost"][ok], meta[ok, 2], rtol=1e-9, atol=1e-9)
    assert np.allclose(out["min_sep"][ok], meta[ok, 3], atol=1e-7)
    assert (out["status"] == 4).sum() == (meta[:, 0] == 4).sum() >= 1  # the infeasible-x0 fixture is detected


def test_matches_c_port_on_seeded_batch(eng, ospec):
    from conflict_rez_amd import scenarios
    from oracle import port

    table, _ = scenarios.load_reference_table()
    k0, noise = scenarios.sample_scenarios(16, table, seed=11)
    x0, ref, nbr, zu = scenarios.mpc_batch_from_table(eng.spec, table, k0, noise)
    out = eng.solve(x0, ref, nbr, zu)
    n_ok = 0
    for b in range(len(x0)):
        r = port.solve(ospec, x0[b], ref[b], nbr[b], zu[b].T)
        assert r["status"] == out["status"][b]
        if r["status"] == 0:
            n_ok += 1
            assert r["iters"] == out["iters"][b]
            assert np.abs(r["p"].T[:5] - out["zu"][b][:5]).max() < TOL
            assert np.abs(r["p"].T[5:] - out["zu"][b][5:]).max() < TOL_U
    assert n_ok >= len(x0) // 2


def test_duals_certify_reference_constraints(eng, ospec):
    """Returned l, m, lambda_ij, lambda_ji, s satisfy the reference's own constraint rows."""
    from conflict_rez_amd import scenarios
    from oracle.mpc_nlp import reference_residuals

    table, _ = scenarios.load_reference_table()
    k0, noise = scenarios.sample_scenarios(4, table, seed=5)
    x0, ref, nbr, zu = scenarios.mpc_batch_from_table(eng.spec, table, k0, noise)
    out = eng.solve(x0, ref, nbr, zu)
    checked = 0
    for b in np.flatnonzero(out["status"] == 0):
        z = out["zu"][b]
        sol = dict(x=z[0], y=z[1], psi=z[2], v=z[3], delta=z[4], a=z[5], w=z[6], l=out["l"][b], m=out["m"][b],
                   lam_ij=out["lam_ij"][b], lam_ji=out["lam_ji"][b], s=out["s"][b])
        r = reference_residuals(ospec, x0[b], ref[b], nbr[b], sol)
        assert r["eq"] < 1e-2 and r["ineq"] < 1e-2 and r["bound"] < 1e-9, r
        assert abs(r["cost"] - out["cost"][b]) < 1e-8 * max(1.0, r["cost"])
        checked += 1
    assert checked > 0


def test_full_batch_properties(eng):
    """B = 1024 scenarios x 4 vehicles (BASELINE.json config 3): size-independent properties."""
    from conflict_rez_amd import scenarios

    table, _ = scenarios.load_reference_table()
    k0, noise = scenarios.sample_scenarios(1024, table, seed=2024)
    x0, ref, nbr, zu = scenarios.mpc_batch_from_table(eng.spec, table, k0, noise)
    out = eng.solve(x0, ref, nbr, zu, want_duals=False)
    ok = out["status"] == 0
    assert ok.mean() > 0.8, ok.mean()
    assert set(np.unique(out["status"])) <= {0, 1, 2, 4, 5}
    z = out["zu"][ok]
    assert np.abs(z[:, :5, 0] - x0[ok]).max() < 1e-2  # initial-state row
    assert out["min_sep"][ok].min() > 0.05 - 1e-2  # every block separated by dmin (to constr_viol_tol)
    b = eng.spec.bounds
    for col, j in ((0, 0), (1, 1), (3, 2), (4, 3), (5, 4), (6, 5)):
        assert z[:, col].min() >= b[2 * j] - 1e-9 and z[:, col].max() <= b[2 * j + 1] + 1e-9
    # permutation invariance: instances are independent
    perm = np.random.default_rng(0).permutation(len(x0))[:256]
    out2 = eng.solve(x0[perm], ref[perm], nbr[perm], zu[perm], want_duals=False)
    assert np.array_equal(out2["status"], out["status"][perm])
    assert np.array_equal(out2["zu"], out["zu"][perm])


def test_order_of_neighbours_and_obstacles_does_not_matter(eng):
    """Two more size-independent properties at the full batch (1024 scenarios x 4 vehicles, planned table): the NLP does not know an
    order of its neighbours or of its obstacles (the reference loops over `self.others` / the obstacle list and adds one block of rows
    each, vehicle_follower.py:280-352), so listing them in another order must give the same trajectory.  The kernel assigns blocks to
    lanes by their index, so the sums run in another order: outcomes equal on all but a handful of instances (a solve on the edge of
    its stopping rule may take one iteration more), trajectories of the rest to rounding (median below 1e-10, 99 % below 1e-6)."""
    import dataclasses

    from conflict_rez_amd import engine, scenarios

    table, _ = scenarios.load_reference_table(kind="planned")
    k0, noise = scenarios.sample_scenarios(1024, table, seed=2024, spec=eng.spec)
    x0, ref, nbr, zu = scenarios.mpc_batch_from_table(eng.spec, table, k0, noise)
    base = eng.solve(x0, ref, nbr, zu, want_duals=False)
    # neighbours in reverse order
    a = eng.solve(x0, ref, np.ascontiguousarray(nbr[:, ::-1]), zu, want_duals=False)
    # obstacles in another order (a second engine: the obstacle list is part of the spec)
    perm = [3, 0, 5, 1, 4, 2]
    sp2 = dataclasses.replace(eng.spec, A_obs=eng.spec.A_obs[perm], b_obs=eng.spec.b_obs[perm])
    e2 = engine.Engine(sp2, max_batch=len(x0))
    b = e2.solve(x0, ref, nbr, zu, want_duals=False)
    e2.close()
    for name, o in (("neighbours", a), ("obstacles", b)):
        same = (o["status"] == base["status"]) & (o["iters"] == base["iters"])
        assert same.mean() > 0.99, (name, same.mean())
        ok = same & (base["status"] == 0)
        dz = np.abs(o["zu"][ok] - base["zu"][ok]).reshape(int(ok.sum()), -1).max(1)
        # (long solves amplify the rounding of the re-ordered sums: 2.7e-5 measured on the worst of 3,600 instances)
        assert dz.max() < 1e-3 and np.quantile(dz, 0.99) < 1e-6 and np.median(dz) < 1e-10, (name, dz.max(), np.quantile(dz, 0.99), np.median(dz))
        assert abs(int((o["status"] == 0).sum()) - int((base["status"] == 0).sum())) <= 4, name


def test_mirror_symmetry(eng):
    """A third size-independent property at the full batch: the parking lot's NLP is symmetric under the reflection y -> 35 - y
    (the y bounds [7.5, 27.5] are symmetric about 17.5, the body about its axis): mirror the obstacles (A diag(1, -1), b - 35 A_y),
    the state, the reference, the neighbours and the warm start (psi, delta, w change sign), solve, mirror back -- the same
    trajectory.  Every sign in the geometry code (face normals, vertex order, the vertex-vertex cones, dw = d(R b)/dpsi) is on this
    path twice."""
    import dataclasses

    from conflict_rez_amd import engine, scenarios

    table, _ = scenarios.load_reference_table(kind="planned")
    k0, noise = scenarios.sample_scenarios(1024, table, seed=2024, spec=eng.spec)
    x0, ref, nbr, zu = scenarios.mpc_batch_from_table(eng.spec, table, k0, noise)
    base = eng.solve(x0, ref, nbr, zu, want_duals=False)

    def mir_pose(a, axis):  # rows (x, y, psi, ...) along `axis`
        a = np.array(a, float)
        idx = [slice(None)] * a.ndim
        idx[axis] = 1; a[tuple(idx)] = 35.0 - a[tuple(idx)]
        idx[axis] = 2; a[tuple(idx)] = -a[tuple(idx)]
        return a

    x0m = mir_pose(x0, 1); x0m[:, 4] = -x0m[:, 4]
    zum = mir_pose(zu, 1); zum[:, 4] = -zum[:, 4]; zum[:, 6] = -zum[:, 6]
    A, b = eng.spec.A_obs, eng.spec.b_obs
    spm = dataclasses.replace(eng.spec, A_obs=A * np.array([1.0, -1.0]), b_obs=b - 35.0 * A[:, :, 1])
    em = engine.Engine(spm, max_batch=len(x0))
    out = em.solve(x0m, mir_pose(ref, 1), mir_pose(nbr, 2), zum, want_duals=False)
    em.close()
    back = mir_pose(out["zu"], 1); back[:, 4] = -back[:, 4]; back[:, 6] = -back[:, 6]
    same = (out["status"] == base["status"]) & (out["iters"] == base["iters"])
    assert same.mean() > 0.99, same.mean()
    ok = same & (base["status"] == 0)
    dz = np.abs(back[ok] - base["zu"][ok]).reshape(int(ok.sum()), -1).max(1)
    assert dz.max() < 1e-3 and np.quantile(dz, 0.99) < 1e-6 and np.median(dz) < 1e-10, (dz.max(), np.quantile(dz, 0.99), np.median(dz))


def test_half_turn_symmetry(eng):
    """And the rotation by pi about the lot's centre (x -> 35 - x, y -> 35 - y, psi -> psi + pi; both box bounds are symmetric about
    17.5; obstacles -A, b - 35 (A_x + A_y)): the headings leave the range the fixtures cover, every cos / sin changes sign, and the
    solution turns with the problem."""
    import dataclasses

    from conflict_rez_amd import engine, scenarios

    table, _ = scenarios.load_reference_table(kind="planned")
    k0, noise = scenarios.sample_scenarios(1024, table, seed=2025, spec=eng.spec)
    x0, ref, nbr, zu = scenarios.mpc_batch_from_table(eng.spec, table, k0, noise)
    base = eng.solve(x0, ref, nbr, zu, want_duals=False)

    def turn(a, axis, sign=1.0):  # rows (x, y, psi, ...) along `axis`
        a = np.array(a, float)
        idx = [slice(None)] * a.ndim
        for r in (0, 1):
            idx[axis] = r; a[tuple(idx)] = 35.0 - a[tuple(idx)]
        idx[axis] = 2; a[tuple(idx)] = a[tuple(idx)] + sign * np.pi
        return a

    A, b = eng.spec.A_obs, eng.spec.b_obs
    spt = dataclasses.replace(eng.spec, A_obs=-A, b_obs=b - 35.0 * (A[:, :, 0] + A[:, :, 1]))
    et = engine.Engine(spt, max_batch=len(x0))
    out = et.solve(turn(x0, 1), turn(ref, 1), turn(nbr, 2), turn(zu, 1), want_duals=False)
    et.close()
    back = turn(out["zu"], 1, -1.0)
    same = (out["status"] == base["status"]) & (out["iters"] == base["iters"])
    assert same.mean() > 0.99, same.mean()
    ok = same & (base["status"] == 0)
    dz = np.abs(back[ok] - base["zu"][ok]).reshape(int(ok.sum()), -1).max(1)
    assert dz.max() < 1e-3 and np.quantile(dz, 0.99) < 1e-6 and np.median(dz) < 1e-9, (dz.max(), np.quantile(dz, 0.99), np.median(dz))


def test_closed_loop_on_device(eng, ospec):
    """cfz_loop_step (loop_prep / solve_kernel / loop_post) AND cfz_loop_run (the persistent loop_kernel, what bench.py
    times) against a host replay of the same Jacobi iteration with the oracle's C port: reference-table indexing,
    `_adv_onestep`, carried multipliers, shift fallback, plant RK4 -- equal status and iteration count of every solve,
    states and predictions to 1e-6 (rounding is amplified by the closed loop, not reset by it)."""
    from conflict_rez_amd import scenarios

    table, _ = scenarios.load_reference_table()
    S, steps = 8, 5
    k0, noise = scenarios.sample_scenarios(S, table, seed=3)
    eng.loop_init(table, k0, noise)
    from oracle.closed_loop import replay as host_replay

    replay = list(host_replay(ospec, table, k0, noise, steps, dt=eng.spec.dt, wb=eng.spec.wb))
    n_fallback = 0
    for t, (state, pred, status, iters) in enumerate(replay):
        eng.loop_step()
        got = eng.loop_get()
        assert np.array_equal(got["status"], status), (t, got["status"], status)
        assert np.array_equal(got["iters"], iters), (t, got["iters"], iters)
        assert np.abs(got["state"] - state).max() < 1e-6, t
        assert np.abs(got["pred"] - pred).max() < 1e-6, t
        n_fallback += int((status != 0).sum())
    assert (replay[-1][2] == 0).mean() > 0.7
    assert n_fallback >= 1  # the shift fallback of loop_post ran (the replay at this seed has 21 of them)
    # the persistent launch: all `steps` iterations in one kernel, same end point as the replay
    eng.loop_init(table, k0, noise)
    eng.loop_run(steps)
    got = eng.loop_get()
    state, pred, status, iters = replay[-1]
    assert np.array_equal(got["status"], status) and np.array_equal(got["iters"], iters)
    assert np.abs(got["state"] - state).max() < 1e-6 and np.abs(got["pred"] - pred).max() < 1e-6
    # every vehicle moved along its reference: position error against the table after `steps`
    V, T = table.shape[0], table.shape[1]
    for s in range(S):
        for v in range(V):
            tgt = table[v, min(k0[s] + steps, T - 1), :2]
            assert np.hypot(*(got["state"][s, v, :2] - tgt)) < 1.0


def test_every_solve_of_the_bench_workload_against_the_port(ospec):
    """The workload that produces the bench's number -- planned reference table, feasible starts, sampler seed 2024, multipliers
    carried from one MPC iteration to the next -- checked solve by solve: after every `cfz_loop_step` of the device loop the C port
    solves the SAME inputs (the device's own states and predictions of the iteration before: rounding differences between the two
    implementations are not fed back, so a Jacobi ping-pong cannot amplify them) with its own carried multipliers.  Equal status and
    iteration count of EVERY solve (256 scenarios x 4 vehicles x 8 iterations), converged predictions to 1e-5.  Covers restorations
    (starts half a metre inside a neighbour's prediction), status 4 / 5 exits and the carried shift hint as they occur."""
    from conflict_rez_amd import engine, scenarios
    from oracle import port
    from oracle.closed_loop import step_inputs

    spec = scenarios.parking_lot_spec()
    table, _ = scenarios.load_reference_table(kind="planned")
    S, steps = 256, 8
    k0, noise = scenarios.sample_scenarios(1024, table, seed=2024, spec=spec)
    k0, noise = k0[:S], noise[:S]
    V, N = table.shape[0], spec.N
    e = engine.Engine(spec, max_batch=S * V)
    e.loop_init(table, k0, noise)
    carry = [[None] * V for _ in range(S)]
    n = n_resto = 0
    seen = set()
    for t in range(steps):
        g0 = e.loop_get()
        state, pred = g0["state"].reshape(S, V, 5), g0["pred"].reshape(S, V, 7, N)
        e.loop_step()
        g1 = e.loop_get()
        st, it, p1 = g1["status"].reshape(S, V), g1["iters"].reshape(S, V), g1["pred"].reshape(S, V, 7, N)
        for s in range(S):
            for v in range(V):
                x0, ref, nb, w = step_inputs(table, k0[s] + t, state[s], pred[s], v)
                r = port.solve(ospec, x0, ref, nb, w.T.copy(), carry=carry[s][v])
                carry[s][v] = r["carry"]
                assert (r["status"], r["iters"]) == (int(st[s, v]), int(it[s, v])), (t, s, v, r["status"], r["iters"], st[s, v], it[s, v])
                if r["status"] == 0:  # (measured worst case over the 8,192 solves: 1.9e-6, at an input w where v ~ 0 -- TOL_U above; 1e-6 held until the
                                       # sweep moved to the matrix cores.  Port and kernel share the sweep's bits, not the reductions': DESIGN.md section 5)
                    assert np.abs(r["p"].T - p1[s, v]).max() < 1e-5, (t, s, v)
                n += 1; seen.add(r["status"])
                n_resto += r["status"] == 0 and r["iters"] >= 35
    e.close()
    assert n == S * V * steps and {0, 4, 5} <= seen and n_resto >= 3


def test_persistent_launch_and_the_carried_shift_hint():
    """On the bench's workload: the persistent launch equals the stepwise loop bit for bit; and `carry_shift` does what it is for --
    the solves that follow a long converged solve of the same vehicle (35+ iterations: the late curvature shift, or a restoration) take
    a median of 16 iterations with the hint and 36 without, and over the run the hint saves iterations."""
    from conflict_rez_amd import engine, scenarios

    spec = scenarios.parking_lot_spec()
    table, _ = scenarios.load_reference_table(kind="planned")
    S, steps = 128, 20
    k0, noise = scenarios.sample_scenarios(1024, table, seed=2024, spec=spec)
    k0, noise = k0[:S], noise[:S]
    runs = {}
    for cs in (1, 0):
        e = engine.Engine(spec, max_batch=4 * S, carry_shift=cs)
        e.loop_init(table, k0, noise)
        its, sts = [], []
        for t in range(steps):
            e.loop_step()
            g = e.loop_get()
            its.append(g["iters"].copy().reshape(S, 4)); sts.append(g["status"].copy().reshape(S, 4))
        last = e.loop_get()
        if cs == 1:
            e.loop_init(table, k0, noise)
            e.loop_run(steps)
            pers = e.loop_get()
            for key in ("state", "pred", "status", "iters"):
                assert np.array_equal(last[key], pers[key]), key
        e.close()
        runs[cs] = (np.array(its), np.array(sts))

    def after_long(its, sts):  # iterations of the converged solve that follows a converged solve of 35+ iterations of the same vehicle
        return [its[t + 1, s, v] for t in range(steps - 1) for s in range(S) for v in range(4)
                if its[t, s, v] >= 35 and sts[t, s, v] == 0 and sts[t + 1, s, v] == 0]

    a1, a0 = after_long(*runs[1]), after_long(*runs[0])  # (C port on the same scenarios: 44 solves, median 16, against 57, median 36)
    assert len(a1) >= 20 and len(a0) >= 20 and np.median(a1) <= 25 and np.median(a0) >= 30, (len(a1), np.median(a1), len(a0), np.median(a0))
    assert runs[1][0].sum() < runs[0][0].sum()


def test_persistent_loop_equals_stepwise_loop(eng):
    """cfz_loop_run(K) (one persistent launch, scenarios free-running) == K x cfz_loop_step, bit for bit:
    the same solves on the same inputs, only scheduled differently.  More scenarios than resident
    workgroups so that the work queue really recycles workgroups."""
    from conflict_rez_amd import scenarios

    table, _ = scenarios.load_reference_table()
    S, K = 256, 6
    k0, noise = scenarios.sample_scenarios(S, table, seed=11)
    eng.loop_init(table, k0, noise)
    for _ in range(K):
        eng.loop_step()
    a = eng.loop_get()
    eng.loop_init(table, k0, noise)
    n_it = eng.loop_run(K)
    b = eng.loop_get()
    for key in ("state", "pred", "status", "iters"):
        assert np.array_equal(a[key], b[key]), key
    assert n_it >= int(b["iters"].sum())
    # split runs continue where the last one stopped
    eng.loop_init(table, k0, noise)
    eng.loop_run(2); eng.loop_run(1); eng.loop_run(3)
    c = eng.loop_get()
    for key in ("state", "pred", "status", "iters"):
        assert np.array_equal(a[key], c[key]), key


def test_carried_multipliers_match_oracle(eng):
    """cfz_mpc_set_carry: consecutive MPC iterations of one slot started from the previous solve's multipliers
    reproduce the oracle's carried sequence (tests/golden/carry_golden.npz); without the flag the solve is cold."""
    import os

    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    ci, cg = np.load(os.path.join(here, "carry_inputs.npz")), np.load(os.path.join(here, "carry_golden.npz"))
    for t in range(3):
        idx = [t, 3 + t, 6 + t]  # slot s = sequence s; the third: a cornered vehicle whose successors start with the curvature
        #                          shift its first solve needed (cfz_options.carry_shift: 10 and 14 iterations instead of 38 and 44)
        out = eng.solve(ci["x0"][idx], ci["ref"][idx], ci["nbr"][idx], ci["zu"][idx], want_duals=False,
                        carry=None if t == 0 else [1, 1, 1])
        for slot, i in enumerate(idx):
            assert (out["status"][slot], out["iters"][slot]) == (int(cg["meta"][i, 0]), int(cg["meta"][i, 1])), (t, slot)
            assert np.abs(out["zu"][slot] - cg["sol"][i]).max() < 1e-6
    # same inputs again without the flag: the cold iteration counts
    out = eng.solve(ci["x0"][[2, 5]], ci["ref"][[2, 5]], ci["nbr"][[2, 5]], ci["zu"][[2, 5]], want_duals=False)
    assert list(out["iters"]) == [int(cg["meta"][2, 4]), int(cg["meta"][5, 4])]


def test_closed_loop_carry_saves_iterations():
    """The closed loop carries multipliers from one MPC iteration to the next: same outcomes (statuses within a
    handful of instances, states within the solver tolerance band), less than 60 % of the iterations."""
    from conflict_rez_amd import engine, scenarios

    spec = scenarios.parking_lot_spec()
    table, _ = scenarios.load_reference_table()
    S, K = 128, 8
    k0, noise = scenarios.sample_scenarios(S, table, seed=5)
    res = {}
    for carry in (1, 0):
        e = engine.Engine(spec, max_batch=S * 4, carry_duals=carry)
        e.loop_init(table, k0, noise)
        e.loop_run(1)
        first = e.loop_get()["iters"].sum()
        n_it = e.loop_run(K - 1)
        res[carry] = (e.loop_get(), n_it, first)
        e.close()
    a, b = res[1][0], res[0][0]
    assert res[1][2] == res[0][2]  # the first iteration has nothing to carry
    assert res[1][1] < 0.6 * res[0][1], (res[1][1], res[0][1])
    assert (a["status"] != b["status"]).mean() < 0.02
    # a different outcome of one solve (converged / fallback) sends that scenario down another path: compare the rest
    d = np.abs(a["state"].reshape(-1, 5) - b["state"].reshape(-1, 5)).max(1)
    assert (d < 5e-2).mean() > 0.95 and np.median(d) < 1e-3


def test_other_shapes_and_error_paths():
    """Shapes other than the headline one (no neighbours / 4 obstacles = BASELINE.json configs[1]; short horizons; no
    obstacles; a batch of one) against the C port, and the C ABI's error convention (-1 + cfz_last_error)."""
    from conflict_rez_amd import engine, scenarios
    from oracle import port
    from oracle.mpc_nlp import MpcSpec

    table, _ = scenarios.load_reference_table()
    # (round 6: N = 32 / 31 -- no / exactly one stage's worth of spare lanes for the stage-0 check -- and N = 4, too short for the value
    # function to leave the cos / sin slots alone: the horizons where the kernel's layout switches over, tests/test_emu_kernel.py)
    for n_obs, n_nbr, N, B in ((4, 0, 30, 5), (6, 1, 12, 3), (0, 2, 8, 1), (6, 3, 32, 4), (6, 3, 31, 4), (6, 1, 4, 4)):
        sp = scenarios.parking_lot_spec(n_nbr=n_nbr, N=N, n_obs=n_obs)
        osp = MpcSpec(N=N, dt=sp.dt, A_obs=sp.A_obs, b_obs=sp.b_obs, n_nbr=n_nbr)
        k0, noise = scenarios.sample_scenarios(B, table, seed=4)
        x0, ref, nbr, zu = scenarios.mpc_batch_from_table(sp, table[: n_nbr + 1], k0, noise[:, : n_nbr + 1])
        x0, ref, nbr, zu = x0[:B], ref[:B], nbr[:B], zu[:B]
        e = engine.Engine(sp, max_batch=B)
        out = e.solve(x0, ref, nbr, zu)
        for b in range(B):
            r = port.solve(osp, x0[b], ref[b], nbr[b], zu[b].T)
            assert (r["status"], r["iters"]) == (out["status"][b], out["iters"][b]), (n_obs, n_nbr, N, b)
            if r["status"] == 0:
                assert np.abs(r["p"].T[:5] - out["zu"][b][:5]).max() < TOL and np.abs(r["p"].T[5:] - out["zu"][b][5:]).max() < TOL_U
        assert out["l"].shape == (B, N, 4 * n_obs) and out["lam_ij"].shape == (B, n_nbr, N, 4)
        # one instance more than the handle was built for
        with pytest.raises(RuntimeError, match="batch size out of range"):
            e.solve(np.repeat(x0, 2, 0), np.repeat(ref, 2, 0), np.repeat(nbr, 2, 0), np.repeat(zu, 2, 0))
        e.close()
    # a horizon or an obstacle count beyond the compiled limits is refused at creation
    with pytest.raises(ValueError, match="compiled limits"):
        engine.Engine(scenarios.parking_lot_spec(N=65), max_batch=1)
    with pytest.raises(RuntimeError, match="batch"):
        engine.Engine(scenarios.parking_lot_spec(), max_batch=0)
    with pytest.raises(RuntimeError, match="loop_init"):
        e2 = engine.Engine(scenarios.parking_lot_spec(), max_batch=4)
        try:
            e2.loop_step()
        finally:
            e2.close()


def test_vehicle_sharded_loop_matches_device_loop():
    """Partitioning B (distributed.VehicleShardedLoop: RCCL all-gather of the predictions, then `cfz_vsl_step` -- prep,
    solve, read-back / fallback, plant as HIP kernels on torch's stream) with a single rank owning all four vehicles = the
    device-resident loop `cfz_loop_step`, step for step and bit for bit."""
    import socket

    import torch
    import torch.distributed as dist

    from conflict_rez_amd import engine, scenarios
    from conflict_rez_amd.distributed import VehicleShardedExchange, VehicleShardedLoop

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        spec = scenarios.parking_lot_spec()
        table, _ = scenarios.load_reference_table()
        S, K = 32, 4
        k0, noise = scenarios.sample_scenarios(S, table, seed=21)
        ea, eb = engine.Engine(spec, max_batch=S * 4), engine.Engine(spec, max_batch=S * 4)
        ea.loop_init(table, k0, noise)
        vl = VehicleShardedLoop(eb, VehicleShardedExchange(4), table, k0, noise)
        for t in range(K):
            ea.loop_step()
            vl.step(sync=True)
            a = ea.loop_get()
            assert np.array_equal(a["status"].ravel(), vl.status.cpu().numpy()), t
            assert np.array_equal(a["iters"].ravel(), vl.iters.cpu().numpy()), t
            # the same kernels on both sides (solve_kernel, the same RK4 plant): bit for bit
            assert np.array_equal(a["state"].reshape(-1, 5), vl.state.reshape(-1, 5).cpu().numpy())
            assert np.array_equal(a["pred"].reshape(-1, 7, spec.N), vl.pred.reshape(-1, 7, spec.N).cpu().numpy())
        ea.close(); eb.close()
    finally:
        dist.destroy_process_group()


def test_joint_dual_ws_certificates(eng, tmp_path):
    """cfz_joint_dual_ws (multi_vehicle_planner.py:208-341): the duals satisfy the reference's rows (:292-295) exactly,
    d is the separation of the two bodies for face-vertex closest features (known distances of aligned rectangles),
    and `MultiVehiclePlanner.joint_dual_ws` lays the results out as the reference does."""
    from oracle.mpc_nlp import rot

    rng = np.random.default_rng(3)
    n = 200
    pa = np.stack([rng.uniform(5, 30, n), rng.uniform(8, 27, n), rng.uniform(-3.2, 3.2, n)], 1)
    pb = pa + np.stack([rng.uniform(-9, 9, n), rng.uniform(-9, 9, n), rng.uniform(-3.2, 3.2, n)], 1)
    lam, mu, s, d = eng.joint_dual_ws(pa, pb)
    G, g = np.array([[1.0, 0], [0, 1], [-1, 0], [0, -1]]), np.asarray(eng.spec.g, float)
    from oracle.geometry import body_polygon_world, polygon_distance

    n_vv = 0
    for k in range(n):
        tA = G @ rot(-pa[k, 2]); tb = tA @ pa[k, :2] + g
        oA = G @ rot(-pb[k, 2]); ob = oA @ pb[k, :2] + g
        assert (lam[k] >= 0).all() and (mu[k] >= 0).all() and s[k] @ s[k] <= 1 + 1e-12
        assert np.abs(tA.T @ lam[k] + s[k]).max() < 1e-12 and np.abs(oA.T @ mu[k] - s[k]).max() < 1e-12
        assert abs(-tb @ lam[k] - ob @ mu[k] - d[k]) < 1e-10
        # the reference MAXIMISES d (:296): the optimum is the distance of the two bodies.  Feasible duals certify
        # d <= distance (weak duality); equality with an independently computed distance proves optimality.
        dist, _, _ = polygon_distance(body_polygon_world(pa[k], g), body_polygon_world(pb[k], g))
        if dist > 1e-6:
            assert abs(d[k] - dist) < 1e-7, (k, d[k], dist)
            n_vv += (lam[k] > 1e-9).sum() == 2 and (mu[k] > 1e-9).sum() == 2  # a direction between face normals on both bodies
        else:
            assert d[k] <= 1e-9
    assert n_vv >= 10  # vertex-vertex closest features are among the cases
    # two parallel vehicles side by side, 3 m apart centre to centre: 3 - 0.9 - 0.9; nose to tail on one line: gap 2
    lam, mu, s, d = eng.joint_dual_ws([[10.0, 15.0, 0.0], [10.0, 15.0, 0.0]], [[10.0, 18.0, 0.0], [15.9, 15.0, 0.0]])
    assert abs(d[0] - 1.2) < 1e-12 and abs(d[1] - (15.9 - 0.6 - 10.0 - 3.3)) < 1e-12
    # corner to corner: front-left corner of the first (13.3, 15.9) and rear-right corner of the second (15.3, 16.9)
    lam, mu, s, d = eng.joint_dual_ws([[10.0, 15.0, 0.0]], [[15.9, 17.8, 0.0]])
    assert abs(d[0] - np.hypot(2.0, 1.0)) < 1e-12 and np.allclose(s[0], -np.array([2.0, 1.0]) / np.hypot(2.0, 1.0), atol=1e-12)
    # the planner surface
    from conflict_rez_amd import strategy as strat
    from conflict_rez_amd.control.multi_vehicle_planner import MultiVehiclePlanner
    from conflict_rez_amd.pytypes import VehiclePrediction

    fn = str(tmp_path / "4v_rl_traj")
    strat.write_strategy(fn, strat.generate_strategy(4))
    agents = ["vehicle_%d" % i for i in range(4)]
    mvp = MultiVehiclePlanner(fn, {a: True for a in agents}, {a: {"front": (1, 0, 0), "back": (0, 0, 1)} for a in agents},
                              {a: None for a in agents}, {a: None for a in agents})
    K = 5
    for i, a in enumerate(agents):
        mvp.vehicles[a].N = 4 + i
        p = VehiclePrediction()
        m_ = mvp.vehicles[a].N * (K + 1)
        p.x, p.y, p.psi = 10.0 + 5 * i + 0.01 * np.arange(m_), 15.0 + 0.0 * np.arange(m_), 0.1 * i + 0.0 * np.arange(m_)
        mvp.single_results[a] = p
    mvp.joint_dual_ws(K=K)
    assert len(mvp.agent_pairs) == 6 and set(mvp.joint_l0["vehicle_0"]) == {"vehicle_1", "vehicle_2", "vehicle_3"}
    l01 = mvp.joint_l0["vehicle_0"]["vehicle_1"]
    assert len(l01) == 4 and len(l01[0]) == K + 1 and l01[0][0].shape == (4,)
    assert mvp.joint_s0[("vehicle_2", "vehicle_3")][5][K].shape == (2,) and len(mvp.joint_l0["vehicle_3"]["vehicle_2"]) == 6


def test_python_shim_closed_loop_on_gpu(tmp_path):
    """`MultiDistributedFollower` through the real engine: 4 vehicles, 40 iterations, vehicles never overlap
    (separating-axis check on the driven states) and follow their plans; the drop-in surface end to end."""
    from conflict_rez_amd import strategy as strat
    from conflict_rez_amd.control.vehicle_follower import MultiDistributedFollower
    from conflict_rez_amd.pytypes import VehicleState
    from test_follower_host import _references

    fn = str(tmp_path / "4v_rl_traj")
    strat.write_strategy(fn, strat.generate_strategy(4))
    names = [f"vehicle_{i}" for i in range(4)]
    mdf = MultiDistributedFollower(fn, {a: True for a in names}, {a: {"front": (1, 0, 0), "back": (0, 1, 0)} for a in names},
                                   {a: VehicleState() for a in names}, {a: None for a in names})
    mdf.setup_multi_vehicles(references=_references())
    mdf.solve(num_iter=40, dump=False)
    g = np.array([3.3, 0.9, 0.6, 0.9])
    corners = np.array([[g[0], g[1]], [-g[2], g[1]], [-g[2], -g[3]], [g[0], -g[3]]])

    def poly(v, i):
        c, s = np.cos(v.final_traj.psi[i]), np.sin(v.final_traj.psi[i])
        return np.array([v.final_traj.x[i], v.final_traj.y[i]]) + corners @ np.array([[c, s], [-s, c]])

    def separated(P, Q):
        for poly_ in (P, Q):
            for a, b in zip(poly_, np.roll(poly_, -1, 0)):
                n = np.array([b[1] - a[1], a[0] - b[0]])
                if (P @ n).max() < (Q @ n).min() or (Q @ n).max() < (P @ n).min():
                    return True
        return False

    n_fail = 0
    for v in mdf.vehicles:
        n_fail += sum(t == 0.5 for t in v.iter_time)
        ref = v.interpolate_states([v.state.t])
        assert np.hypot(v.state.x.x - ref.x[0], v.state.x.y - ref.y[0]) < 0.5
    assert n_fail <= 8
    for i in range(41):
        for a in range(4):
            for b in range(a + 1, 4):
                assert separated(poly(mdf.vehicles[a], i), poly(mdf.vehicles[b], i)), (i, a, b)


@pytest.mark.parametrize("prod", [False, True])
def test_full_size_instances_against_the_independent_solver_on_gpu(prod):
    """The HIP engine through the C ABI against optima of the reference's NLP computed by an INDEPENDENT solver on an
    independent statement (polygon distances instead of OBCA duals, scipy SLSQP; tests/golden/mpc_independent.npz,
    N = 30, six obstacles, three neighbours): feasible for the reference's constraints and the same optimum on all twelve
    instances, vertex-vertex contacts included.
    The assertions are tests/test_independent_solver.py:check_against_independent, shared with the CPU test of the port."""
    from conflict_rez_amd import engine, scenarios
    from test_independent_solver import TIGHT_FULL, _independent_fixture, check_against_independent

    d, _ = _independent_fixture()
    opts = {} if prod else dict(**TIGHT_FULL, stall_iters=0)
    e = engine.Engine(scenarios.parking_lot_spec(), max_batch=len(d["x0"]), **opts)
    out = e.solve(d["x0"], d["ref"], d["nbr"], d["zu"], want_duals=False)

    def solve(b, x0, ref, nbr, zu):
        return int(out["status"][b]), out["zu"][b]

    check_against_independent(solve, 1e-4, prod)
    e.close()


@pytest.mark.parametrize("fixture", ["mpc_independent_more.npz", "mpc_independent_obs.npz", "mpc_independent_turn.npz"])
@pytest.mark.parametrize("prod", [False, True])
def test_population_against_the_independent_solver_on_gpu(prod, fixture):
    """The populations of tests/test_independent_solver.py (active rows from the bench's sampler, intruder corners with
    vertex-vertex contacts, static obstacles squeezed past) in one batch each through the C ABI, same assertions as the CPU
    test of the port."""
    from conflict_rez_amd import engine, scenarios
    from test_independent_solver import POPULATIONS, TIGHT_FULL, _fixture_file, check_against_independent

    d, _ = _fixture_file(fixture)
    opts = {} if prod else dict(**TIGHT_FULL, stall_iters=0)
    e = engine.Engine(scenarios.parking_lot_spec(), max_batch=len(d["x0"]), **opts)
    out = e.solve(d["x0"], d["ref"], d["nbr"], d["zu"], want_duals=False)
    check_against_independent(lambda b, *a: (int(out["status"][b]), out["zu"][b]), 1e-4, prod, fixture=fixture, better=POPULATIONS[fixture][0],
                              fails=POPULATIONS[fixture][1], stuck=POPULATIONS[fixture][2])
    e.close()


def test_node_loop_on_gpu(tmp_path):
    """The reference's ROS2 deployment protocol (ros2_ws/src/confrez_ros/src/vehicle_node.py:111-190) without ROS, against
    the real engine: four `VehicleNode`s over the in-process bus, every node stepping ITS vehicle with a batch of one in
    its own carry slot of the shared engine.  30 ticks: every node steps, solves converge from the carried multipliers
    in a few iterations, the vehicles never overlap and follow their plans."""
    from conflict_rez_amd import strategy as strat
    from conflict_rez_amd.control.vehicle_follower import MultiDistributedFollower
    from conflict_rez_amd.node import InProcessBus, VehicleNode
    from conflict_rez_amd.pytypes import VehicleState
    from test_follower_host import _references

    fn = str(tmp_path / "4v_rl_traj")
    strat.write_strategy(fn, strat.generate_strategy(4))
    names = [f"vehicle_{i}" for i in range(4)]
    mdf = MultiDistributedFollower(fn, {a: True for a in names}, {a: {"front": (1, 0, 0), "back": (0, 1, 0)} for a in names},
                                   {a: VehicleState() for a in names}, {a: None for a in names})
    mdf.setup_multi_vehicles(references=_references())
    assert [v.slot for v in mdf.vehicles] == [0, 1, 2, 3]
    iters = {a: [] for a in names}
    orig = mdf.engine.solve

    def counting(*args, **kw):
        out = orig(*args, **kw)
        iters[names[int(kw["slots"][0])]].append((int(out["status"][0]), int(out["iters"][0])))
        return out

    mdf.engine.solve = counting
    bus = InProcessBus()
    nodes = [VehicleNode(v, 4, bus) for v in mdf.vehicles]
    for n in nodes:
        n.publish_prediction()
    ticks = 30
    for _ in range(ticks):
        for n in nodes:
            n.timer_callback()
    assert [n.steps for n in nodes] == [ticks - 1] * 3 + [ticks]  # in the first round only the last node has heard everybody
    for a in names:
        st = np.array(iters[a])
        assert (st[:, 0] == 0).mean() > 0.85, (a, st[:, 0])
        assert np.median(st[1:, 1]) <= 4, (a, st[:, 1])  # carried multipliers: a few iterations per step
    g = np.array([3.3, 0.9, 0.6, 0.9])
    corners = np.array([[g[0], g[1]], [-g[2], g[1]], [-g[2], -g[3]], [g[0], -g[3]]])

    def poly(v, i):
        c, s = np.cos(v.final_traj.psi[i]), np.sin(v.final_traj.psi[i])
        return np.array([v.final_traj.x[i], v.final_traj.y[i]]) + corners @ np.array([[c, s], [-s, c]])

    def separated(P, Q):
        for poly_ in (P, Q):
            for a_, b_ in zip(poly_, np.roll(poly_, -1, 0)):
                n_ = np.array([b_[1] - a_[1], a_[0] - b_[0]])
                if (P @ n_).max() < (Q @ n_).min() or (Q @ n_).max() < (P @ n_).min():
                    return True
        return False

    for i in range(ticks - 1):
        for a in range(4):
            for b in range(a + 1, 4):
                assert separated(poly(mdf.vehicles[a], i), poly(mdf.vehicles[b], i)), (i, a, b)
    for v in mdf.vehicles:
        ref = v.interpolate_states([v.state.t])
        assert np.hypot(v.state.x.x - ref.x[0], v.state.x.y - ref.y[0]) < 0.5


def test_dual_ws_certificates(eng, ospec):
    """`cfz_dual_ws` (reference Vehicle.dual_ws, vehicle.py:233-296: maximise d over the duals): every returned (lambda, mu)
    satisfies the reference's rows (:276-280) for its pose with |A'lambda| = 1, and d IS the optimum: the Euclidean distance
    of body and obstacle from an independent computation (a QP over the vertices, oracle/geometry.py) -- face-vertex and
    vertex-vertex closest features alike."""
    from conflict_rez_amd import scenarios
    from oracle.geometry import body_polygon_world, polygon_distance
    from oracle.mpc_nlp import polytope_vertices, rot

    table, _ = scenarios.load_reference_table()
    rng = np.random.default_rng(5)
    poses = np.concatenate([table[:, ::7, :3].reshape(-1, 3)[::5],
                            np.stack([rng.uniform(3, 32, 80), rng.uniform(14.5, 20.5, 80), rng.uniform(-3.2, 3.2, 80)], 1)])
    l, m, d = eng.dual_ws(poses)
    G, g = ospec.G, ospec.g
    n_vv = 0
    for k in range(len(poses)):
        t, R = poses[k, :2], rot(poses[k, 2])
        W = body_polygon_world(poses[k], g)
        for j in range(ospec.n_obs):
            A, b = ospec.A_obs[j], ospec.b_obs[j]
            lj, mj = l[k, 4 * j:4 * j + 4], m[k, 4 * j:4 * j + 4]
            assert lj.min() >= 0 and mj.min() >= 0
            assert np.abs(G.T @ mj + R.T @ A.T @ lj).max() < 1e-12
            assert abs(np.dot(A.T @ lj, A.T @ lj) - 1.0) < 1e-12
            assert abs(np.dot(-g, mj) + np.dot(A @ t - b, lj) - d[k, j]) < 1e-10
            dist, _, _ = polygon_distance(polytope_vertices(A, b)[0], W)
            if dist > 1e-6:
                assert abs(d[k, j] - dist) < 1e-7, (k, j, d[k, j], dist)
                n_vv += (lj > 1e-9).sum() == 2 and (mj > 1e-9).sum() == 2
            else:
                assert d[k, j] <= 1e-9
    assert n_vv >= 10
    # known answers: axis-aligned vehicle beside obstacle 0 (box x in [2.85,14.65], y in [7.5,13.75]); and diagonally off
    # its corner (14.65, 13.75): rear-left body corner at (15.65, 15.75) -> distance hypot(1, 2)
    _, _, d0 = eng.dual_ws(np.array([[8.0, 16.25, 0.0], [20.0, 10.0, 0.0], [16.25, 16.65, 0.0]]))
    assert abs(d0[0, 0] - (16.25 - 0.9 - 13.75)) < 1e-12 and abs(d0[1, 0] - (20.0 - 0.6 - 14.65)) < 1e-12
    assert abs(d0[2, 0] - np.hypot(1.0, 2.0)) < 1e-12


def test_late_shift_fixture(eng):
    """tests/golden/mpc_late_shift.npz (full-KKT oracle): solves that pass iteration 60 with a scaled row curvature switch to
    the shifted one (cfz_options.shift_after) and converge; with shift_after = 0 the same solves run into max_iter."""
    import os

    from conflict_rez_amd import engine

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mpc_late_shift.npz"))
    out = eng.solve(g["x0"], g["ref"], g["nbr"], g["zu"])
    assert out["status"].tolist() == [0] * len(g["x0"]) and out["iters"].tolist() == g["iters_shift"].tolist()
    assert np.abs(out["zu"][:, :5] - g["sol"][:, :5]).max() < 1e-6 and np.abs(out["zu"][:, 5:] - g["sol"][:, 5:]).max() < 1e-4
    e0 = engine.Engine(eng.spec, max_batch=16, shift_after=0, err_stall_iters=0, reg_dual_rows=0.0)  # neither the dual regularisation nor the late shift, no error-stall stop: to the limit
    try:
        o0 = e0.solve(g["x0"], g["ref"], g["nbr"], g["zu"])
    finally:
        e0.close()
    assert o0["iters"].tolist() == g["iters_noshift"].tolist() and (o0["status"] == 1).all()


def test_duplicate_carry_slots_are_refused(eng, golden):
    """`cfz_mpc_set_slots`: two instances of one launch on the same carry record would race on it (and hand one vehicle the other's
    multipliers), so a call with a repeated slot is an API error; distinct slots go through."""
    a = slice(0, 3)
    with pytest.raises(RuntimeError, match="duplicate carry slot"):
        eng.solve(golden["x0"][a], golden["ref"][a], golden["nbr"][a], golden["zu"][a], want_duals=False, slots=[5, 7, 5])
    out = eng.solve(golden["x0"][a], golden["ref"][a], golden["nbr"][a], golden["zu"][a], want_duals=False, slots=[5, 7, 9])
    assert out["status"].tolist() == golden["meta"][a, 0].astype(int).tolist()
