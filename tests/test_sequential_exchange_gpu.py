"""The sequential exchange of the closed loop (`cfz_loop_set_order`, `Engine.loop_set_order`) on the GPU: every solve against the C
port on inputs rebuilt by the rule, the persistent launch against the stepwise loop, the clearance statement, the API's refusals and
the reference surface (`MultiDistributedFollower.solve(order=...)`).

The rule: in MPC iteration t the V solves of scenario s run in the order order[s]; the vehicle of rank r plans against the predictions
of the vehicles ranked before it from iteration t (not advanced: they start at time t) and the predictions of iteration t-1 of the
others, advanced one step.  A converged solve then keeps dmin - constr_viol_tol from every prediction ranked before it at stages 1..N-1.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audit_binding as ab  # noqa: E402
from loop_cases import orders as _orders  # noqa: E402

HYST = 1e-3  # the working set's hysteresis: a row enters it within 1 mm of its bound


def _bench_workload(S):
    from conflict_rez_amd import scenarios

    spec = scenarios.parking_lot_spec()
    table, _ = scenarios.load_reference_table(kind="planned")
    k0, noise = scenarios.sample_scenarios(1024, table, seed=2024, spec=spec)
    return spec, table, k0[:S], noise[:S]


def _violations(spec, pred, status, order, thr):
    """(checked pairs, [(s, v, u, k, distance)] below thr): every converged vehicle v against every u ranked before it in its
    scenario, predictions pred [S,V,7,N] of one iteration at stages 1..N-1."""
    S, V, N = pred.shape[0], pred.shape[1], pred.shape[3]
    P = ab.body(spec.g, pred[:, :, 0, 1:], pred[:, :, 1, 1:], pred[:, :, 2, 1:])  # [S,V,N-1,4,2]
    rank = np.argsort(order, axis=1)
    n, bad = 0, []
    for v in range(V):
        for u in range(V):
            if u == v:
                continue
            sel = (rank[:, u] < rank[:, v]) & (status[:, v] == 0)
            if not sel.any():
                continue
            d = ab.signed_distance(P[sel, v], P[sel, u])  # [n_sel, N-1]
            n += int(sel.sum())
            for i, k in zip(*np.nonzero(d < thr)):
                bad.append((int(np.flatnonzero(sel)[i]), v, u, int(k) + 1, float(d[i, k])))
    return n, bad


def test_every_sequential_solve_of_the_bench_workload_against_the_port(ospec):
    """128 scenarios of the bench workload, 8 `loop_step`s under seeded per-scenario orders (identity and reversed included): after
    every step each solve's inputs are rebuilt by the rule from `loop_get` before and after the step (ranks before v: after the step,
    not advanced; ranks after v and v's own warm start: before the step, advanced) and solved by the C port with its own carry record
    per (s, v).  Equal status and iteration count of every solve, converged predictions to 1e-5 (the Jacobi test's tolerance)."""
    from conflict_rez_amd import engine
    from oracle import port
    from oracle.closed_loop import step_inputs

    spec, table, k0, noise = _bench_workload(128)
    S, steps = len(k0), 8
    V = table.shape[0]
    order = _orders(S, V, seed=5)
    rank = np.argsort(order, axis=1)
    e = engine.Engine(spec, max_batch=S * V)
    e.loop_init(table, k0, noise)
    e.loop_set_order(order)
    carry = [[None] * V for _ in range(S)]
    n, worst, seen = 0, 0.0, set()
    for t in range(steps):
        g0 = e.loop_get()
        e.loop_step()
        g1 = e.loop_get()
        state, pred, p1 = g0["state"], g0["pred"], g1["pred"]
        for s in range(S):
            for v in order[s]:
                x0, ref, nb, w = step_inputs(table, k0[s] + t, state[s], pred[s], v, p1[s], order[s][: rank[s, v]])
                r = port.solve(ospec, x0, ref, nb, w.T.copy(), carry=carry[s][v])
                carry[s][v] = r["carry"]
                got = (int(g1["status"][s, v]), int(g1["iters"][s, v]))
                assert (r["status"], r["iters"]) == got, (t, s, int(v), r["status"], r["iters"], got)
                if r["status"] == 0:
                    dev = float(np.abs(r["p"].T - p1[s, v]).max())
                    worst = max(worst, dev)
                    assert dev < 1e-5, (t, s, int(v), dev)
                n += 1
                seen.add(r["status"])
    e.close()
    print(f"{n} sequential solves equal to the port's (status {sorted(seen)}), worst converged |dp| {worst:.2e}")
    assert n == S * V * steps and 0 in seen


@pytest.mark.parametrize("S,blocks_per_cu", [(16, None), (1024, 1)])
def test_persistent_equals_stepwise_in_sequential_mode(S, blocks_per_cu, monkeypatch):
    """Sequential exchange: one persistent launch of 6 iterations, three launches of 2 + 1 + 3 and 6 `loop_step`s give the same
    state, predictions, status, iterations and record, bit for bit.  S = 16 has fewer scenarios than workgroups; S = 1024 with
    one workgroup per CU recycles workgroups over many items."""
    from conflict_rez_amd import engine

    if blocks_per_cu is not None:
        monkeypatch.setenv("CFZ_LOOP_BLOCKS_PER_CU", str(blocks_per_cu))
    spec, table, k0, noise = _bench_workload(S)
    V, K = table.shape[0], 6
    order = _orders(S, V, seed=11)
    e = engine.Engine(spec, max_batch=S * V)
    runs = {}
    for how in ("step", "split", "one"):
        e.loop_init(table, k0, noise)
        e.loop_set_order(order)
        e.loop_record(K)
        if how == "step":
            for _ in range(K):
                e.loop_step()
        elif how == "split":
            for k in (2, 1, 3):
                e.loop_run(k)
        else:
            e.loop_run(K)
        runs[how] = dict(e.loop_get(), **{"rec_" + k: v for k, v in e.loop_history().items()})
    e.close()
    for how in ("split", "one"):
        for key, val in runs["step"].items():
            assert np.array_equal(val, runs[how][key]), (how, key)
    assert (runs["one"]["rec_status"] == 0).mean() > 0.5


def test_clearance_statement_of_the_sequential_exchange():
    """Bench workload, 256 scenarios, 20 steps, seeded orders: every converged solve's new prediction keeps dmin - constr_viol_tol
    (less the working set's 1 mm hysteresis) from the new prediction of every vehicle ranked before it, at stages 1..N-1.  Printed, not
    asserted: how often the same predicate fails under Jacobi on the same workload, and the realised minimum clearance of both modes."""
    from conflict_rez_amd import engine

    spec, table, k0, noise = _bench_workload(256)
    S, steps, V = len(k0), 20, table.shape[0]
    tol = engine.default_options().constr_viol_tol
    thr = spec.dmin - tol - HYST
    order = _orders(S, V, seed=3)
    e = engine.Engine(spec, max_batch=S * V)
    report = {}
    for mode in ("sequential", "jacobi"):
        e.loop_init(table, k0, noise)
        e.loop_set_order(order if mode == "sequential" else None)
        e.loop_record(steps)
        n, bad, conv = 0, [], 0
        for t in range(steps):
            e.loop_step()
            g = e.loop_get()
            n_t, bad_t = _violations(spec, g["pred"], g["status"], order, thr)
            n += n_t; conv += int((g["status"] == 0).sum())
            bad += [(t,) + b for b in bad_t]
        clear = e.loop_audit()["clear"][:, 0]
        report[mode] = (n, bad, conv, float(clear.min()), int((clear < 0).sum()))
        print(f"{mode}: {n} (converged solve, earlier rank) pairs, {len(bad)} stage distances below {thr:.3f} m, "
              f"{conv} converged solves; realised vehicle-vehicle clearance min {clear.min():.4f} m, {int((clear < 0).sum())} scenarios "
              f"with contact" + (f"; first: (t, s, v, u, k, d) = {bad[0]}" if bad else ""))
    e.close()
    n, bad = report["sequential"][:2]
    assert n > 0.5 * S * steps * (V - 1) * V / 2, n
    assert not bad, bad[:10]


def test_api_refusals_and_reset():
    """Refused: a row that is not a permutation, a wrong shape, a call before `loop_init` (in Python and in the C library).  After
    `loop_set_order` then `loop_init`, and after `loop_set_order(None)`, a run equals a Jacobi run on a fresh handle, bit for bit; the
    identity order is not Jacobi."""
    import ctypes as C

    from conflict_rez_amd import engine

    spec, table, k0, noise = _bench_workload(32)
    S, V, K = len(k0), table.shape[0], 4
    fresh = engine.Engine(spec, max_batch=S * V)
    with pytest.raises(RuntimeError, match="cfz_loop_init has not been called"):
        fresh.loop_set_order(np.arange(V))
    fresh.loop_init(table, k0, noise)
    fresh.loop_run(K)
    jac = fresh.loop_get()
    fresh.close()

    e = engine.Engine(spec, max_batch=S * V)
    e.loop_init(table, k0, noise)
    for bad in ([0, 1, 2, 2], [0, 1, 2], np.zeros((S + 1, V), int), [[0, 1, 2, 3]] * (S - 1) + [[1, 2, 3, 4]], [0.0, 1.0, 2.0, 3.0]):
        with pytest.raises(ValueError):
            e.loop_set_order(bad)
    raw = np.tile(np.arange(V, dtype=np.int32), (S, 1)); raw[7] = [3, 3, 1, 0]
    assert e.lib.cfz_loop_set_order(e._h, raw.ctypes.data_as(C.c_void_p)) != 0
    assert "permutation" in e.lib.cfz_last_error().decode()

    def run():
        e.loop_run(K)
        return e.loop_get()

    e.loop_set_order(_orders(S, V, seed=1))
    e.loop_init(table, k0, noise)  # resets the order to Jacobi
    for key, val in run().items():
        assert np.array_equal(val, jac[key]), ("after loop_init", key)
    e.loop_init(table, k0, noise)
    e.loop_set_order(np.arange(V))
    e.loop_set_order(None)
    for key, val in run().items():
        assert np.array_equal(val, jac[key]), ("after loop_set_order(None)", key)
    e.loop_init(table, k0, noise)
    e.loop_set_order(np.arange(V))  # one order for every scenario
    ident = run()
    assert not np.array_equal(ident["pred"], jac["pred"])
    e.close()


def test_reference_surface_sequential_on_gpu(tmp_path):
    """`MultiDistributedFollower.solve(order=...)` on the real engine, 4 vehicles, 40 iterations in the strategy's planning priority:
    every converged step keeps the clearance statement against the vehicles stepped before it, and the driven states never overlap
    (the separating-axis check of the Jacobi shim test)."""
    from conflict_rez_amd import engine
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
    order = [names[i] for i in strat.DEFAULT_ORDER if i < 4]
    log = []  # (agent, status, pred x, y, psi) of every step, in the order they ran
    for v in mdf.vehicles:
        def wrapped(out, b=0, solve_time=None, _v=v, _orig=v.finish_step):
            _orig(out, b, solve_time=solve_time)
            log.append((_v.agent, _v.status, np.stack([_v.pred.x, _v.pred.y, _v.pred.psi]).copy()))
        v.finish_step = wrapped
    n_iter = 40
    mdf.solve(num_iter=n_iter, dump=False, order=order)
    assert [a for a, _, _ in log] == order * n_iter
    spec = mdf.vehicles[0].spec
    thr = spec.dmin - engine.default_options().constr_viol_tol - HYST
    n_checked = 0
    for i in range(n_iter):
        it = log[4 * i: 4 * i + 4]
        for r, (a, st, p) in enumerate(it):
            if st != 0:
                continue
            for _, _, q in it[:r]:
                d = ab.signed_distance(ab.body(spec.g, p[0, 1:], p[1, 1:], p[2, 1:]), ab.body(spec.g, q[0, 1:], q[1, 1:], q[2, 1:]))
                assert d.min() >= thr, (i, a, r, float(d.min()))
                n_checked += 1
    assert n_checked >= 3 * n_iter

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

    for i in range(n_iter + 1):
        for a in range(4):
            for b in range(a + 1, 4):
                assert separated(poly(mdf.vehicles[a], i), poly(mdf.vehicles[b], i)), (i, a, b)
