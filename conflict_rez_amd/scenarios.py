"""Synthetic inputs for the batched MPC engine.

The 4-vehicle parking-lot scenario: the six static obstacle boxes of the reference
(`compute_obstacles`), one planned reference trajectory per vehicle (a table sampled every
dt = 0.1 s) and, per scenario, a random start time on those references plus state noise.
Two reference tables are package data (`load_reference_table(kind)`):
  "planned"   `conflict_rez_amd/data/refs_4v_planned.npz`: what `VehicleFollower.plan_single_path` produces (vehicle_follower.py:91-138:
              state_ws -> dual_ws -> collocation plan with free dt) for the four vehicles of the synthetic strategy
              (`strategy.generate_strategy(4)`) on the GPU planning kernels, sampled every dt (7.8-15.7 s plans); written by
              `planned_reference_table` on an MI355X and reproduced by it in the GPU tests.  SURVEY.md 8d config 3 names this table.
  "state_ws"  `conflict_rez_amd/data/refs_4v.npz`: the four vehicles' `Vehicle.state_ws` warm-start plans (vehicle.py:99-231,
              tube-constrained, 18-30 s long); the table of rounds 1-2, and the one the MPC goldens were generated on.
The MPC's own NLP never sees how a table was made.
"""
import os

import numpy as np

from .control.compute_sets import compute_obstacles
from .engine import ProblemSpec
from .obstacle_types import GeofenceRegion
from .vehicle_types import VehicleBody, VehicleConfig

_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")
_REFS = os.path.join(_DATA, "refs_4v.npz")
_TABLES = {"state_ws": _REFS, "planned": os.path.join(_DATA, "refs_4v_planned.npz")}


def parking_lot_spec(n_nbr=3, N=30, dt=0.1, n_obs=6, dmin=0.05):
    """`ProblemSpec` of the reference's MPC (vehicle_follower.py:146) on the reference's map.
    n_obs = 4 keeps obstacles 0,1,3,4 (BASELINE.json config 2 wording)."""
    obs = compute_obstacles()
    if n_obs == 4:
        obs = [obs[i] for i in (0, 1, 3, 4)]
    elif n_obs != 6:
        obs = obs[:n_obs]
    return ProblemSpec.from_objects(obs, VehicleBody(), VehicleConfig(), GeofenceRegion(), n_nbr=n_nbr, N=N, dt=dt, dmin=dmin)


def grow_obstacles(spec: ProblemSpec, margin):
    """The obstacles of `spec` with every face moved outwards by `margin` metres (inwards if negative): (A, b + margin * |A rows|).
    The reference map's rows are unit normals, so its b moves by the margin itself."""
    A, b = np.array(spec.A_obs, float), np.array(spec.b_obs, float)
    return A, b + float(margin) * np.linalg.norm(A, axis=-1)


def shift_obstacles(spec: ProblemSpec, dx, dy):
    """The obstacles of `spec` moved by (dx, dy): {p + d : A p <= b} = {q : A q <= b + A d} -> (A, b + A (dx, dy))."""
    A, b = np.array(spec.A_obs, float), np.array(spec.b_obs, float)
    return A, b + A @ np.array([float(dx), float(dy)])


def map_spec(spec: ProblemSpec, A, b):
    """The `ProblemSpec` of a plain engine that stands on the map (A, b) and is otherwise `spec`: what a scenario of
    `Engine.loop_set_maps` on that map solves."""
    import dataclasses

    return dataclasses.replace(spec, A_obs=np.array(A, float), b_obs=np.array(b, float))


def load_reference_table(path=None, kind="state_ws"):
    """[V, T, 7] planned trajectories (x,y,psi,v,delta,a,w) sampled every dt; held at the goal.  kind: "state_ws" or "planned"
    (module docstring); `path` overrides."""
    d = np.load(path or _TABLES[kind])
    return d["table"].copy(), d["lengths"].copy()


def planned_reference_table(dt=0.1, pad=30, device=0):
    """[V, T, 7] reference table from the build's own planning chain on the GPU ("run the build's
    own single-vehicle plan for the 4 agents of the synthetic strategy once"): per vehicle `cfz_state_ws`, then the
    collocation plan `cfz_colloc` from it, evaluated every `dt` with `Vehicle.interpolate_states` (degree-5 Lagrange
    interpolant per interval, vehicle.py:722-829) and held at the goal for `pad` further samples.  Returns
    (table, lengths, info); raises RuntimeError if a plan does not converge (as the reference's IPOPT call would)."""
    import tempfile

    from . import strategy as strat
    from .control.vehicle_follower import VehicleFollower
    from .pytypes import VehicleState

    hist = strat.generate_strategy(4)
    trajs, info = [], {}
    with tempfile.TemporaryDirectory() as d:
        fn = os.path.join(d, "4v_rl_traj")
        strat.write_strategy(fn, hist)
        from .control.compute_sets import interp_along_sets
        from .vehicle_types import VehicleBody

        paths = interp_along_sets(fn, VehicleBody(), 30)
        for a in sorted(hist):
            v = VehicleFollower(rl_file_name=fn, agent=a, color={"front": (1, 0, 0), "back": (0, 1, 0)}, init_offset=VehicleState(),
                                final_heading=float(paths[a][-1, 2]))
            v.plan_single_path(spline_ws=True)
            if not getattr(v, "plan_refined", False):
                raise RuntimeError(f"collocation plan of {a} did not converge")
            t_end = float(v.reference_traj.t[-1])
            tt = np.arange(0.0, t_end + 0.5 * dt, dt)
            r = v.interpolate_states(tt)
            trajs.append(np.stack([r.x, r.y, r.psi, r.v, r.u_steer, r.u_a, r.u_steer_dot], 1))
            info[a] = dict(t_end=t_end, samples=len(tt))
    T = max(len(t) for t in trajs) + pad
    table = np.zeros((len(trajs), T, 7))
    for i, tr in enumerate(trajs):
        table[i, : len(tr)] = tr
        table[i, len(tr):, :3] = tr[-1, :3]  # goal pose held, at rest
    return table, np.array([len(t) for t in trajs]), info


def _quad_distance(P, Q):
    """Distance of convex quadrilaterals P, Q [..., 4, 2] (vertex arrays), 0 when they touch or overlap: the smallest
    vertex-to-edge distance of the two boundaries, or 0 if a vertex of one lies inside the other / two edges cross."""
    def point_edges(A, B):  # squared distance of every vertex of A to every edge of B -> [..., 4, 4]
        b0, e = B, np.roll(B, -1, axis=-2) - B
        w = A[..., :, None, :] - b0[..., None, :, :]
        t = np.clip((w * e[..., None, :, :]).sum(-1) / np.maximum((e * e).sum(-1)[..., None, :], 1e-300), 0.0, 1.0)
        d = w - t[..., None] * e[..., None, :, :]
        return (d * d).sum(-1)

    def inside(A, B):  # a vertex of A inside B (either orientation)
        e = np.roll(B, -1, axis=-2) - B
        w = A[..., :, None, :] - B[..., None, :, :]
        cr = e[..., None, :, 0] * w[..., 1] - e[..., None, :, 1] * w[..., 0]
        return ((cr >= 0).all(-1) | (cr <= 0).all(-1)).any(-1)

    def edges_cross(A, B):
        a0, a1, b0, b1 = A[..., :, None, :], np.roll(A, -1, axis=-2)[..., :, None, :], B[..., None, :, :], np.roll(B, -1, axis=-2)[..., None, :, :]
        def orient(p, q, r):
            return (q[..., 0] - p[..., 0]) * (r[..., 1] - p[..., 1]) - (q[..., 1] - p[..., 1]) * (r[..., 0] - p[..., 0])
        return ((orient(a0, a1, b0) * orient(a0, a1, b1) < 0) & (orient(b0, b1, a0) * orient(b0, b1, a1) < 0)).any((-1, -2))

    d = np.sqrt(np.minimum(point_edges(P, Q).min((-1, -2)), point_edges(Q, P).min((-1, -2))))
    return np.where(inside(P, Q) | inside(Q, P) | edges_cross(P, Q), 0.0, d)


def start_clearances(spec: ProblemSpec, table, k0, noise):
    """[S, V]: distance of every vehicle's body at its measured start state (table pose at k0 + noise) from the nearest static
    obstacle or other vehicle (0 = touching or overlapping).  A vehicle that starts closer than dmin - constr_viol_tol has an
    infeasible first NLP (status 4: the pose of stage 0 is pinned to the measured state, vehicle_follower.py:194-199, :280-290)."""
    S, V = len(k0), table.shape[0]
    x = table[np.arange(V)[None, :], np.asarray(k0)[:, None], :3] + noise[..., :3]  # [S, V, 3]
    g = np.asarray(spec.g, float)
    BV = np.array([[g[0], g[1]], [-g[2], g[1]], [-g[2], -g[3]], [g[0], -g[3]]])
    c, s_ = np.cos(x[..., 2]), np.sin(x[..., 2])
    W = x[..., None, :2] + np.stack([c[..., None] * BV[:, 0] - s_[..., None] * BV[:, 1], s_[..., None] * BV[:, 0] + c[..., None] * BV[:, 1]], -1)  # [S, V, 4, 2]
    out = np.full((S, V), np.inf)
    for j in range(spec.n_obs):  # static obstacles: vertices from the H-representation (4 half-planes, adjacent rows meet)
        A, b = np.asarray(spec.A_obs[j], float), np.asarray(spec.b_obs[j], float)
        ang = np.argsort(np.arctan2(A[:, 1], A[:, 0]))
        PV = np.array([np.linalg.solve(A[[ang[i], ang[(i + 1) % 4]]], b[[ang[i], ang[(i + 1) % 4]]]) for i in range(4)])
        out = np.minimum(out, _quad_distance(W, PV[None, None]))
    for a in range(V):
        for b_ in range(a + 1, V):
            d = _quad_distance(W[:, a], W[:, b_])
            out[:, a] = np.minimum(out[:, a], d); out[:, b_] = np.minimum(out[:, b_], d)
    return out


def start_box_excess(spec: ProblemSpec, table, k0, noise):
    """[S, V]: how far every vehicle's measured start state (table state at k0 + noise) lies OUTSIDE the boxes of the MPC's NLP on
    x, y, v, delta (vehicle_follower.py:205-240; 0 = inside).  The state of stage 0 is pinned to the measurement (:194-199) and
    bounded like every other stage, so an excess above constr_viol_tol makes the first NLP infeasible (status 4) -- e.g. a plan that
    drives at the speed limit, measured with +0.05 m/s of noise."""
    V = table.shape[0]
    x = table[np.arange(V)[None, :], np.asarray(k0)[:, None], :5] + noise  # [S, V, 5]
    b = np.asarray(spec.bounds, float).reshape(6, 2)
    out = np.zeros(x.shape[:2])
    for q, c in enumerate((0, 1, 3, 4)):
        out = np.maximum(out, np.maximum(b[q, 0] - x[..., c], x[..., c] - b[q, 1]))
    return out


def sample_scenarios(S, table, seed=2024, horizon_margin=30, noise=(0.05, 0.05, 0.02, 0.05, 0.0), spec=None, margin=0.01, box_tol=1e-2):
    """Start sample k0[S] ~ U[0, T - margin) and state noise [S, V, 5] (sigma_xy 0.05 m,
    sigma_psi 0.02 rad, sigma_v 0.05 m/s).
    spec (optional): only FEASIBLE starts -- a scenario in which some vehicle's measured state is closer than dmin - margin to an
    obstacle or to another vehicle, or outside the NLP's state boxes by more than box_tol (`start_box_excess`: round 4 found the
    planned table's vehicle 1 at the speed limit, so that half of its noisy starts were), is drawn again (start time and noise,
    same generator, up to 50 times): such a state is not one `VehicleFollower` can be in (its first NLP is infeasible, status 4).  Without spec: the draws of rounds 1-2 as they come
    (the MPC goldens and the closed-loop tests were generated on those)."""
    rng = np.random.default_rng(seed)
    V, T = table.shape[0], table.shape[1]
    k0 = rng.integers(0, max(T - horizon_margin, 1), size=S).astype(np.int32)
    nz = rng.normal(0.0, 1.0, size=(S, V, 5)) * np.asarray(noise)
    if spec is not None:
        for _ in range(50):
            bad = np.flatnonzero((start_clearances(spec, table, k0, nz).min(1) < spec.dmin - margin)
                                 | (start_box_excess(spec, table, k0, nz).max(1) > box_tol))
            if not len(bad):
                break
            k0[bad] = rng.integers(0, max(T - horizon_margin, 1), size=len(bad)).astype(np.int32)
            nz[bad] = rng.normal(0.0, 1.0, size=(len(bad), V, 5)) * np.asarray(noise)
    return k0, nz


def lane_sampler(spec: ProblemSpec, B=256, seed=1234, speed=1.0, radius=12.0):
    """BASELINE.md section 4, config 2 (SURVEY.md 8d "Config 2"): B independent single-vehicle MPC-form problems (N stages, no
    neighbours) in the lane between the two rows of parking spots: x0 ~ U[5, 30], y0 ~ U[15, 20], psi0 in {0, pi} + N(0, 0.05),
    v0 ~ U[-1, 1], delta0 = 0, `default_rng(seed)`; the reference is a straight segment (even instances) or an arc of `radius` m
    bending back towards the lane's centre line (odd instances), driven at `speed` m/s along the lane direction from the start
    position.  Returns x0 [B, 5], ref [B, 3, N], zu [B, 7, N] (warm start = the reference at the measured speed, inputs zero)."""
    rng = np.random.default_rng(seed)
    N, dt = spec.N, spec.dt
    x = rng.uniform(5.0, 30.0, B); y = rng.uniform(15.0, 20.0, B)
    lane = rng.integers(0, 2, B) * np.pi
    psi = lane + rng.normal(0.0, 0.05, B)
    v = rng.uniform(-1.0, 1.0, B)
    x0 = np.stack([x, y, psi, v, np.zeros(B)], 1)
    s_ = speed * dt * (np.arange(N) + 1.0)
    ref = np.zeros((B, 3, N)); zu = np.zeros((B, 7, N))
    for b in range(B):
        if b % 2 == 0:
            ref[b, 0] = x[b] + s_ * np.cos(lane[b]); ref[b, 1] = y[b]; ref[b, 2] = lane[b]
        else:  # an arc towards the centre line y = 17.5
            k = (1.0 if y[b] < 17.5 else -1.0) * (1.0 if lane[b] == 0.0 else -1.0) / radius
            th = lane[b] + k * s_
            ref[b, 0] = x[b] + (np.sin(th) - np.sin(lane[b])) / k; ref[b, 1] = y[b] - (np.cos(th) - np.cos(lane[b])) / k; ref[b, 2] = th
        zu[b, :3] = ref[b]; zu[b, 3] = v[b]
    return x0, ref, zu


def mpc_batch_from_table(spec: ProblemSpec, table, k0, noise):
    """Host arrays of one cold MPC step for S scenarios x V vehicles, instance order [s][v]:
    x0 [B,5], ref [B,3,N], nbr [B,V-1,3,N], zu [B,7,N] (the first `step()` of every vehicle:
    prediction = the planned trajectory incl. v, delta, a, w as `get_current_ref` seeds it
    (vehicle_follower.py:397-400), neighbours' predictions = theirs, all advanced by one)."""
    V, T, N = table.shape[0], table.shape[1], spec.N
    S = len(k0)
    B = S * V
    x0 = np.zeros((B, 5)); ref = np.zeros((B, 3, N)); nbr = np.zeros((B, V - 1, 3, N)); zu = np.zeros((B, 7, N))
    for s in range(S):
        idx = np.minimum(k0[s] + np.arange(N), T - 1)
        adv = np.minimum(np.arange(N) + 1, N - 1)
        preds = table[:, idx, :]  # [V,N,7]
        for v in range(V):
            b = s * V + v
            x0[b] = table[v, k0[s], :5] + noise[s, v]
            ref[b] = preds[v][:, :3].T
            zu[b] = preds[v][adv].T
            others = [u for u in range(V) if u != v]
            for o, u in enumerate(others):
                nbr[b, o] = preds[u][adv][:, :3].T
    return x0, ref, nbr, zu


def plan_scenarios(strategies, init_offsets=None, final_headings=None, dt=0.1, pad=30, device=0):
    """The reference tables of P strategies in one planning chain: `VehicleFollower.plan_single_path(strict=True)`
    (vehicle_follower.py:73, reference :91-138) for all P x V plans with ONE `cfz_state_ws` launch and ONE `cfz_colloc` launch
    (heterogeneous strategy lengths are one batch), each plan sampled every `dt` as `planned_reference_table` samples it and
    padded to a common length by holding the goal at rest.  `dual_ws` is skipped: `cfz_colloc` does not read the duals
    (`Vehicle.setup_single_final_problem`).
    strategies: P dicts agent -> list of {"front", "back"} (`strategy.generate_strategy`), the same V agents in each;
    init_offsets [P][V][3] (x, y, psi added to each start, as `VehicleFollower(init_offset=...)`); final_headings [P][V] or
    None (default: the heading of the last cell pair, as `planned_reference_table`).
    Returns dict(tables [P,V,T,7], lengths [P,V] (samples before the padding, 0 for a plan that failed), ws_status, ws_iters,
    colloc_status, colloc_iters [P,V] (-1: stage not run because the one before it failed), ok [P] (every plan of the strategy
    converged)).  A plan that does not converge is reported, not replaced: its rows of the table stay zero."""
    import tempfile

    from . import engine as eng
    from . import strategy as strat
    from .control.compute_sets import interp_along_sets
    from .control.vehicle import radau_points
    from .control.vehicle_follower import VehicleFollower
    from .pytypes import VehiclePrediction, VehicleState

    N_ws, K, N_per_set, shrink = 30, 5, 5, 0.5  # plan_single_path's defaults
    P = len(strategies)
    agents = sorted(strategies[0])
    V = len(agents)
    if any(sorted(h) != agents for h in strategies):
        raise ValueError("every strategy must have the same agents")
    plans = []  # (follower, init_pose, tube, guess, final_heading), [p][v] flattened
    with tempfile.TemporaryDirectory() as d:
        for p, hist in enumerate(strategies):
            fn = os.path.join(d, f"strategy_{p}")
            strat.write_strategy(fn, hist)
            paths = interp_along_sets(fn, VehicleBody(), N_ws)
            for i, a in enumerate(agents):
                off = VehicleState()
                if init_offsets is not None:
                    off.x.x, off.x.y, off.e.psi = (float(c) for c in np.asarray(init_offsets, float)[p, i, :3])
                fh = float(paths[a][-1, 2]) if final_headings is None else final_headings[p][i]
                v = VehicleFollower(rl_file_name=fn, agent=a, color={"front": (1, 0, 0), "back": (0, 1, 0)}, init_offset=off,
                                    final_heading=fh, printer=lambda *_: None)
                s0 = v.init_state
                init_pose = [s0.x.x + off.x.x, s0.x.y + off.x.y, s0.e.psi + off.e.psi]
                tube = [((st["back"].A, st["back"].b), (st["front"].A, st["front"].b)) for st in v.rl_tube[1:]]
                plans.append((v, off, init_pose, tube, paths[a], fh))
    v0 = plans[0][0]
    vc, r = v0.vehicle_config, v0.region
    bounds = [r.x_min, r.x_max, r.y_min, r.y_max, vc.v_min, vc.v_max, vc.delta_min, vc.delta_max, vc.a_min, vc.a_max, vc.w_delta_min, vc.w_delta_max]
    n = P * V
    ws_status, ws_iters = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    co_status, co_iters = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    # stage 1: every warm start in one launch (Vehicle.state_ws, vehicle.py:99-231)
    ws = eng.state_ws([q[2] for q in plans], [q[3] for q in plans], [q[4] for q in plans], [q[5] for q in plans], device=device,
                      N=N_ws, dt=dt, wb=v0.vehicle_body.wb, shrink_tube=shrink, bounded_input=0, bounds=bounds)
    fps, idx = [], []
    for b, (res, q) in enumerate(zip(ws, plans)):
        ws_status[b], ws_iters[b] = res["status"], res["iters"]
        if res["status"] != 0:
            continue
        v = q[0]
        T = N_ws * (v.num_sets - 1)
        tr = res["traj"]
        zu0 = VehiclePrediction()
        zu0.t = np.linspace(0, T * dt, T + 1, endpoint=True)
        zu0.x, zu0.y, zu0.psi, zu0.v, zu0.u_steer = (tr[:, c].copy() for c in range(5))
        zu0.u_a, zu0.u_steer_dot = tr[:, 5].copy(), tr[:, 6].copy()
        zuc = v.interp_ws_for_collocation(zu0=zu0, K=K, N_per_set=N_per_set)
        fps.append(v.setup_single_final_problem(zu0=zuc, init_offset=q[1], final_heading=q[5], K=K, N_per_set=N_per_set, shrink_tube=shrink))
        idx.append(b)
    # stage 2: every collocation plan in one launch (vehicle.py:360-661)
    sols = {}
    if fps:
        res = eng.colloc(fps[0]["spec"], [f["init_pose"] for f in fps], [f["tube"] for f in fps], [f["guess"] for f in fps],
                         [f["dt0"] for f in fps], [f["final_heading"] for f in fps], device=device, N_per_set=N_per_set, shrink_tube=shrink)
        for b, rr in zip(idx, res):
            co_status[b], co_iters[b] = rr["status"], rr["iters"]
            if rr["status"] == 0:
                sols[b] = rr
    # sampling: the collocation interpolant every dt (get_solution / get_interpolator, vehicle.py:663-829)
    tau_root = np.append(0.0, radau_points(K))
    trajs = {}
    for b, rr in sols.items():
        v = plans[b][0]
        tr, dtp = rr["traj"], float(rr["dt"])
        Nc = tr.shape[0]
        result = VehiclePrediction()
        result.t = (np.arange(Nc)[:, None] + tau_root[None, :]).ravel() * dtp
        result.x, result.y, result.psi, result.v, result.u_steer, result.u_a, result.u_steer_dot = (tr[:, :, c].ravel() for c in range(7))
        v.get_interpolator(K=K, N=Nc, dt=dtp, opt=result)
        tt = np.arange(0.0, float(result.t[-1]) + 0.5 * dt, dt)
        s_ = v.interpolate_states(tt)
        trajs[b] = np.stack([s_.x, s_.y, s_.psi, s_.v, s_.u_steer, s_.u_a, s_.u_steer_dot], 1)
    T = (max(len(t) for t in trajs.values()) if trajs else 1) + pad
    tables = np.zeros((P, V, T, 7))
    lengths = np.zeros((P, V), np.int64)
    for b, tr in trajs.items():
        p, i = divmod(b, V)
        tables[p, i, : len(tr)] = tr
        tables[p, i, len(tr):, :3] = tr[-1, :3]  # goal pose held, at rest
        lengths[p, i] = len(tr)
    sh = (P, V)
    return dict(tables=tables, lengths=lengths, ws_status=ws_status.reshape(sh), ws_iters=ws_iters.reshape(sh),
                colloc_status=co_status.reshape(sh), colloc_iters=co_iters.reshape(sh), ok=(co_status.reshape(sh) == 0).all(1))


def delay_tables(tables, delays):
    """Plan sets in which some vehicles leave late: tables [V,T,7] or [P,V,T,7] (x, y, psi, v, delta, a, w), delays whole samples >= 0,
    [V] (the same for every set) or [P,V].  Each vehicle is held for its delay at sample 0 (pose and steering angle kept, v = a = w = 0),
    then follows its plan, then repeats its last sample up to the common length T + max(delays) -> tables of that length, shaped as
    given: what `Engine.loop_init` takes.  Lag tau of `Engine.plan_conflicts` for the pair (u, w) is this with delays[w] = tau (tau > 0)
    or delays[u] = -tau, at lag 0."""
    tables = np.asarray(tables, dtype=np.float64)
    single = tables.ndim == 3
    tab = tables[None] if single else tables
    if tab.ndim != 4 or tab.shape[3] != 7 or 0 in tab.shape:
        raise ValueError(f"expected tables of shape [P, V, T, 7] or [V, T, 7], got {tables.shape}")
    P, V, T = tab.shape[:3]
    d = np.asarray(delays)
    if d.dtype.kind not in "iu":
        raise ValueError(f"delays must be whole numbers of samples, got dtype {d.dtype}")
    if d.shape not in ((V,), (P, V)):
        raise ValueError(f"delays must have shape ({V},) or ({P}, {V}), got {d.shape}")
    if (d < 0).any():
        raise ValueError("delays must not be negative")
    d = np.broadcast_to(d, (P, V))
    idx = np.clip(np.arange(T + int(d.max()))[None, None, :] - d[:, :, None], -1, T - 1)  # [P, V, T']; -1: still waiting
    out = np.take_along_axis(tab, np.maximum(idx, 0)[..., None], axis=2)
    out[..., [3, 5, 6]] = np.where((idx < 0)[..., None], 0.0, out[..., [3, 5, 6]])
    return out[0] if single else out


def _plan_sets(tables):
    """(tables as [P, V, T, 7], whether a single set [V, T, 7] was given)."""
    tables = np.asarray(tables, dtype=np.float64)
    single = tables.ndim == 3
    tab = tables[None] if single else tables
    if tab.ndim != 4 or tab.shape[3] != 7 or 0 in tab.shape:
        raise ValueError(f"expected tables of shape [P, V, T, 7] or [V, T, 7], got {tables.shape}")
    return tab, single


def plan_lengths(tables):
    """The length of every plan of tables [V,T,7] or [P,V,T,7] that are held at their last pose to a common T: the first sample from
    which the pose (x, y, psi) no longer changes, plus one -> int32 [V] or [P,V], in [1, T].  What `Engine.plan_schedule` takes as
    `length`: the goal sample is length - 1, what lies beyond is padding."""
    tab, single = _plan_sets(tables)
    T = tab.shape[2]
    moved = (tab[:, :, :, :3] != tab[:, :, -1:, :3]).any(-1)  # [P, V, T]: the pose differs from the last one
    last = np.where(moved.any(-1), T - 1 - np.argmax(moved[:, :, ::-1], axis=-1), -1)  # the last sample that differs, -1: none
    out = (last + 2).astype(np.int32)
    return out[0] if single else out


def hold_points(tables, v_tol=0.1, length=None):
    """Where the vehicles of tables [V,T,7] or [P,V,T,7] may wait: sample 0, every sample with |v| <= v_tol (a parking manoeuvre rests at
    each change of direction) and everything from the goal sample length - 1 on (length None: `plan_lengths(tables)`) -> uint8 of shape
    [V,T] or [P,V,T], what `Engine.plan_schedule` takes as `hold`."""
    tab, single = _plan_sets(tables)
    P, V, T = tab.shape[:3]
    n = plan_lengths(tab) if length is None else np.broadcast_to(np.asarray(length), (P, V))
    hold = np.abs(tab[..., 3]) <= v_tol
    hold[:, :, 0] = True
    hold |= np.arange(T)[None, None, :] >= (n[:, :, None] - 1)
    hold = hold.astype(np.uint8)
    return hold[0] if single else hold


def schedule_tables(tables, schedule):
    """Plan sets driven along a schedule of `Engine.plan_schedule`: tables [V,T,7] or [P,V,T,7], schedule whole samples [V,H] or [P,V,H],
    non-decreasing in t.  Row t of vehicle v is its row schedule[v, t]; where the vehicle is held (the next row is the same sample, and
    it is not the schedule's last sample, the goal) v = a = w = 0 with the pose and the steering angle kept; rows at the goal are
    copies -> tables of length H, shaped as given: what `Engine.loop_init` takes.  For a schedule that is a start delay,
    schedule[v, t] = clip(t - d[v], 0, T - 1), this is `delay_tables(tables, d)`."""
    tab, single = _plan_sets(tables)
    P, V, T = tab.shape[:3]
    s = np.asarray(schedule)
    if s.dtype.kind not in "iu":
        raise ValueError(f"schedule must hold whole samples, got dtype {s.dtype}")
    if single and s.ndim == 2:
        s = s[None]
    if s.ndim != 3 or s.shape[:2] != (P, V) or s.shape[2] == 0:
        raise ValueError(f"schedule must have shape ({P}, {V}, H), got {np.asarray(schedule).shape}")
    if (s < 0).any() or (s >= T).any() or (np.diff(s, axis=2) < 0).any():
        raise ValueError("schedule must hold samples in [0, T) that do not decrease (a set without an answer has none)")
    out = np.take_along_axis(tab, s[..., None].astype(np.int64), axis=2)
    held = np.zeros(s.shape, bool)
    held[:, :, :-1] = (s[:, :, 1:] == s[:, :, :-1]) & (s[:, :, :-1] < s[:, :, -1:])
    out[..., [3, 5, 6]] = np.where(held[..., None], 0.0, out[..., [3, 5, 6]])
    return out[0] if single else out


def distinct_strategies(n_vehicles=4, delays=(0, 1, 2)):
    """The distinct strategies `strategy.generate_strategy` gives over every priority order x start delays in delays^n (infeasible
    combinations skipped), in the order first met.  Returns (strategies, combos): combos[i] lists the (order, delays) that give
    strategy i."""
    from itertools import permutations, product

    from . import strategy as strat

    seen, out, combos = {}, [], []
    for order in permutations(range(n_vehicles)):
        for dl in product(delays, repeat=n_vehicles):
            try:
                h = strat.generate_strategy(n_vehicles, list(order), list(dl))
            except RuntimeError:
                continue
            key = repr(sorted((a, [sorted(c.items()) for c in h[a]]) for a in h))
            if key not in seen:
                seen[key] = len(out)
                out.append(h)
                combos.append([])
            combos[seen[key]].append((order, dl))
    return out, combos
