"""Oracle (test infrastructure): the closed loop of `MultiDistributedFollower.solve` (reference
confrez/control/vehicle_follower.py:630-663) replayed on the host with the plain-C port of the solver.

Per MPC iteration and scenario: every vehicle's prediction is copied first (Jacobi exchange, :636-637), then every
vehicle steps (:642-647): `_adv_onestep` shift of its own and its neighbours' predictions (:413-426, :444-476), solve
(:479) started from the multipliers its previous solve left (`cfz_port_solve_carry`; the reference hands the old duals
to `opti.set_initial`, :458-464), read-back (:484-500) or shift fallback (:501-524), plant over dt (:528-543).

`step_inputs` is the one host statement of what a solve is fed; `replay` is the one loop around it, with the sequential exchange
(`order`), the disturbances (`d`) and the lossy exchange (`comm`) of the device loop as options.

Used by the GPU tests (the device loop must reproduce it solve by solve) and by bench.py's `cpu_baseline` leg (the same workload
timed on the host cores).  Never imported by the product package.
"""
import numpy as np

from . import port
from .dynamics import plant_step
from .mpc_nlp import MpcSpec


def seed(table, k0, noise, N, table_of=None):
    """State and first prediction of every (scenario, vehicle) as `get_current_ref` seeds them (:397-400).  table [V,T,7], or a pool
    [P,V,T,7] with table_of [S]."""
    S = len(k0)
    V, T = table.shape[-3], table.shape[-2]
    state = np.zeros((S, V, 5)); pred = np.zeros((S, V, 7, N))
    for s in range(S):
        tab = table if table_of is None else table[table_of[s]]
        for v in range(V):
            pred[s, v] = tab[v, np.minimum(k0[s] + np.arange(N), T - 1), :].T
            state[s, v] = tab[v, k0[s], :5] + noise[s, v]
    return state, pred


def step_inputs(table, k, state, pred, v, new_pred=None, before=(), read=None):
    """Inputs of vehicle v's solve in one iteration of one scenario: (measured state [5], reference window [3,N], neighbours [V-1,3,N],
    shifted warm start [7,N]).  table [V,T,7]: the scenario's plans, k its clock (k0 + t); state [V,5], pred [V,7,N]: before the step.
    Sequential exchange: the vehicles in `before` (ranked before v) are read from new_pred [V,7,N], this step's predictions, unshifted.
    read(u, earlier) -> (message [7,N], rows [N]): what v reads of neighbour u instead (a lossy exchange; `replay`)."""
    V, T, N = table.shape[0], table.shape[1], pred.shape[-1]
    adv = np.minimum(np.arange(N) + 1, N - 1)
    kr = np.minimum(k + np.arange(N), T - 1)
    if read is None:
        def read(u, earlier):
            return (new_pred[u], np.arange(N)) if earlier else (pred[u], adv)
    nb = []
    for u in range(V):
        if u != v:
            msg, rows = read(u, u in before)
            nb.append(msg[:3][:, rows])
    return state[v], table[v, kr, :3].T, np.stack(nb) if nb else np.zeros((0, 3, N)), pred[v][:, adv]


def replay(ospec: MpcSpec, table, k0, noise, steps, dt=0.1, wb=2.5, carry_duals=True, opt=None, *, order=None, d=None, box=None,
           table_of=None, comm=None, ages=None):
    """Generator: after every iteration yields (state [S,V,5], pred [S,V,7,N], status [S,V], iters [S,V]).
    ospec, opt: one MpcSpec and one IpmOptions (or None) for the batch, or a sequence of S of either: scenario s is solved with its own
    entry (the device's problem and map pools); specs that differ in N or n_nbr are refused, as the device refuses them.
    order [S,V]: the sequential exchange, scenario s steps its vehicles in the order order[s] (None: Jacobi).  d [K,S,V,12]: the device's
    disturbances (`Engine.loop_disturbance`) with box [2,2], the bounds of (a, w): the solver sees state + d[0:5], the plant takes
    clip(input + d[5:7]) from the true state, d[7:12] is added to what it returns.  table_of [S]: `table` is a pool [P,V,T,7].
    comm(t) -> the lossy exchange in force in iteration t, or None (comm None: never any).  The loop then keeps the history of
    messages (message tau is the prediction array after iteration tau; tau = -1: the seed; iteration t's own messages are read by the
    vehicles ranked later in it) and asks the setting one question per neighbour, `read(t, s, v, u, earlier, N) -> (tau, rows [N])`:
    the message vehicle v takes of neighbour u and the rows it reads of it; lossless, that is (t - 1, advanced), or (t, as it stands)
    of a neighbour ranked `earlier`.  ages (a list, or None) receives (t, s, v, u, age) of every such read."""
    S, V = len(k0), table.shape[-3]
    specs = [ospec] * S if isinstance(ospec, MpcSpec) else list(ospec)
    opts = list(opt) if isinstance(opt, (list, tuple)) else [opt] * S
    N = specs[0].N
    if len(specs) != S or len(opts) != S or any((sp.N, sp.n_nbr) != (N, specs[0].n_nbr) for sp in specs):
        raise ValueError(f"replay: {S} scenarios take one spec and one options entry each, the specs equal in N and n_nbr")
    state, pred = seed(table, k0, noise, N, table_of)
    hist = {-1: pred}
    carry = [[None] * V for _ in range(S)]
    kws = [{} if o is None else {"opt": o} for o in opts]
    for t in range(steps):
        cm = None if comm is None else comm(t)
        newp = hist[t] = pred.copy()
        status = np.zeros((S, V), int); iters = np.zeros((S, V), int)
        for s in range(S):
            tab = table if table_of is None else table[table_of[s]]
            done = []  # (stays empty under Jacobi)
            for v in (range(V) if order is None else order[s]):
                read = None
                if cm is not None:
                    def read(u, earlier):
                        tau, rows = cm.read(t, s, v, u, earlier, N)
                        if ages is not None:
                            ages.append((t, s, v, u, (t if earlier else t - 1) - tau))
                        return hist[tau][s, u], rows
                x0, ref, nb, w = step_inputs(tab, k0[s] + t, state[s], pred[s], v, newp[s], done, read)
                dd = None if d is None else d[t, s, v]
                r = port.solve(specs[s], x0 if dd is None else x0 + dd[:5], ref, nb, w.T.copy(), **kws[s], carry=carry[s][v] if carry_duals else None)
                carry[s][v] = r["carry"]
                newp[s, v] = r["p"].T if r["status"] == 0 else w
                u = newp[s, v][5:7, 0] if dd is None else np.clip(newp[s, v][5:7, 0] + dd[5:7], box[:, 0], box[:, 1])
                state[s, v] = plant_step(state[s, v], u, dt, wb)
                if dd is not None:
                    state[s, v] += dd[7:12]
                status[s, v], iters[s, v] = r["status"], r["iters"]
                if order is not None:
                    done.append(v)
        pred = newp
        if comm is None:
            del hist[t - 1]  # (nothing reads further back than the previous iteration)
        yield state.copy(), pred.copy(), status, iters
