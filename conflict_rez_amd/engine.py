"""ctypes binding of libconfrez_hip.so (C ABI: include/confrez_hip.h).

This is the only place the Python package touches the solver.  There is no CPU fallback:
if the HIP library is missing or no GPU is visible, construction raises.
"""
import ctypes as C
import itertools
import os
from dataclasses import dataclass, field

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libconfrez_hip.so")
MAX_OBS, MAX_NBR, MAX_N = 8, 7, 32

STATUS_NAMES = {0: "converged", 1: "iteration limit", 2: "line search failed", 3: "non-finite iterate",
                4: "measured state in collision (infeasible)", 5: "constraint violation stalled (locally infeasible)"}


class _CSpec(C.Structure):
    _fields_ = [
        ("N", C.c_int32), ("n_obs", C.c_int32), ("n_nbr", C.c_int32), ("rk_substeps", C.c_int32),
        ("dt", C.c_double), ("wb", C.c_double), ("dmin", C.c_double),
        ("g", C.c_double * 4), ("bounds", C.c_double * 12), ("weights", C.c_double * 6),
        ("A_obs", C.c_double * (MAX_OBS * 8)), ("b_obs", C.c_double * (MAX_OBS * 4)),
    ]


_OPT_INTS = ("max_iter", "max_backtrack", "filter_cap", "stall_iters", "row_curvature", "carry_duals", "vv_rows", "shift_after", "restoration", "shift_stagnation", "err_stall_iters", "carry_shift")
_OPT_DBLS = ("tol constr_viol_tol dual_inf_tol compl_inf_tol mu_init kappa_eps kappa_mu theta_mu tau_min bound_push "
             "bound_frac s_max kappa_sigma eta_phi gamma_theta gamma_phi delta_sw s_theta s_phi reg_primal stall_kappa warm_push reg_dual_rows resto_first").split()


KERNEL_AUTO, KERNEL_WIDE, KERNEL_NARROW = 0, 1, 2  # cfz_plan_options.kernel / cfz_colloc_options.kernel (include/confrez_hip.h)


class _CPlanOptions(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("N", "max_iter", "bounded_input", "stall_iters", "kernel", "reserved0")] + [
        ("dt", C.c_double), ("wb", C.c_double), ("shrink_tube", C.c_double), ("bounds", C.c_double * 12),
        ("tol", C.c_double), ("constr_viol_tol", C.c_double), ("mu_init", C.c_double), ("curv_kappa", C.c_double)]


class _CCollocOptions(C.Structure):
    _fields_ = [("N_per_set", C.c_int32), ("max_iter", C.c_int32), ("exact_rows", C.c_int32), ("one_pivot", C.c_int32), ("vv_rows", C.c_int32), ("kernel", C.c_int32),
                ("shrink_tube", C.c_double),
                ("tol", C.c_double), ("constr_viol_tol", C.c_double), ("mu_init", C.c_double), ("curv_kappa", C.c_double),
                ("structured", C.c_int32), ("reserved1", C.c_int32)]


class _COptions(C.Structure):
    _fields_ = [(k, C.c_int32) for k in _OPT_INTS] + [(k, C.c_double) for k in _OPT_DBLS]


@dataclass
class ProblemSpec:
    """Constants of the MPC-step NLP (`cfz_spec`); defaults are the reference's
    (`VehicleFollower.setup_controller`, `VehicleBody`, `VehicleConfig`, `GeofenceRegion`)."""

    N: int = 30
    dt: float = 0.1
    n_nbr: int = 3
    A_obs: np.ndarray = field(default_factory=lambda: np.zeros((0, 4, 2)))
    b_obs: np.ndarray = field(default_factory=lambda: np.zeros((0, 4)))
    g: np.ndarray = field(default_factory=lambda: np.array([3.3, 0.9, 0.6, 0.9]))
    wb: float = 2.5
    bounds: np.ndarray = field(
        default_factory=lambda: np.array([2.5, 32.5, 7.5, 27.5, -2.5, 2.5, -0.85, 0.85, -1.5, 1.5, -1.0, 1.0])
    )
    dmin: float = 0.05
    weights: np.ndarray = field(default_factory=lambda: np.array([100.0, 100, 100, 1, 1, 1]))
    rk_substeps: int = 4

    @property
    def n_obs(self):
        return int(np.asarray(self.A_obs).shape[0])

    @classmethod
    def from_objects(cls, obstacles, vehicle_body, vehicle_config, region, n_nbr, N=30, dt=0.1, dmin=0.05):
        """From the reference-style objects (`Polytope` list, `VehicleBody`, `VehicleConfig`, `GeofenceRegion`)."""
        vc, r = vehicle_config, region
        return cls(
            N=N, dt=dt, n_nbr=n_nbr, dmin=dmin, wb=vehicle_body.wb, g=np.asarray(vehicle_body.b, float),
            A_obs=np.stack([o.A for o in obstacles]) if obstacles else np.zeros((0, 4, 2)),
            b_obs=np.stack([o.b for o in obstacles]) if obstacles else np.zeros((0, 4)),
            bounds=np.array([r.x_min, r.x_max, r.y_min, r.y_max, vc.v_min, vc.v_max, vc.delta_min, vc.delta_max,
                             vc.a_min, vc.a_max, vc.w_delta_min, vc.w_delta_max], float),
        )

    def to_c(self):
        if self.n_obs > MAX_OBS or self.n_nbr > MAX_NBR or self.N > MAX_N:
            raise ValueError("problem exceeds the engine's compiled limits")
        s = _CSpec()
        s.N, s.n_obs, s.n_nbr, s.rk_substeps = self.N, self.n_obs, self.n_nbr, self.rk_substeps
        s.dt, s.wb, s.dmin = self.dt, self.wb, self.dmin
        s.g[:] = [float(v) for v in self.g]
        s.bounds[:] = [float(v) for v in self.bounds]
        s.weights[:] = [float(v) for v in self.weights]
        A = np.zeros((MAX_OBS, 4, 2)); b = np.zeros((MAX_OBS, 4))
        if self.n_obs:
            A[: self.n_obs], b[: self.n_obs] = self.A_obs, self.b_obs
        s.A_obs[:] = list(A.ravel()); s.b_obs[:] = list(b.ravel())
        return s


_lib = None

ABI_VERSION = 6  # CFZ_ABI_VERSION of include/confrez_hip.h

_i, _d, _vp, _P = C.c_int, C.c_double, C.c_void_p, C.POINTER
_h = _ws = _vp  # cfz_handle *, cfz_plan_ws *: opaque
_spec, _opt, _popt, _copt = _P(_CSpec), _P(_COptions), _P(_CPlanOptions), _P(_CCollocOptions)

# The binding's one statement of include/confrez_hip.h: every function of the header, in its order, name -> (restype, argtypes).
# tests/test_abi.py parses the header and holds each row to its prototype (count and type of every parameter).
PROTOTYPES = {
    "cfz_default_spec": (None, [_spec]),
    "cfz_default_options": (None, [_opt]),
    "cfz_create": (_i, [_spec, _opt, _i, _i, _P(_vp)]),
    "cfz_destroy": (_i, [_h]),
    "cfz_max_batch": (_i, [_h]),
    "cfz_kernel_info": (_i, [_h, _vp, _vp]),
    "cfz_mpc_set_params": (_i, [_h, _i, _vp, _vp, _vp]),
    "cfz_mpc_set_warm": (_i, [_h, _i, _vp]),
    "cfz_mpc_set_carry": (_i, [_h, _i, _vp]),
    "cfz_mpc_set_carry_device": (_i, [_h, _i, _vp]),
    "cfz_mpc_set_slots": (_i, [_h, _i, _vp]),
    "cfz_mpc_solve": (_i, [_h, _i]),
    "cfz_mpc_get": (_i, [_h, _i] + [_vp] * 6),
    "cfz_mpc_stats": (_i, [_h, _i] + [_vp] * 5),
    "cfz_last_solve_ms": (_d, [_h]),
    "cfz_mpc_solve_device": (_i, [_h, _i] + [_vp] * 8),
    "cfz_vsl_step": (_i, [_h, _i, _i, _i, _vp, _i, _vp, _vp, _i] + [_vp] * 8),
    "cfz_dual_ws": (_i, [_h, _i] + [_vp] * 4),
    "cfz_joint_dual_ws": (_i, [_h, _i] + [_vp] * 6),
    "cfz_default_plan_options": (None, [_popt]),
    "cfz_plan_ws_create": (_i, [_i, _P(_vp)]),
    "cfz_plan_ws_destroy": (_i, [_ws]),
    "cfz_plan_ws_trim": (_i, [_ws]),
    "cfz_state_ws_w": (_i, [_ws, _i, _popt] + [_vp] * 9),
    "cfz_state_ws": (_i, [_i, _i, _popt] + [_vp] * 9),
    "cfz_state_ws_default_guess": (_i, [C.c_int32, C.c_int32, _vp, _d, _vp, _vp]),
    "cfz_default_colloc_options": (None, [_copt]),
    "cfz_colloc_w": (_i, [_ws, _i, _spec, _copt] + [_vp] * 11),
    "cfz_colloc": (_i, [_i, _i, _spec, _copt] + [_vp] * 11),
    "cfz_joint_colloc_w": (_i, [_ws, _i, _i, _spec, _copt] + [_vp] * 6 + [_i] + [_vp] * 6),
    "cfz_joint_colloc": (_i, [_i, _i, _i, _spec, _copt] + [_vp] * 6 + [_i] + [_vp] * 6),
    "cfz_colloc_band_info": (_i, [_i, _vp, _vp, _i, _i, _i] + [_vp] * 4),
    "cfz_colloc_elimination_info": (_i, [_i, _vp, _vp, _i, _i, _i, _vp, _i] + [_vp] * 5),
    "cfz_abi_version": (_i, []),
    "cfz_loop_init": (_i, [_h, _i, _i, _vp, _vp, _vp]),
    "cfz_loop_step": (_i, [_h]),
    "cfz_loop_run": (_i, [_h, _i]),
    "cfz_loop_last_iterations": (C.c_long, [_h]),
    "cfz_loop_last_converged": (C.c_long, [_h]),
    "cfz_loop_last_status_counts": (_i, [_h, _vp]),
    "cfz_loop_get": (_i, [_h] + [_vp] * 4),
    "cfz_loop_set_order": (_i, [_h, _vp]),
    "cfz_loop_set_disturbance": (_i, [_h, C.c_uint64] + [_vp] * 5),
    "cfz_loop_disturbance": (_i, [_h, _i, _i, _vp]),
    "cfz_loop_set_comm": (_i, [_h, C.c_uint64, _vp, _i, _i, _vp]),
    "cfz_loop_comm": (_i, [_h, _i, _i, _vp]),
    "cfz_problem_check": (_i, [_spec, _opt, _spec, _opt]),
    "cfz_loop_set_problems": (_i, [_h, _i, _vp, _vp, _vp]),  # (arrays of cfz_spec and cfz_options, passed raw)
    "cfz_map_check": (_i, [_spec, _vp, _vp]),
    "cfz_loop_set_maps": (_i, [_h, _i, _vp, _vp, _vp]),
    "cfz_loop_init_tables": (_i, [_h, _i, _i, _i] + [_vp] * 4),
    "cfz_loop_record": (_i, [_h, _i]),
    "cfz_loop_history": (_i, [_h, _i, _i, _vp, _vp, _vp]),
    "cfz_loop_audit": (_i, [_h, _i, _i, _d, _d, _d] + [_vp] * 4),
    "cfz_audit": (_i, [_h, _i, _i, _i, _vp, _vp, _d, _d, _d] + [_vp] * 4),
    "cfz_audit_maps": (_i, [_h, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _d, _d, _d] + [_vp] * 4),
    "cfz_loop_score": (_i, [_h, _i, _i, _d, _d, _d, _d, _vp, _vp]),
    "cfz_score": (_i, [_h, _i, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _d, _d, _d, _d, _vp, _vp]),
    "cfz_plan_conflicts": (_i, [_h, _i, _i, _i, _vp, _i, _d, _vp, _vp]),
    "cfz_loop_plan_conflicts": (_i, [_h, _i, _d, _vp, _vp]),
    "cfz_delay_search": (_i, [_h, _i, _i, _i, _vp, _vp, _i] + [_vp] * 4),
    "cfz_plan_delays": (_i, [_h, _i, _i, _i, _vp, _i, _d, _i] + [_vp] * 4),
    "cfz_loop_plan_delays": (_i, [_h, _i, _d, _i] + [_vp] * 4),
    "cfz_plan_coordination": (_i, [_h, _i, _i, _i, _vp, _vp, _d, _vp]),
    "cfz_plan_schedule": (_i, [_h, _i, _i, _i, _vp, _vp, _vp, _i, _d, _i, _i] + [_vp] * 5),
    "cfz_loop_plan_schedule": (_i, [_h, _vp, _vp, _i, _d, _i, _i] + [_vp] * 5),
    "cfz_last_error": (C.c_char_p, []),
    "cfz_source_hash": (C.c_char_p, []),
}
EXPORTS = tuple(PROTOTYPES)


def load_library(path=None):
    """Loads libconfrez_hip.so and binds every row of PROTOTYPES.  The package's own library must export them all; one named by `path`
    or CFZ_LIBRARY (a diagnostic build, another commit's build: tools/) may lack some, which then stay unbound."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    own = not (path or os.environ.get("CFZ_LIBRARY"))
    path = path or os.environ.get("CFZ_LIBRARY") or LIB_PATH
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). conflict_rez_amd has no CPU solver."
        )
    lib = C.CDLL(path)
    # the struct mirrors above have the layout of this version of the header: a library of another version would read shorter structs
    version = lib.cfz_abi_version() if hasattr(lib, "cfz_abi_version") else "none"
    if version != ABI_VERSION:
        raise RuntimeError(f"{path}: struct layout version {version}, this binding is written against {ABI_VERSION}: rebuild the library")
    missing = []
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            missing.append(name)
        else:
            fn.restype, fn.argtypes = restype, argtypes
    if missing and own:
        raise RuntimeError(f"{path} lacks symbols {missing}")
    _lib = lib
    return lib


# tolerances of the audit's arrival test (`Engine.loop_audit`, `Engine.audit`): position [m], heading [rad], speed [m/s]
ARRIVE_TOL = dict(pos_tol=0.3, psi_tol=0.1, v_tol=0.1)

# columns of the score's raw arrays, in the order of include/confrez_hip.h (CFZ_SCORE_NVAL, CFZ_SCORE_NCNT)
SCORE_VAL = ("dx2", "dy2", "psi2", "a2", "vw2", "delta2", "da2", "dw2", "absv", "dev2_max")
SCORE_CNT = ("steps", "arrive", "failed", "fail_run", "reversals", "waiting", "near_steps", "first_near", "iters_sum", "iters_max", "dev_max_step")


def score_summary(val, cnt, dt, weights):
    """The score of a closed loop from the raw arrays of `cfz_loop_score` / `cfz_score`: val [S,V,10], cnt [S,V,11], the time step dt
    and the six weights of the reference's objective (`ProblemSpec.weights`: x, y, psi, a, v w, delta), [6] or one row per scenario [S,6]
    -> dict of every column by name (`SCORE_VAL`, `SCORE_CNT`), each [S,V], and
    cost = weights . (dx2, dy2, psi2, a2, vw2, delta2); track_rms = sqrt((dx2 + dy2) / steps), track_max = sqrt(dev2_max) [m];
    time = dt steps, distance = dt absv, wait = dt waiting."""
    val, cnt = np.asarray(val, dtype=np.float64), np.asarray(cnt)
    if val.ndim != 3 or val.shape[2] != len(SCORE_VAL) or cnt.shape != val.shape[:2] + (len(SCORE_CNT),):
        raise ValueError(f"expected val [S, V, {len(SCORE_VAL)}] and cnt [S, V, {len(SCORE_CNT)}], got {val.shape} and {cnt.shape}")
    S = val.shape[0]
    w = np.asarray(weights, dtype=np.float64)
    if w.shape not in ((6,), (S, 6)):
        raise ValueError(f"weights must have shape (6,) or ({S}, 6), got {w.shape}")
    w = np.broadcast_to(w, (S, 6))
    out = {name: val[..., i] for i, name in enumerate(SCORE_VAL)}
    out.update({name: cnt[..., i] for i, name in enumerate(SCORE_CNT)})
    out["cost"] = (val[..., :6] * w[:, None, :]).sum(-1)
    out["track_rms"] = np.sqrt((out["dx2"] + out["dy2"]) / out["steps"])
    out["track_max"] = np.sqrt(out["dev2_max"])
    out["time"] = dt * out["steps"]
    out["distance"] = dt * out["absv"]
    out["wait"] = dt * out["waiting"]
    return out


def _score_args(near, tol):
    """(pos_tol, psi_tol, v_tol, near) of a score call as floats: the tolerances default to ARRIVE_TOL, unknown names are refused."""
    unknown = set(tol) - set(ARRIVE_TOL)
    if unknown:
        raise TypeError(f"unknown tolerance(s) {sorted(unknown)}: expected {sorted(ARRIVE_TOL)}")
    t = {**ARRIVE_TOL, **tol}
    return float(t["pos_tol"]), float(t["psi_tol"]), float(t["v_tol"]), float(near)


def _conflict_args(max_lag, margin, spec):
    """(D, margin) of a conflict-map call: the window as a non-negative int, margin None meaning the problem's `dmin`."""
    D = int(max_lag)
    if D != max_lag or D < 0:
        raise ValueError(f"max_lag must be a non-negative whole number of samples, got {max_lag!r}")
    return D, float(spec.dmin if margin is None else margin)


def _conflict_out(P, V, D):
    """The raw arrays of `cfz_plan_conflicts` / `cfz_loop_plan_conflicts`: clear [P, npair, 2D+1], info [P, npair, 2D+1, 3]."""
    npair = V * (V - 1) // 2
    return np.full((P, npair, 2 * D + 1), np.inf), np.full((P, npair, 2 * D + 1, 3), -1, np.int32)


def _conflict_dict(clear, info, V, D):
    pairs = np.array([(u, w) for u in range(V) for w in range(u + 1, V)], np.int32).reshape(-1, 2)
    return dict(clear=clear, when=info[..., 0], first=info[..., 1], count=info[..., 2], pairs=pairs, lags=np.arange(-D, D + 1, dtype=np.int32))


def _delay_args(slack, cap, P, V, D):
    """(slack, cap) of a delay search: the slack as a non-negative int; cap None, or [V] (every set's) or [P, V] whole numbers in
    [0, D] as a contiguous int32 [P, V]."""
    r = int(slack)
    if r != slack or r < 0:
        raise ValueError(f"slack must be a non-negative whole number of samples, got {slack!r}")
    if cap is None:
        return r, None
    c = np.asarray(cap)
    if c.shape not in ((V,), (P, V)):
        raise ValueError(f"expected cap of shape [{V}] or [{P}, {V}], got {c.shape}")
    ci = c.astype(np.int32)
    if c.size and (not (ci == c).all() or ci.min() < 0 or ci.max() > D):
        raise ValueError(f"cap must hold whole numbers in [0, {D}]")
    return r, np.ascontiguousarray(np.broadcast_to(ci, (P, V)))


def _delay_out(P, V):
    """The raw arrays of the delay entry points: delays [P, V], info [P, 3], rclear [P] (NaN where the library does not write it)."""
    return np.full((P, V), -1, np.int32), np.full((P, 3), -1, np.int32), np.full(P, np.nan)


def _delay_dict(delays, info, rclear):
    return dict(delays=delays, found=info[:, 0] == 1, span=info[:, 1], total=info[:, 2], clear=rclear)


def _length_arg(length, P, V):
    """length None, or [V] (every set's) or [P, V] whole numbers as a contiguous int32 [P, V] (the library checks the range)."""
    if length is None:
        return None
    n = np.asarray(length)
    if n.shape not in ((V,), (P, V)) or n.dtype.kind not in "iu":
        raise ValueError(f"expected whole numbers length of shape [{V}] or [{P}, {V}], got {n.dtype} {n.shape}")
    return np.ascontiguousarray(np.broadcast_to(n.astype(np.int32), (P, V)))


def _schedule_args(hold, horizon, margin, slack, orders, length, P, V, T, spec):
    """(hold, H, margin, slack, orders, length) of a schedule call on P sets x V vehicles x T samples: hold [V, T] (every set's) or
    [P, V, T], non-zero where a vehicle may wait, as contiguous uint8; horizon None: T + 64; margin None: the problem's `dmin`; orders
    None: every permutation in `itertools.permutations` order for V <= 4, else [O, V] or one order [V], as contiguous int32."""
    hold = np.asarray(hold)
    if hold.shape not in ((V, T), (P, V, T)):
        raise ValueError(f"expected hold of shape [{V}, {T}] or [{P}, {V}, {T}], got {hold.shape}")
    hold = np.ascontiguousarray(np.broadcast_to(hold != 0, (P, V, T)), dtype=np.uint8)
    H = T + 64 if horizon is None else int(horizon)
    if horizon is not None and H != horizon:
        raise ValueError(f"horizon must be a whole number of samples, got {horizon!r}")
    r = int(slack)
    if r != slack or r < 0:
        raise ValueError(f"slack must be a non-negative whole number of samples, got {slack!r}")
    if orders is None:
        if V > 4:
            raise ValueError(f"orders is required for more than 4 vehicles ({V}! orders are not searched by default): pass a list [O, {V}]")
        orders = list(itertools.permutations(range(V)))
    o = np.asarray(orders)
    if o.ndim == 1:
        o = o[None]
    if o.ndim != 2 or o.shape[1] != V or o.shape[0] == 0 or o.dtype.kind not in "iu":
        raise ValueError(f"expected whole numbers orders of shape [O, {V}], got {o.dtype} {o.shape}")
    return hold, H, float(spec.dmin if margin is None else margin), r, np.ascontiguousarray(o, dtype=np.int32), _length_arg(length, P, V)


def _schedule_out(P, V, H):
    """The raw arrays of the schedule entry points: schedule [P, V, H], arrival [P, V], waits [P, V], info [P, 5]."""
    return np.full((P, V, H), -1, np.int32), np.full((P, V), -1, np.int32), np.full((P, V), -1, np.int32), np.full((P, 5), -1, np.int32)


def _schedule_dict(schedule, arrival, waits, info):
    return dict(schedule=schedule, arrival=arrival, waits=waits, found=info[:, 0] == 1, order=info[:, 1], makespan=info[:, 2], total=info[:, 3],
                feasible_orders=info[:, 4])


def conflict_summary(out):
    """What a conflict map (`Engine.plan_conflicts`, `Engine.loop_plan_conflicts`) says about every plan set, pure numpy.
    Per (set, pair) [P, npair]: clear0, the clearance at lag 0; slack_late, the largest m in [0, D] with count == 0 at every lag in
    [0, m] (how many samples the pair's second vehicle may run late before the plans come within the margin), -1 if lag 0 itself is in
    conflict; slack_early, likewise on [-m, 0] (the first vehicle late).  Per set [P]: depth = max(0, -min over pairs of clear0), the
    planned penetration at lag 0; slack, the minimum over pairs of the smaller of slack_late and slack_early; critical_pair [P, 2], the
    (first) pair that sets it.  Without pairs (V = 1): depth 0, slack D, critical_pair (-1, -1)."""
    clear, count, pairs = np.asarray(out["clear"], dtype=np.float64), np.asarray(out["count"]), np.asarray(out["pairs"])
    if clear.ndim != 3 or clear.shape[2] % 2 != 1 or count.shape != clear.shape or pairs.shape != (clear.shape[1], 2):
        raise ValueError(f"expected clear, count [P, npair, 2D+1] and pairs [npair, 2], got {clear.shape}, {count.shape} and {pairs.shape}")
    P, npair, D = clear.shape[0], clear.shape[1], clear.shape[2] // 2
    free = count == 0
    res = dict(clear0=clear[..., D],
               slack_late=np.cumprod(free[..., D:], axis=-1).sum(-1).astype(np.int64) - 1,
               slack_early=np.cumprod(free[..., D::-1], axis=-1).sum(-1).astype(np.int64) - 1)
    if npair == 0:
        res.update(depth=np.zeros(P), slack=np.full(P, D, np.int64), critical_pair=np.full((P, 2), -1, np.int32))
        return res
    pair_slack = np.minimum(res["slack_late"], res["slack_early"])
    crit = pair_slack.argmin(1)
    res.update(depth=np.maximum(0.0, -res["clear0"].min(1)), slack=pair_slack.min(1), critical_pair=pairs[crit])
    return res


def _options(struct_type, default_fn_name, what, options):
    """The library's defaults of one of its option structs with the overrides `options` applied (an array field element by element);
    a name the struct does not have is refused, not dropped."""
    o = struct_type()
    getattr(load_library(), default_fn_name)(C.byref(o))
    for k, v in options.items():
        if not hasattr(o, k):
            raise TypeError(f"unknown {what} option {k!r}")
        if isinstance(getattr(o, k), C.Array):
            getattr(o, k)[:] = [float(x) for x in v]
        else:
            setattr(o, k, v)
    return o


def default_options(**overrides):
    return _options(_COptions, "cfz_default_options", "solver", overrides)


def problem_check(base, spec, base_options=None, **options):
    """`cfz_problem_check`: may `spec` stand in a problem pool (`Engine.loop_set_problems`) of an engine created with `base` and the
    default options changed by the dict `base_options`?  `options` are the entry's overrides, applied to the engine's options as
    `loop_set_problems` applies them.  Host arithmetic, needs no GPU.  Raises ValueError with the library's text, which names the first
    field that differs from the handle (geometry, time base, carry_duals) or is invalid.  `Engine.problem_check` passes its own."""
    lib = load_library()
    base_options = dict(base_options or {})
    cb, cs, bo, co = base.to_c(), spec.to_c(), default_options(**base_options), default_options(**{**base_options, **options})
    if lib.cfz_problem_check(C.byref(cb), C.byref(bo), C.byref(cs), C.byref(co)) != 0:
        raise ValueError("cfz_problem_check: " + lib.cfz_last_error().decode())


def pack_problems(problems, options=None):
    """The arrays `cfz_loop_set_problems` takes: problems is a sequence of ProblemSpec or (ProblemSpec, {option overrides}), the overrides
    applied to `options` (a dict of overrides of the default options: what the engine was created with) -> (P, cfz_spec[P], cfz_options[P]);
    None -> (0, None, None), which switches the pool off."""
    if problems is None:
        return 0, None, None
    problems = list(problems)
    if not problems:
        raise ValueError("a problem pool needs at least one problem (None switches it off)")
    specs, opts = (_CSpec * len(problems))(), (_COptions * len(problems))()
    for p, item in enumerate(problems):
        spec, over = item if isinstance(item, tuple) else (item, {})
        if not isinstance(spec, ProblemSpec) or not isinstance(over, dict):
            raise TypeError(f"problems[{p}] must be a ProblemSpec or (ProblemSpec, dict of option overrides)")
        specs[p] = spec.to_c()
        opts[p] = default_options(**{**(options or {}), **over})
    return len(problems), specs, opts


def pack_maps(spec, maps):
    """The arrays `cfz_loop_set_maps` takes: maps is a sequence whose entries are each a list of obstacle objects (`.A` [4,2], `.b` [4], as
    `ProblemSpec.from_objects` takes them), a pair of arrays (A [n_obs,4,2], b [n_obs,4]) or a ProblemSpec (its A_obs, b_obs) ->
    (A [M,n_obs,4,2], b [M,n_obs,4]), n_obs that of `spec`.  An entry with another obstacle count is refused by name."""
    no = spec.n_obs
    A, b = np.zeros((len(maps), no, 4, 2)), np.zeros((len(maps), no, 4))
    for m, item in enumerate(maps):
        if isinstance(item, ProblemSpec):
            Am, bm = item.A_obs, item.b_obs
        elif isinstance(item, (tuple, list)) and len(item) == 2 and not hasattr(item[0], "A"):
            Am, bm = item
        elif isinstance(item, (tuple, list)) and all(hasattr(o, "A") and hasattr(o, "b") for o in item):
            Am, bm = [o.A for o in item], [o.b for o in item]
        else:
            raise TypeError(f"maps[{m}] must be a list of obstacles (.A, .b), a pair of arrays (A, b) or a ProblemSpec")
        Am = np.asarray(Am, dtype=np.float64).reshape(-1, 4, 2) if np.size(Am) else np.zeros((0, 4, 2))
        bm = np.asarray(bm, dtype=np.float64) if np.size(bm) else np.zeros((0, 4))
        if len(Am) != no or bm.shape != (len(Am), 4):
            raise ValueError(f"maps[{m}] has {len(Am)} obstacles (b of shape {bm.shape}), the engine's spec has {no}")
        A[m], b[m] = Am, bm
    return A, b


def map_check(spec, A, b):
    """`cfz_map_check`: may the obstacles A [n_obs,4,2], b [n_obs,4] stand in a map pool (`Engine.loop_set_maps`) of an engine created
    with `spec`?  Host arithmetic, needs no GPU.  Raises ValueError with the library's text, which names the obstacle that has an entry
    that is not finite or is no bounded quadrilateral."""
    lib = load_library()
    A, b = _f64(A, (spec.n_obs, 4, 2)), _f64(b, (spec.n_obs, 4))
    cs = spec.to_c()
    if lib.cfz_map_check(C.byref(cs), _ptr(A), _ptr(b)) != 0:
        raise ValueError("cfz_map_check: " + lib.cfz_last_error().decode())


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _seed64(seed):
    """The 64-bit key of a counter-based stream, as the C ABI takes it."""
    return C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)


def _stream_ids(stream, S):
    """Per-scenario stream ids [S] as uint32 (None: the library's default, scenario s draws from stream s)."""
    if stream is None:
        return None
    st = np.asarray(stream)
    if st.dtype.kind not in "iu" or st.shape != (S,) or (st < 0).any() or (st > 0xFFFFFFFF).any():
        raise ValueError(f"stream must hold {S} integers in [0, 2^32)")
    return np.ascontiguousarray(st, dtype=np.uint32)


def _f64(a, shape):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.shape != tuple(shape):
        raise ValueError(f"expected array of shape {tuple(shape)}, got {a.shape}")
    return a


def _ck(rc, name):
    if rc != 0:
        raise RuntimeError(f"{name}: " + load_library().cfz_last_error().decode())


def _pack_tubes(tubes):
    """Per vehicle a list over strategy steps 1.. of ((A_back, b_back), (A_front, b_front)) -> the 24 doubles per step the library reads."""
    return np.ascontiguousarray(np.concatenate([np.concatenate([np.asarray(A, float).ravel(), np.asarray(b, float).ravel()])
                                                for t in tubes for cellpair in t for (A, b) in cellpair]))


def _headings(final_headings, n):
    """Terminal headings [n], NaN where a vehicle has none (None, or no list at all)."""
    return np.array([np.nan if (final_headings is None or final_headings[b] is None) else float(final_headings[b]) for b in range(n)])


def _pairs(pairs):
    """Vehicle pairs as int32 [n, 2]; None (every pair) stays None."""
    return None if pairs is None else np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))


def trim_default_workspaces():
    """`cfz_plan_ws_trim(NULL)`: release the device memory of the calling thread's own workspaces behind `state_ws`, `colloc`,
    `joint_colloc` called without `ws=` (a 256-plan joint launch leaves 25 GB there)."""
    _ck(load_library().cfz_plan_ws_trim(None), "cfz_plan_ws_trim")


class PlanWorkspace:
    """`cfz_plan_ws`: a stream and the device buffers of the planning calls, kept between calls.  Pass as `ws=` to
    `state_ws`, `colloc`, `joint_colloc_batch`; without it those use a per-thread workspace inside the library."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        self._w = C.c_void_p()
        _ck(self.lib.cfz_plan_ws_create(int(device), C.byref(self._w)), "cfz_plan_ws_create")

    def trim(self):
        """`cfz_plan_ws_trim`: give the device memory held between calls back now (the next call allocates again)."""
        _ck(self.lib.cfz_plan_ws_trim(self._w), "cfz_plan_ws_trim")

    def close(self):
        if getattr(self, "_w", None):
            self.lib.cfz_plan_ws_destroy(self._w)
            self._w = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def state_ws_default_guess(init_pose, tube, final_heading=None, N=30):
    """`cfz_state_ws_default_guess`: the path through the tube's cells that `cfz_state_ws` starts from when it is given no guess
    (host arithmetic, no GPU).  tube as for `state_ws` (one vehicle); returns [N (n_sets - 1) + 1, 3]."""
    lib = load_library()
    n_sets = len(tube) + 1
    t = _pack_tubes([tube])
    g = np.zeros((N * (n_sets - 1) + 1, 3))
    p0 = _f64(np.asarray(init_pose, float)[:3], (3,))
    _ck(lib.cfz_state_ws_default_guess(n_sets, N, _ptr(p0), float("nan") if final_heading is None else float(final_heading), _ptr(t), _ptr(g)),
        "cfz_state_ws_default_guess")
    return g


def state_ws(init_poses, tubes, guesses=None, final_headings=None, device=0, ws=None, **options):
    """`cfz_state_ws`: the warm-start plans of several vehicles in one launch.
    init_poses [B][3]; tubes: per vehicle a list over strategy steps 1.. of ((A_back, b_back), (A_front, b_front));
    guesses: per vehicle an array [T+1, 3] of x, y, psi, or None (that vehicle then starts from `state_ws_default_guess`);
    final_headings: per vehicle a float or None.
    options: fields of `cfz_plan_options` (N, dt, wb, shrink_tube, bounded_input, max_iter, tol, ...).
    Returns a list of dict(traj [T+1,7], status, iters, cost)."""
    lib = load_library()
    po = _options(_CPlanOptions, "cfz_default_plan_options", "plan", options)
    B = len(tubes)
    n_sets = np.array([len(t) + 1 for t in tubes], dtype=np.int32)
    T = po.N * (n_sets - 1)
    tube = _pack_tubes(tubes)
    init = _f64(np.asarray(init_poses, float), (B, 3))
    fh = _headings(final_headings, B)
    guess = None
    if guesses is not None and any(g is not None for g in guesses):
        # a mixed batch (the reference's own `spline_ws_config`: vehicle_0 without a spline guess, the others with one): the vehicles
        # without a guess get the one the library would build for them, the others keep theirs (they used to lose it)
        gs = [np.asarray(g, float)[: T[b] + 1, :3] if g is not None else
              state_ws_default_guess(init[b], tubes[b], None if np.isnan(fh[b]) else float(fh[b]), N=po.N) for b, g in enumerate(guesses)]
        guess = np.ascontiguousarray(np.concatenate(gs))
        assert guess.shape[0] == int((T + 1).sum())
    traj = np.zeros((int((T + 1).sum()), 7))
    status, iters, cost = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B)
    args = (B, C.byref(po), _ptr(n_sets), _ptr(init), _ptr(fh), _ptr(tube), _ptr(guess), _ptr(traj), _ptr(status), _ptr(iters), _ptr(cost))
    _ck(lib.cfz_state_ws(int(device), *args) if ws is None else lib.cfz_state_ws_w(ws._w, *args), "cfz_state_ws")
    out, o = [], 0
    for b in range(B):
        out.append(dict(traj=traj[o : o + T[b] + 1].copy(), status=int(status[b]), iters=int(iters[b]), cost=float(cost[b])))
        o += T[b] + 1
    return out


def colloc(spec, init_poses, tubes, guesses, dt0s, final_headings=None, device=0, ws=None, **options):
    """`cfz_colloc`: the collocation plans (vehicle.py:360-661) of several vehicles in one launch.
    spec: ProblemSpec (wb, dmin, body, bounds, static obstacles); init_poses [B][3]; tubes as in `state_ws`;
    guesses: per vehicle an array [6 N, 7] of x, y, psi, v, delta, a, w at the collocation points; dt0s [B];
    options: fields of `cfz_colloc_options` (N_per_set, max_iter, shrink_tube, tol, constr_viol_tol, ...).
    Returns a list of dict(traj [N, 6, 7], dt, status, iters, cost)."""
    lib = load_library()
    co = _options(_CCollocOptions, "cfz_default_colloc_options", "collocation", options)
    B = len(tubes)
    n_sets = np.array([len(t) + 1 for t in tubes], dtype=np.int32)
    Np = co.N_per_set * (n_sets - 1) * 6
    tube = _pack_tubes(tubes)
    init = _f64(np.asarray(init_poses, float), (B, 3))
    fh = _headings(final_headings, B)
    guess = np.ascontiguousarray(np.concatenate([_f64(np.asarray(g, float), (int(Np[b]), 7)) for b, g in enumerate(guesses)]))
    dt0 = _f64(np.asarray(dt0s, float), (B,))
    traj, dt = np.zeros((int(Np.sum()), 7)), np.zeros(B)
    status, iters, cost = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B)
    cs = spec.to_c()
    args = (B, C.byref(cs), C.byref(co), _ptr(n_sets), _ptr(init), _ptr(fh), _ptr(tube), _ptr(guess), _ptr(dt0),
            _ptr(traj), _ptr(dt), _ptr(status), _ptr(iters), _ptr(cost))
    _ck(lib.cfz_colloc(int(device), *args) if ws is None else lib.cfz_colloc_w(ws._w, *args), "cfz_colloc")
    out, o = [], 0
    for b in range(B):
        out.append(dict(traj=traj[o : o + Np[b]].reshape(-1, 6, 7).copy(), dt=float(dt[b]), status=int(status[b]), iters=int(iters[b]), cost=float(cost[b])))
        o += Np[b]
    return out


def source_hash():
    """`cfz_source_hash`: which kernel sources the loaded library was built from (16 hex digits, or "unknown")."""
    lib = load_library()
    return lib.cfz_source_hash().decode()


def colloc_band_info(n_sets, N_per_set=5, n_obs=6, pairs=None, has_final=None):
    """`cfz_colloc_band_info`: (unknowns nk, half-bandwidth kb, bytes of the band) of the banded system of one (joint) collocation
    plan of len(n_sets) vehicles with n_sets[a] strategy steps each (host arithmetic, needs no GPU)."""
    lib = load_library()
    ns = np.ascontiguousarray(np.asarray(n_sets, np.int32))
    hf = None if has_final is None else np.ascontiguousarray(np.asarray(has_final, np.int32))
    pr = _pairs(pairs)
    nk, kb, bb = C.c_int32(), C.c_int32(), C.c_int64()
    _ck(lib.cfz_colloc_band_info(len(ns), _ptr(ns), _ptr(hf), int(N_per_set), int(n_obs), 0 if pr is None else len(pr), _ptr(pr),
                                 C.addressof(nk), C.addressof(kb), C.addressof(bb)), "cfz_colloc_band_info")
    return int(nk.value), int(kb.value), int(bb.value)


def colloc_elimination_info(n_sets, N_per_set=5, n_obs=6, pairs=None, has_final=None, structured=1):
    """`cfz_colloc_elimination_info`: dict(nk, kb, band_bytes, alg_bytes, workspace_bytes) of the elimination one (joint) collocation plan
    goes through (host arithmetic, needs no GPU); alg_bytes: bytes per Newton system, bench.py's roofline of the planning kernels."""
    lib = load_library()
    ns = np.ascontiguousarray(np.asarray(n_sets, np.int32))
    hf = None if has_final is None else np.ascontiguousarray(np.asarray(has_final, np.int32))
    pr = _pairs(pairs)
    nk, kb, bb, ab, wb = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64()
    _ck(lib.cfz_colloc_elimination_info(len(ns), _ptr(ns), _ptr(hf), int(N_per_set), int(n_obs), 0 if pr is None else len(pr), _ptr(pr), int(structured),
                                        C.addressof(nk), C.addressof(kb), C.addressof(bb), C.addressof(ab), C.addressof(wb)), "cfz_colloc_elimination_info")
    return dict(nk=int(nk.value), kb=int(kb.value), band_bytes=int(bb.value), alg_bytes=int(ab.value), workspace_bytes=int(wb.value))


def joint_colloc_batch(spec, scenarios, pairs=None, device=0, ws=None, **options):
    """`cfz_joint_colloc`: B joint collocation plans (one workgroup each) of V vehicles with one shared dt per plan and pairwise
    separation rows (multi_vehicle_planner.py:343-480).  scenarios: list of dict(init_poses [V][3], tubes, guesses, dt0,
    final_headings) with per-vehicle entries as in `colloc`, the same V in every scenario; pairs: list of (a, b) vehicle
    index pairs, default all.  Returns a list of dict(traj: per vehicle [N_a, 6, 7], dt, status, iters, cost)."""
    lib = load_library()
    co = _options(_CCollocOptions, "cfz_default_colloc_options", "collocation", options)
    B, V = len(scenarios), len(scenarios[0]["tubes"])
    assert all(len(sc["tubes"]) == V for sc in scenarios)
    tubes = [t for sc in scenarios for t in sc["tubes"]]
    n_sets = np.array([len(t) + 1 for t in tubes], dtype=np.int32)
    Np = co.N_per_set * (n_sets - 1) * 6
    tube = _pack_tubes(tubes)
    init = _f64(np.concatenate([np.asarray(sc["init_poses"], float).reshape(V, 3) for sc in scenarios]), (B * V, 3))
    fh = _headings([f for sc in scenarios for f in (sc.get("final_headings") or [None] * V)], B * V)
    guesses = [g for sc in scenarios for g in sc["guesses"]]
    guess = np.ascontiguousarray(np.concatenate([_f64(np.asarray(g, float), (int(Np[b]), 7)) for b, g in enumerate(guesses)]))
    dt0 = _f64(np.array([float(sc["dt0"]) for sc in scenarios]), (B,))
    pr = _pairs(pairs)
    traj, dt = np.zeros((int(Np.sum()), 7)), np.zeros(B)
    status, iters, cost = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B)
    cs = spec.to_c()
    args = (B, V, C.byref(cs), C.byref(co), _ptr(n_sets), _ptr(init), _ptr(fh), _ptr(tube), _ptr(guess), _ptr(dt0),
            0 if pr is None else len(pr), _ptr(pr), _ptr(traj), _ptr(dt), _ptr(status), _ptr(iters), _ptr(cost))
    _ck(lib.cfz_joint_colloc(int(device), *args) if ws is None else lib.cfz_joint_colloc_w(ws._w, *args), "cfz_joint_colloc")
    out, o = [], 0
    for b in range(B):
        tr = []
        for a in range(V):
            n = int(Np[b * V + a])
            tr.append(traj[o : o + n].reshape(-1, 6, 7).copy())
            o += n
        out.append(dict(traj=tr, dt=float(dt[b]), status=int(status[b]), iters=int(iters[b]), cost=float(cost[b])))
    return out


def joint_colloc(spec, init_poses, tubes, guesses, dt0, final_headings=None, pairs=None, device=0, **options):
    """One joint plan: `joint_colloc_batch` with a single scenario.  Returns dict(traj: per vehicle [N_a, 6, 7], dt, status, iters, cost)."""
    return joint_colloc_batch(spec, [dict(init_poses=init_poses, tubes=tubes, guesses=guesses, dt0=dt0, final_headings=final_headings)],
                              pairs=pairs, device=device, **options)[0]


class Engine:
    """One batched solver instance on one GPU (a `cfz_handle`)."""

    def __init__(self, spec: ProblemSpec, max_batch: int, device: int = 0, **options):
        self.lib = load_library()
        self.spec = spec
        self.max_batch = int(max_batch)
        self.options = dict(options)  # (the base of the overrides of loop_set_problems)
        self._h = C.c_void_p()
        self._S = self._V = 0  # scenarios and vehicles of the closed loop; 0 until loop_init (the library refuses loop calls before it)
        self._P = self._T = 0  # plan sets of the closed loop's pool and their samples
        self._rec_cap = self._rec_used = 0
        cs, co = spec.to_c(), default_options(**options)
        _ck(self.lib.cfz_create(C.byref(cs), C.byref(co), int(device), self.max_batch, C.byref(self._h)), "cfz_create")

    def close(self):
        if getattr(self, "_h", None):
            self.lib.cfz_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    _ck = staticmethod(_ck)

    # ---- host-buffer path ------------------------------------------------------------------
    def solve(self, x0, ref, nbr, zu, want_duals=True, carry=None, slots=None):
        """x0 [B,5], ref [B,3,N], nbr [B,n_nbr,3,N], zu [B,7,N] (warm start) ->
        dict(zu, status, iters, cost, kkt_err, min_sep[, l, m, lam_ij, lam_ji, s], solve_ms).
        carry: int/bool [B]; carry[b] says that this solve of slot b is the MPC iteration following the one last
        solved in slot b, so the interior point starts from its multipliers (`cfz_mpc_set_carry`).
        slots: int [B]; the carry record instance b reads and refreshes (`cfz_mpc_set_slots`; default b)."""
        sp = self.spec
        N, no, nn = sp.N, sp.n_obs, sp.n_nbr
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        B = x0.shape[0]
        x0 = _f64(x0, (B, 5)); ref = _f64(ref, (B, 3, N)); zu = _f64(zu, (B, 7, N))
        nbr = _f64(nbr, (B, nn, 3, N)) if nn else None
        self._ck(self.lib.cfz_mpc_set_params(self._h, B, _ptr(x0), _ptr(ref), _ptr(nbr)), "cfz_mpc_set_params")
        self._ck(self.lib.cfz_mpc_set_warm(self._h, B, _ptr(zu)), "cfz_mpc_set_warm")
        if carry is not None:
            cflags = np.ascontiguousarray(np.broadcast_to(np.asarray(carry), (B,)), dtype=np.int32)
            self._ck(self.lib.cfz_mpc_set_carry(self._h, B, _ptr(cflags)), "cfz_mpc_set_carry")
        if slots is not None:
            sl = np.ascontiguousarray(np.broadcast_to(np.asarray(slots), (B,)), dtype=np.int32)
            self._ck(self.lib.cfz_mpc_set_slots(self._h, B, _ptr(sl)), "cfz_mpc_set_slots")
        self._ck(self.lib.cfz_mpc_solve(self._h, B), "cfz_mpc_solve")
        out = dict(zu=np.empty((B, 7, N)), status=np.empty(B, np.int32), iters=np.empty(B, np.int32),
                   cost=np.empty(B), kkt_err=np.empty(B), min_sep=np.empty(B))
        if want_duals:
            out.update(l=np.zeros((B, N, 4 * no)), m=np.zeros((B, N, 4 * no)), lam_ij=np.zeros((B, nn, N, 4)),
                       lam_ji=np.zeros((B, nn, N, 4)), s=np.zeros((B, nn, N, 2)))
        self._ck(self.lib.cfz_mpc_get(self._h, B, _ptr(out["zu"]), _ptr(out.get("l")), _ptr(out.get("m")),
                                      _ptr(out.get("lam_ij")), _ptr(out.get("lam_ji")), _ptr(out.get("s"))), "cfz_mpc_get")
        self._ck(self.lib.cfz_mpc_stats(self._h, B, _ptr(out["status"]), _ptr(out["iters"]), _ptr(out["cost"]),
                                        _ptr(out["kkt_err"]), _ptr(out["min_sep"])), "cfz_mpc_stats")
        out["solve_ms"] = self.last_solve_ms()
        return out

    def kernel_info(self):
        """(LDS bytes per instance, resident instances per CU)."""
        a, b = C.c_int32(), C.c_int32()
        self._ck(self.lib.cfz_kernel_info(self._h, C.byref(a), C.byref(b)), "cfz_kernel_info")
        return a.value, b.value

    def last_solve_ms(self):
        return float(self.lib.cfz_last_solve_ms(self._h))

    def set_carry(self, flags):
        """`cfz_mpc_set_carry` for the next solve (host or device path): flags [B] int."""
        flags = np.ascontiguousarray(flags, dtype=np.int32)
        self._ck(self.lib.cfz_mpc_set_carry(self._h, len(flags), _ptr(flags)), "cfz_mpc_set_carry")

    def set_carry_device(self, B, d_flags):
        """`cfz_mpc_set_carry_device`: flags as a device int32 array (torch tensor or pointer), no copy, no sync."""
        p = C.c_void_p(d_flags.data_ptr() if hasattr(d_flags, "data_ptr") else int(d_flags))
        self._ck(self.lib.cfz_mpc_set_carry_device(self._h, int(B), p), "cfz_mpc_set_carry_device")

    # ---- device-pointer path (torch tensors or any object with data_ptr()) --------------------
    def solve_device(self, B, d_x0, d_ref, d_nbr, d_zu, d_status, d_iters, d_stats, stream=None):
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else int(t))
        self._ck(self.lib.cfz_mpc_solve_device(self._h, int(B), ptr(d_x0), ptr(d_ref), ptr(d_nbr), ptr(d_zu),
                                               ptr(d_status), ptr(d_iters), ptr(d_stats),
                                               None if stream is None else C.c_void_p(int(stream))), "cfz_mpc_solve_device")

    def vsl_step(self, S, V, d_own, T, d_table, d_k0, t, d_allpred, d_pred, d_state, d_status, d_iters, d_stats, d_carry, stream=None):
        """`cfz_vsl_step`: one iteration of the vehicle-sharded closed loop on device tensors, no host synchronisation."""
        ptr = lambda x: C.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))
        self._ck(self.lib.cfz_vsl_step(self._h, int(S), int(V), int(d_own.numel()), ptr(d_own), int(T), ptr(d_table), ptr(d_k0), int(t),
                                       ptr(d_allpred), ptr(d_pred), ptr(d_state), ptr(d_status), ptr(d_iters), ptr(d_stats), ptr(d_carry),
                                       None if stream is None else C.c_void_p(int(stream))), "cfz_vsl_step")

    # ---- dual warm start (Vehicle.dual_ws) ------------------------------------------------------------
    def dual_ws(self, poses):
        """poses [n,3] (x,y,psi) -> (l [n,4 n_obs], m [n,4 n_obs], d [n,n_obs])."""
        poses = np.ascontiguousarray(poses, dtype=np.float64)
        n, no = poses.shape[0], self.spec.n_obs
        poses = _f64(poses, (n, 3))
        l, m, d = np.zeros((n, 4 * no)), np.zeros((n, 4 * no)), np.zeros((n, no))
        self._ck(self.lib.cfz_dual_ws(self._h, n, _ptr(poses), _ptr(l), _ptr(m), _ptr(d)), "cfz_dual_ws")
        return l, m, d

    def joint_dual_ws(self, poses_this, poses_other):
        """`cfz_joint_dual_ws`: poses [n,3] of two vehicles -> (lam [n,4], mu [n,4], s [n,2], d [n])."""
        pa = _f64(np.asarray(poses_this, float), (len(poses_this), 3))
        pb = _f64(np.asarray(poses_other, float), (len(pa), 3))
        n = len(pa)
        lam, mu, s, d = np.zeros((n, 4)), np.zeros((n, 4)), np.zeros((n, 2)), np.zeros(n)
        self._ck(self.lib.cfz_joint_dual_ws(self._h, n, _ptr(pa), _ptr(pb), _ptr(lam), _ptr(mu), _ptr(s), _ptr(d)), "cfz_joint_dual_ws")
        return lam, mu, s, d

    # ---- batched closed loop ------------------------------------------------------------------------
    def loop_init(self, ref_table, k0, noise=None, table_of=None):
        """ref_table [V,T,7] (x,y,psi,v,delta,a,w) followed by every scenario (`cfz_loop_init`), or a pool of plan sets [P,V,T,7]
        of which scenario s follows set table_of[s] (`cfz_loop_init_tables`; table_of None: set s, P == S); k0 int32 [S],
        noise [S,V,5] or None."""
        V = self.spec.n_nbr + 1
        ref_table = np.ascontiguousarray(ref_table, dtype=np.float64)
        k0 = np.ascontiguousarray(k0, dtype=np.int32)
        S = k0.shape[0]
        if noise is not None:
            noise = _f64(noise, (S, V, 5))
        if ref_table.ndim == 3:
            if table_of is not None:
                raise ValueError("table_of needs a pool of plan sets [P, V, T, 7]")
            T = ref_table.shape[1]
            ref_table = _f64(ref_table, (V, T, 7))
            self._ck(self.lib.cfz_loop_init(self._h, S, T, _ptr(ref_table), _ptr(k0), _ptr(noise)), "cfz_loop_init")
        else:
            P, T = ref_table.shape[0], ref_table.shape[2]
            ref_table = _f64(ref_table, (P, V, T, 7))
            tof = None if table_of is None else np.ascontiguousarray(table_of, dtype=np.int32)
            if tof is not None and tof.shape != (S,):
                raise ValueError(f"table_of must have shape ({S},), got {tof.shape}")
            self._ck(self.lib.cfz_loop_init_tables(self._h, S, P, T, _ptr(ref_table), _ptr(tof), _ptr(k0), _ptr(noise)),
                     "cfz_loop_init_tables")
        self._S, self._V = S, V
        self._P, self._T = (1 if ref_table.ndim == 3 else ref_table.shape[0]), T
        self._rec_cap, self._rec_used = 0, 0

    def loop_set_order(self, order):
        """`cfz_loop_set_order`: the exchange rule of the closed loop's later steps and runs.  None: Jacobi (every vehicle plans
        against the others' predictions of the previous iteration, advanced; the default, and what `loop_init` restores).  [V]
        (one order for every scenario) or [S, V] integers (one per scenario): the vehicles of a scenario solve one after another
        in that order, each against the predictions of those before it from the same iteration (not advanced) and the previous
        iteration's predictions of the others, advanced."""
        if order is None or not self._S:  # (before loop_init the library refuses the call)
            self._ck(self.lib.cfz_loop_set_order(self._h, None), "cfz_loop_set_order")
            return
        S, V = self._S, self._V
        o = np.asarray(order)
        if o.dtype.kind not in "iu":
            raise ValueError(f"order must hold integers, got dtype {o.dtype}")
        if o.shape == (V,):
            o = np.broadcast_to(o, (S, V))
        if o.shape != (S, V):
            raise ValueError(f"order must have shape ({V},) or ({S}, {V}), got {np.shape(order)}")
        bad = np.flatnonzero((np.sort(o, axis=1) != np.arange(V)).any(axis=1))
        if bad.size:
            raise ValueError(f"order[{bad[0]}] = {o[bad[0]].tolist()} is not a permutation of 0..{V - 1}")
        o = np.ascontiguousarray(o, dtype=np.int32)
        self._ck(self.lib.cfz_loop_set_order(self._h, _ptr(o)), "cfz_loop_set_order")

    def loop_set_disturbance(self, seed, meas=None, act=None, proc=None, level=None, stream=None):
        """`cfz_loop_set_disturbance`: noise on the later steps and runs of the closed loop, drawn on the device from counter-based
        streams (Philox4x32-10 keyed by `seed`; include/confrez_hip.h).  Standard deviations meas [5] of the measurement (x, y, psi, v,
        delta) the solver is pinned to, act [2] of the applied input (a, w; clipped to the input box afterwards), proc [5] of the state
        after the plant; None: zeros, all three None: off (what `loop_init` restores).  level [S] scales the three groups per scenario
        (None: 1), stream [S] is each scenario's stream id (None: s): scenarios with equal ids draw the same noise."""
        S = self._S

        def group(a, n, name):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.shape != (n,):
                raise ValueError(f"{name} must have shape ({n},), got {a.shape}")
            return a

        meas, act, proc = group(meas, 5, "meas"), group(act, 2, "act"), group(proc, 5, "proc")
        if not S:  # (before loop_init the library refuses the call)
            level = stream = None
        level, stream = group(level, S, "level"), _stream_ids(stream, S)
        self._ck(self.lib.cfz_loop_set_disturbance(self._h, _seed64(seed), _ptr(meas), _ptr(act), _ptr(proc), _ptr(level), _ptr(stream)),
                 "cfz_loop_set_disturbance")

    def loop_disturbance(self, t0=0, K=1):
        """`cfz_loop_disturbance`: d [K,S,V,12] that the loop adds at steps [t0, t0 + K) under the setting in force (0:5 measurement,
        5:7 input, 7:12 process); steps count from `loop_init`."""
        S, V = self._S, self._V
        d = np.empty((max(int(K), 0), S, V, 12))
        self._ck(self.lib.cfz_loop_disturbance(self._h, int(t0), int(K), _ptr(d)), "cfz_loop_disturbance")
        return d

    def loop_set_comm(self, seed, p_drop=None, max_age=3, compensate=True, stream=None):
        """`cfz_loop_set_comm`: a lossy prediction exchange on the later steps and runs of the closed loop (include/confrez_hip.h).  A
        neighbour's message of an iteration is lost with probability p_drop (a scalar, or [S] per scenario; None: lossless again, what
        `loop_init` restores), drawn on the device from counter-based streams keyed by `seed`; a vehicle then plans against the newest
        message that arrived, at most max_age (1..6) iterations old, advanced by its age (compensate) or as if it were new (the
        reference's node).  stream [S] is each scenario's stream id (None: s).  Every call that switches it on restarts the message
        history at the current predictions."""
        S = self._S
        if p_drop is None or not S:  # (before loop_init the library refuses the call)
            p = None if p_drop is None else np.zeros(1)
            self._ck(self.lib.cfz_loop_set_comm(self._h, _seed64(seed), _ptr(p), 1, 0, None), "cfz_loop_set_comm")
            return
        p = np.asarray(p_drop)
        if p.dtype.kind not in "fiu":
            raise ValueError(f"p_drop must hold real numbers, got dtype {p.dtype}")
        if p.shape == ():
            p = np.broadcast_to(p, (S,))
        if p.shape != (S,):
            raise ValueError(f"p_drop must be a scalar or have shape ({S},), got {np.shape(p_drop)}")
        p = np.ascontiguousarray(p, dtype=np.float64)
        for name, val in (("max_age", max_age), ("compensate", compensate)):
            if not isinstance(val, (bool, int, np.integer, np.bool_)):
                raise ValueError(f"{name} must be an integer, got {type(val).__name__}")
        stream = _stream_ids(stream, S)
        self._ck(self.lib.cfz_loop_set_comm(self._h, _seed64(seed), _ptr(p), int(max_age), int(compensate), _ptr(stream)), "cfz_loop_set_comm")

    def loop_comm(self, tau0=0, K=1):
        """`cfz_loop_comm`: bool [K,S,V,V], the delivery bits of the messages of iterations [tau0, tau0 + K) under the setting in force;
        [k, s, v, u] is the message from vehicle u to vehicle v, the diagonal True; iterations count from `loop_init`."""
        S, V = self._S, self._V
        b = np.empty((max(int(K), 0), S, V, V), np.int32)
        self._ck(self.lib.cfz_loop_comm(self._h, int(tau0), int(K), _ptr(b)), "cfz_loop_comm")
        return b.astype(bool)

    def problem_check(self, spec, **options):
        """`problem_check` against this engine's spec and the options it was created with: what `loop_set_problems` will decide."""
        problem_check(self.spec, spec, self.options, **options)

    def loop_set_problems(self, problems, problem_of=None):
        """`cfz_loop_set_problems`: per-scenario problem constants on the later steps and runs of the closed loop (include/confrez_hip.h).
        problems: a sequence of ProblemSpec or (ProblemSpec, {option overrides}), the overrides applied to the options this engine was
        created with; problem_of [S]: the problem of each scenario.  Every solve of scenario s then uses that problem's dmin, bounds,
        weights and options; geometry, time base and carry_duals must be the engine's (`problem_check`).  None: off again, what
        `loop_init` restores."""
        P, specs, opts = pack_problems(problems, self.options)
        if P == 0 or not self._S:  # (before loop_init the library refuses the call)
            self._ck(self.lib.cfz_loop_set_problems(self._h, P, specs, opts, None), "cfz_loop_set_problems")
            return
        po = np.asarray(problem_of)
        if po.dtype.kind not in "iu" or po.shape != (self._S,):
            raise ValueError(f"problem_of must hold {self._S} integers, got shape {po.shape}, dtype {po.dtype}")
        po = np.ascontiguousarray(po, dtype=np.int32)
        self._ck(self.lib.cfz_loop_set_problems(self._h, P, specs, opts, _ptr(po)), "cfz_loop_set_problems")

    def _maps(self, maps, map_of, S):
        """(M, A, b, map_of) as the library takes them; maps None or []: (0, None, None, None)."""
        if maps is None or len(maps) == 0:
            return 0, None, None, None
        A, b = pack_maps(self.spec, maps)
        if map_of is None:
            raise ValueError("map_of is required with a pool of maps")
        mo = np.asarray(map_of)
        if mo.dtype.kind not in "iu" or mo.shape != (S,):
            raise ValueError(f"map_of must hold {S} integers, got shape {mo.shape}, dtype {mo.dtype}")
        return len(A), A, b, np.ascontiguousarray(mo, dtype=np.int32)

    def loop_set_maps(self, maps, map_of=None):
        """`cfz_loop_set_maps`: per-scenario obstacle maps on the later steps and runs of the closed loop (include/confrez_hip.h).  maps: a
        sequence of maps as `pack_maps` takes them (lists of obstacles, (A, b) pairs or ProblemSpecs), each with this engine's obstacle
        count; map_of [S]: the map of each scenario.  Every solve of scenario s then stands on that map, and `loop_audit` measures the
        scenario against it.  Composes with `loop_set_problems` in either order.  None or []: off again, what `loop_init` restores."""
        if not self._S and maps is not None and len(maps):  # (before loop_init the library refuses the call)
            A, b = pack_maps(self.spec, maps)
            self._ck(self.lib.cfz_loop_set_maps(self._h, len(A), _ptr(A), _ptr(b), None), "cfz_loop_set_maps")
            return
        M, A, b, mo = self._maps(maps, map_of, self._S)
        self._ck(self.lib.cfz_loop_set_maps(self._h, M, _ptr(A), _ptr(b), _ptr(mo)), "cfz_loop_set_maps")

    def loop_step(self):
        self._ck(self.lib.cfz_loop_step(self._h), "cfz_loop_step")
        if self._rec_cap:
            self._rec_used += 1

    def loop_run(self, K):
        """K closed-loop iterations in one persistent launch (same results as K x loop_step, under either exchange rule)."""
        self._ck(self.lib.cfz_loop_run(self._h, int(K)), "cfz_loop_run")
        if self._rec_cap:
            self._rec_used += int(K)
        return int(self.lib.cfz_loop_last_iterations(self._h))

    def loop_record(self, K):
        """`cfz_loop_record`: record the next K steps (state after the plant, applied (a, w), status, iterations); 0 stops."""
        self._ck(self.lib.cfz_loop_record(self._h, int(K)), "cfz_loop_record")
        self._rec_cap, self._rec_used = int(K), 0

    def loop_history(self, t0=0, K=None):
        """`cfz_loop_history`: recorded steps [t0, t0 + K) (K None: all recorded so far) ->
        dict(traj [K,S,V,7] (x, y, psi, v, delta, a, w), status [K,S,V], iters [K,S,V])."""
        K = self._rec_used - int(t0) if K is None else int(K)
        S, V = self._S, self._V
        out = dict(traj=np.empty((K, S, V, 7)), status=np.empty((K, S, V), np.int32), iters=np.empty((K, S, V), np.int32))
        self._ck(self.lib.cfz_loop_history(self._h, int(t0), K, _ptr(out["traj"]), _ptr(out["status"]), _ptr(out["iters"])),
                 "cfz_loop_history")
        return out

    @staticmethod
    def _audit_out(S, V):
        return dict(clear=np.empty((S, 2)), where=np.empty((S, 6), np.int32), first_contact=np.empty(S, np.int32),
                    arrive=np.empty((S, V), np.int32))

    def loop_audit(self, t0=0, K=None, pos_tol=ARRIVE_TOL["pos_tol"], psi_tol=ARRIVE_TOL["psi_tol"], v_tol=ARRIVE_TOL["v_tol"]):
        """`cfz_loop_audit` over recorded steps [t0, t0 + K) (K None: all recorded so far) -> dict(clear [S,2] (smallest
        vehicle-vehicle, vehicle-obstacle signed distance), where [S,6] ((step, u, w), (step, v, j) of those), first_contact [S],
        arrive [S,V]); steps count from t0, -1 = never."""
        K = self._rec_used - int(t0) if K is None else int(K)
        o = self._audit_out(self._S, self._V)
        self._ck(self.lib.cfz_loop_audit(self._h, int(t0), K, float(pos_tol), float(psi_tol), float(v_tol), _ptr(o["clear"]),
                                         _ptr(o["where"]), _ptr(o["first_contact"]), _ptr(o["arrive"])), "cfz_loop_audit")
        return o

    def audit(self, traj, goal, maps=None, map_of=None, pos_tol=ARRIVE_TOL["pos_tol"], psi_tol=ARRIVE_TOL["psi_tol"], v_tol=ARRIVE_TOL["v_tol"]):
        """`cfz_audit_maps` of a host trajectory traj [K,S,V,7] (x, y, psi, v, ...) with goals [S,V,3], against this engine's body and
        obstacles, or, with maps (as `loop_set_maps` takes them) and map_of [S], scenario s against the obstacles of map map_of[s]
        -> the dict of `loop_audit`."""
        traj = np.ascontiguousarray(traj, dtype=np.float64)
        if traj.ndim != 4 or traj.shape[3] < 4:
            raise ValueError(f"expected traj of shape [K, S, V, 7], got {traj.shape}")
        K, S, V = traj.shape[:3]
        if traj.shape[3] != 7:
            t7 = np.zeros((K, S, V, 7)); t7[..., : traj.shape[3]] = traj; traj = t7
        goal = _f64(goal, (S, V, 3))
        o = self._audit_out(S, V)
        M, A, b, mo = self._maps(maps, map_of, S)
        self._ck(self.lib.cfz_audit_maps(self._h, K, S, V, _ptr(traj), _ptr(goal), M, _ptr(A), _ptr(b), _ptr(mo), float(pos_tol), float(psi_tol),
                                         float(v_tol), _ptr(o["clear"]), _ptr(o["where"]), _ptr(o["first_contact"]), _ptr(o["arrive"])), "cfz_audit_maps")
        return o

    def loop_score(self, t0=0, K=None, near=0.5, weights=None, **tol):
        """`cfz_loop_score` over recorded steps [t0, t0 + K) (K None: all recorded so far): what every vehicle's realised closed loop
        cost against the plan it follows -> the dict of `score_summary` (every raw column by name, cost, track_rms, track_max, time,
        distance, wait; each [S,V]).  near [m]: the distance to another body below which a step counts in `near_steps`; weights [6] or
        [S,6] (None: the engine's `spec.weights`); pos_tol, psi_tol, v_tol as `loop_audit`."""
        args = _score_args(near, tol)
        K = self._rec_used - int(t0) if K is None else int(K)
        S, V = self._S, self._V
        val, cnt = np.empty((S, V, len(SCORE_VAL))), np.empty((S, V, len(SCORE_CNT)), np.int32)
        self._ck(self.lib.cfz_loop_score(self._h, int(t0), K, *args, _ptr(val), _ptr(cnt)), "cfz_loop_score")
        return score_summary(val, cnt, self.spec.dt, self.spec.weights if weights is None else weights)

    def score(self, traj, tables, table_of, k0, status=None, iters=None, near=0.5, weights=None, **tol):
        """`cfz_score` of a host record traj [K,S,V,7] (with status, iters [K,S,V]; None: all 0: what `loop_history` returns) against
        the plan sets tables [P,V,T,7], scenario s following set table_of[s] from the clock index k0[s] of the state before the first
        row; this engine's body, any V up to 8 -> the dict of `loop_score`."""
        args = _score_args(near, tol)
        traj = np.ascontiguousarray(traj, dtype=np.float64)
        if traj.ndim != 4 or traj.shape[3] != 7:
            raise ValueError(f"expected traj of shape [K, S, V, 7], got {traj.shape}")
        K, S, V = traj.shape[:3]
        tables = np.ascontiguousarray(tables, dtype=np.float64)
        if tables.ndim != 4 or tables.shape[1] != V or tables.shape[3] != 7:
            raise ValueError(f"expected tables of shape [P, {V}, T, 7], got {tables.shape}")
        P, T = tables.shape[0], tables.shape[2]
        ints = []
        for name, a, shape in (("table_of", table_of, (S,)), ("k0", k0, (S,)), ("status", status, (K, S, V)), ("iters", iters, (K, S, V))):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.int32)
                if a.shape != shape:
                    raise ValueError(f"{name} must have shape {shape}, got {a.shape}")
            ints.append(a)
        tof, k0, status, iters = ints
        if tof is None or k0 is None:
            raise ValueError("table_of and k0 are required")
        val, cnt = np.empty((S, V, len(SCORE_VAL))), np.empty((S, V, len(SCORE_CNT)), np.int32)
        self._ck(self.lib.cfz_score(self._h, K, S, V, _ptr(traj), _ptr(status), _ptr(iters), P, T, _ptr(tables), _ptr(tof), _ptr(k0), *args,
                                    _ptr(val), _ptr(cnt)), "cfz_score")
        return score_summary(val, cnt, self.spec.dt, self.spec.weights if weights is None else weights)

    def plan_conflicts(self, tables, max_lag, margin=None):
        """`cfz_plan_conflicts`: the conflict map of the plan sets tables [P,V,T,7] (or one set [V,T,7]: P = 1; this engine's body, any
        V up to 8) over the lags -max_lag..max_lag [samples] -> dict(clear (smallest signed distance of the two bodies), when (the
        lowest step that attains it), first (the lowest step closer than margin, -1 none), count (the number of such steps), each
        [P, npair, 2 max_lag + 1]; pairs [npair, 2] (u < w); lags [2 max_lag + 1]).  At lag tau > 0 vehicle w of the pair runs tau
        samples late, at tau < 0 vehicle u runs |tau| late.  margin [m] None: the problem's `dmin`.  `conflict_summary` condenses it."""
        D, margin = _conflict_args(max_lag, margin, self.spec)
        tables = np.ascontiguousarray(tables, dtype=np.float64)
        if tables.ndim == 3:
            tables = tables[None]
        if tables.ndim != 4 or tables.shape[3] != 7 or 0 in tables.shape:
            raise ValueError(f"expected tables of shape [P, V, T, 7] or [V, T, 7], got {tables.shape}")
        P, V, T = tables.shape[:3]
        clear, info = _conflict_out(P, V, D)
        self._ck(self.lib.cfz_plan_conflicts(self._h, P, V, T, _ptr(tables), D, margin, _ptr(clear), _ptr(info)), "cfz_plan_conflicts")
        return _conflict_dict(clear, info, V, D)

    def loop_plan_conflicts(self, max_lag, margin=None):
        """`cfz_loop_plan_conflicts`: `plan_conflicts` of the pool that `loop_init` left on the device (nothing is uploaded, the loop is
        left as it is) -> the same dict, P the pool's."""
        D, margin = _conflict_args(max_lag, margin, self.spec)
        clear, info = _conflict_out(self._P, self._V, D)
        self._ck(self.lib.cfz_loop_plan_conflicts(self._h, D, margin, _ptr(clear), _ptr(info)), "cfz_loop_plan_conflicts")
        return _conflict_dict(clear, info, self._V, D)

    def delay_search(self, cmap, slack=0, cap=None):
        """`cfz_delay_search`: the start delays that make every plan set of the conflict map `cmap` (the dict `plan_conflicts` returns, or
        an edited one: count [P, npair, 2D+1] and, optionally, clear) conflict-free -> dict(delays [P, V] int32 (-1: nothing feasible),
        found [P] bool, span [P] (the largest delay), total [P] (their sum), clear [P] (the smallest clearance of the set under the
        delays; +inf for V = 1, -inf if not found, NaN without cmap["clear"])).  Vehicle v of set p starts delays[p, v] samples late, waiting
        at its first sample: `scenarios.delay_tables(tables, delays)`.  Pair (u, w) then runs at the map's lag delays[w] - delays[u]; every
        lag within `slack` samples of it must lie inside the map's window and be free (count 0, clear finite).  cap [V] or [P, V]: the
        most each vehicle may be delayed (None: D; 0: it leaves on time).  The answer is the smallest under (span, total, the delays as a
        tuple)."""
        count = np.ascontiguousarray(cmap["count"], dtype=np.int32)
        if count.ndim != 3 or count.shape[0] == 0 or count.shape[2] % 2 != 1:
            raise ValueError(f"expected count of shape [P, npair, 2D+1], got {count.shape}")
        P, npair, D = count.shape[0], count.shape[1], count.shape[2] // 2
        V = int(round((1 + np.sqrt(1 + 8 * npair)) / 2))
        if V * (V - 1) // 2 != npair:
            raise ValueError(f"{npair} pairs are not the pairs of a whole number of vehicles")
        clear = cmap.get("clear")
        if clear is not None:
            clear = np.ascontiguousarray(clear, dtype=np.float64)
            if clear.shape != count.shape:
                raise ValueError(f"expected clear of the shape of count {count.shape}, got {clear.shape}")
        slack, cap = _delay_args(slack, cap, P, V, D)
        delays, info, rclear = _delay_out(P, V)
        self._ck(self.lib.cfz_delay_search(self._h, P, V, D, _ptr(count), _ptr(clear), slack, _ptr(cap), _ptr(delays), _ptr(info), _ptr(rclear)),
                 "cfz_delay_search")
        return _delay_dict(delays, info, rclear)

    def plan_delays(self, tables, max_lag, margin=None, slack=0, cap=None):
        """`cfz_plan_delays`: `delay_search(plan_conflicts(tables, max_lag, margin), slack, cap)` with the map computed and searched on
        the device: it never comes back to the host -> the same dict."""
        D, margin = _conflict_args(max_lag, margin, self.spec)
        tables = np.ascontiguousarray(tables, dtype=np.float64)
        if tables.ndim == 3:
            tables = tables[None]
        if tables.ndim != 4 or tables.shape[3] != 7 or 0 in tables.shape:
            raise ValueError(f"expected tables of shape [P, V, T, 7] or [V, T, 7], got {tables.shape}")
        P, V, T = tables.shape[:3]
        slack, cap = _delay_args(slack, cap, P, V, D)
        delays, info, rclear = _delay_out(P, V)
        self._ck(self.lib.cfz_plan_delays(self._h, P, V, T, _ptr(tables), D, margin, slack, _ptr(cap), _ptr(delays), _ptr(info), _ptr(rclear)),
                 "cfz_plan_delays")
        return _delay_dict(delays, info, rclear)

    def loop_plan_delays(self, max_lag, margin=None, slack=0, cap=None):
        """`cfz_loop_plan_delays`: `plan_delays` of the pool that `loop_init` left on the device (nothing is uploaded but the caps, the
        loop is left as it is) -> the same dict, P the pool's."""
        D, margin = _conflict_args(max_lag, margin, self.spec)
        slack, cap = _delay_args(slack, cap, self._P, self._V, D)
        delays, info, rclear = _delay_out(self._P, self._V)
        self._ck(self.lib.cfz_loop_plan_delays(self._h, D, margin, slack, _ptr(cap), _ptr(delays), _ptr(info), _ptr(rclear)), "cfz_loop_plan_delays")
        return _delay_dict(delays, info, rclear)

    def plan_coordination(self, tables, margin=None, length=None):
        """`cfz_plan_coordination`: the coordination diagrams of the plan sets tables [P,V,T,7] (or one set [V,T,7]: P = 1) ->
        dict(blocked [P, npair, T, T] bool, pairs [npair, 2] (u < w)).  blocked[p, q, i, j]: the body of u at its sample i and the body of
        w at its sample j are closer than margin [m] (None: the problem's `dmin`); False beyond length [V] or [P, V] (None: T).  The
        conflict map's count at lag tau is the sum of the diagram along the samples of that lag."""
        tables = np.ascontiguousarray(tables, dtype=np.float64)
        if tables.ndim == 3:
            tables = tables[None]
        if tables.ndim != 4 or tables.shape[3] != 7 or 0 in tables.shape:
            raise ValueError(f"expected tables of shape [P, V, T, 7] or [V, T, 7], got {tables.shape}")
        P, V, T = tables.shape[:3]
        npair, nw = V * (V - 1) // 2, (T + 31) // 32
        words = np.zeros((P, npair, T, nw), np.uint32)
        self._ck(self.lib.cfz_plan_coordination(self._h, P, V, T, _ptr(tables), _ptr(_length_arg(length, P, V)),
                                                float(self.spec.dmin if margin is None else margin), _ptr(words)), "cfz_plan_coordination")
        bits = np.unpackbits(words.view(np.uint8), axis=-1, bitorder="little")[..., :T].astype(bool)  # (little-endian words)
        pairs = np.array([(u, w) for u in range(V) for w in range(u + 1, V)], np.int32).reshape(-1, 2)
        return dict(blocked=bits, pairs=pairs)

    def plan_schedule(self, tables, hold, horizon=None, margin=None, slack=0, orders=None, length=None):
        """`cfz_plan_schedule`: hold-point schedules that make every plan set of tables [P,V,T,7] (or one set [V,T,7]) conflict-free ->
        dict(schedule [P, V, H] int32 (the sample of vehicle v at step t; -1: no order is feasible), arrival [P, V] (the first step at the
        goal sample), waits [P, V] (steps spent waiting before it), found [P] bool, order [P] (the index of the winning order), makespan
        [P] (the largest arrival), total [P] (their sum), feasible_orders [P]).  hold [V, T] or [P, V, T]: non-zero where a vehicle may
        wait for any number of steps (`scenarios.hold_points`; the goal sample length - 1 always, `scenarios.plan_lengths`).  The vehicles
        are scheduled one after the other in a priority order, each arriving as early as the earlier ones' schedules allow and waiting
        as late as possible, with `slack` samples of timing error tolerated around every step; over `orders` (None: all V! for V <= 4)
        the answer is the smallest under (makespan, total, index).  horizon None: T + 64 steps.  `scenarios.schedule_tables(tables,
        schedule)` gives the tables `loop_init` takes."""
        tables = np.ascontiguousarray(tables, dtype=np.float64)
        if tables.ndim == 3:
            tables = tables[None]
        if tables.ndim != 4 or tables.shape[3] != 7 or 0 in tables.shape:
            raise ValueError(f"expected tables of shape [P, V, T, 7] or [V, T, 7], got {tables.shape}")
        P, V, T = tables.shape[:3]
        hold, H, margin, slack, orders, length = _schedule_args(hold, horizon, margin, slack, orders, length, P, V, T, self.spec)
        out = _schedule_out(P, V, max(H, 1))
        self._ck(self.lib.cfz_plan_schedule(self._h, P, V, T, _ptr(tables), _ptr(length), _ptr(hold), H, margin, slack, len(orders), _ptr(orders),
                                            *(_ptr(a) for a in out)), "cfz_plan_schedule")
        return _schedule_dict(*out)

    def loop_plan_schedule(self, hold, horizon=None, margin=None, slack=0, orders=None, length=None):
        """`cfz_loop_plan_schedule`: `plan_schedule` of the pool that `loop_init` left on the device (nothing is uploaded but the hold
        mask, the lengths and the orders; the loop is left as it is) -> the same dict, P the pool's."""
        P, V, T = self._P, self._V, self._T
        if not P:  # (the library refuses the call; it reads none of the arrays first)
            self._ck(self.lib.cfz_loop_plan_schedule(self._h, None, None, 1, 0.0, 0, 1, None, None, None, None, None), "cfz_loop_plan_schedule")
        hold, H, margin, slack, orders, length = _schedule_args(hold, horizon, margin, slack, orders, length, P, V, T, self.spec)
        out = _schedule_out(P, V, max(H, 1))
        self._ck(self.lib.cfz_loop_plan_schedule(self._h, _ptr(length), _ptr(hold), H, margin, slack, len(orders), _ptr(orders), *(_ptr(a) for a in out)),
                 "cfz_loop_plan_schedule")
        return _schedule_dict(*out)

    def loop_last_converged(self):
        """Solves of the last `loop_run` that converged (status 0)."""
        return int(self.lib.cfz_loop_last_converged(self._h))

    def loop_last_status_counts(self):
        """How the solves of the last `loop_run` ended: [6] counts of status 0..5."""
        c = np.zeros(6, dtype=np.int64)
        self._ck(self.lib.cfz_loop_last_status_counts(self._h, c.ctypes.data_as(C.c_void_p)), "cfz_loop_last_status_counts")
        return c

    def loop_get(self):
        S, V, N = self._S, self._V, self.spec.N
        out = dict(state=np.empty((S, V, 5)), pred=np.empty((S, V, 7, N)), status=np.empty((S, V), np.int32),
                   iters=np.empty((S, V), np.int32))
        self._ck(self.lib.cfz_loop_get(self._h, _ptr(out["state"]), _ptr(out["pred"]), _ptr(out["status"]),
                                       _ptr(out["iters"])), "cfz_loop_get")
        return out
