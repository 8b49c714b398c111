"""The score of a realised closed loop, twice: a ctypes binding of the test-only CPU build of the kernel source
(tests/emu/cfz_score_emu.cpp over conflict_rez_amd/csrc/cfz_score.inl, the lanes per vehicle as an argument), and an independent numpy
statement of the definitions of include/confrez_hip.h ("score of a realised trajectory") with plain per-vehicle loops -- no chunks, no
ordered merges -- that both the CPU build and the GPU kernel are checked against.  Also the synthetic records both test modules use."""
import ctypes as C
import functools

import numpy as np

import audit_binding as ab
from emu_build import load, ptr

_i, _d, _vp = C.c_int, C.c_double, C.c_void_p
PROTOTYPES = {  # of tests/emu/cfz_score_emu.cpp
    "cfz_emu_score_group": (_i, [_i]),
    "cfz_emu_score": (_i, [_i, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _d, _d, _d, _d, _i, _vp, _vp]),
}

VAL = ("dx2", "dy2", "psi2", "a2", "vw2", "delta2", "da2", "dw2", "absv", "dev2_max")
CNT = ("steps", "arrive", "failed", "fail_run", "reversals", "waiting", "near_steps", "first_near", "iters_sum", "iters_max", "dev_max_step")
TOL = dict(pos_tol=0.3, psi_tol=0.1, v_tol=0.1)
G = (3.3, 0.9, 0.6, 0.9)  # the default body (front, left, rear, right)
NEAR = 0.5
VS = (1, 2, 3, 4, 5, 8)
KS = (1, 2, 7, 8, 9, 16, 17, 37, 130)


def lib():
    return load("cfz_score_emu", ["tests/emu/cfz_score_emu.cpp"] + ["conflict_rez_amd/csrc/" + f for f in ("cfz_score.inl", "cfz_audit.inl", "cfz_wave.inl")], PROTOTYPES)


def group(V):
    """Lanes per vehicle of score_kernel's wavefront."""
    return int(lib().cfz_emu_score_group(V))


def emu_score(traj, status, iters, tables, table_of, k0, g=G, near=NEAR, lanes=0, **tol):
    """The CPU build with `lanes` lanes per vehicle (0: the kernel's grouping) -> dict(val [S,V,10], cnt [S,V,11])."""
    tol = {**TOL, **tol}
    traj = np.ascontiguousarray(traj, float); tables = np.ascontiguousarray(tables, float)
    K, S, V = traj.shape[:3]
    P, T = tables.shape[0], tables.shape[2]
    status = None if status is None else np.ascontiguousarray(status, np.int32)
    iters = None if iters is None else np.ascontiguousarray(iters, np.int32)
    table_of = np.ascontiguousarray(table_of, np.int32); k0 = np.ascontiguousarray(k0, np.int32); g = np.ascontiguousarray(g, float)
    out = dict(val=np.empty((S, V, len(VAL))), cnt=np.empty((S, V, len(CNT)), np.int32))
    rc = lib().cfz_emu_score(K, S, V, ptr(traj), ptr(status), ptr(iters), P, T, ptr(tables), ptr(table_of), ptr(k0), ptr(g), tol["pos_tol"], tol["psi_tol"],
                             tol["v_tol"], near, lanes, ptr(out["val"]), ptr(out["cnt"]))
    assert rc == 0
    return out


# ---- numpy statement ---------------------------------------------------------------------------------------------------------
def _wrap(e):
    return e - 2 * np.pi * np.rint(e / (2 * np.pi))


def score(traj, status, iters, tables, table_of, k0, g=G, near=NEAR, **tol):
    """val, cnt from their definitions, one vehicle at a time."""
    tol = {**TOL, **tol}
    traj = np.asarray(traj, float); tables = np.asarray(tables, float)
    K, S, V = traj.shape[:3]
    T = tables.shape[2]
    status = np.zeros((K, S, V), np.int32) if status is None else np.asarray(status)
    iters = np.zeros((K, S, V), np.int32) if iters is None else np.asarray(iters)
    W = ab.body(g, traj[..., 0], traj[..., 1], traj[..., 2])  # [K, S, V, 4, 2]
    val, cnt = np.zeros((S, V, len(VAL))), np.zeros((S, V, len(CNT)), np.int32)
    for s in range(S):
        for v in range(V):
            plan, z = tables[table_of[s], v], traj[:, s, v]
            goal = plan[-1]
            at = (((z[:, 0] - goal[0]) ** 2 + (z[:, 1] - goal[1]) ** 2 <= tol["pos_tol"] ** 2) & (np.abs(_wrap(z[:, 2] - goal[2])) <= tol["psi_tol"])
                  & (np.abs(z[:, 3]) <= tol["v_tol"]))
            arrive = int(np.flatnonzero(at)[0]) if at.any() else -1
            upto = arrive + 1 if arrive >= 0 else K
            r = plan[np.minimum(k0[s] + np.arange(K) + 1, T - 1)][:upto]
            z = z[:upto]
            dx, dy, dp = z[:, 0] - r[:, 0], z[:, 1] - r[:, 1], _wrap(z[:, 2] - r[:, 2])
            dev2 = dx ** 2 + dy ** 2
            val[s, v] = [(dx ** 2).sum(), (dy ** 2).sum(), (dp ** 2).sum(), (z[:, 5] ** 2).sum(), ((z[:, 3] * z[:, 6]) ** 2).sum(), (z[:, 4] ** 2).sum(),
                         (np.diff(z[:, 5]) ** 2).sum(), (np.diff(z[:, 6]) ** 2).sum(), np.abs(z[:, 3]).sum(), dev2.max()]
            bad = status[:upto, s, v] != 0
            run = best = 0
            for b in bad:
                run = run + 1 if b else 0
                best = max(best, run)
            sg = np.sign(z[:, 3][np.abs(z[:, 3]) > tol["v_tol"]])
            slow = np.abs(z[:, 3]) <= tol["v_tol"]
            waiting = int(slow.sum()) if arrive < 0 else int(slow[:arrive].sum())
            close = np.zeros(upto, bool)
            for u in range(V):
                if u != v:
                    d = ab.signed_distance(W[:upto, s, v], W[:upto, s, u])
                    close |= (d < near) | (d <= 0)
            it = iters[:upto, s, v]
            cnt[s, v] = [upto, arrive, bad.sum(), best, (sg[1:] != sg[:-1]).sum(), waiting, close.sum(), np.flatnonzero(close)[0] if close.any() else -1,
                         it.sum(), it.max(), int(np.argmax(dev2))]
    return dict(val=val, cnt=cnt)


# ---- synthetic records -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def synthetic(V, K, seed=0):
    """A record of S = 3 scenarios x V vehicles x K steps that follows a pool of two random plan sets loosely: sign runs in v with values
    inside +-v_tol; status drawn with p = 0.5, the last vehicle of scenario 0 failing always and that of scenario 1 never; vehicle 0
    of scenario 0 at its goal from step 0, of scenario 1 at step K - 1, the last vehicle of scenario 2 (V > 1) at step K // 2 and the
    others never; vehicles 0 and 1 of scenario 1 driven through each other; headings a whole number of turns plus at most 1 rad off
    the plan's, so that no wrap is decided near +-pi; plans shorter than k0 + K, so that the clamp is taken.
    -> dict(traj, status, iters, tables, table_of, k0), shared and not to be written to."""
    rng = np.random.default_rng([seed, V, K])
    S, P, T = 3, 2, max(3, K // 2 + 2)
    tables = np.zeros((P, V, T, 7))
    tables[..., 0:2] = rng.uniform(3.0, 30.0, (P, V, T, 2))
    tables[..., 2] = rng.uniform(-1.0, 1.0, (P, V, T))
    table_of = np.array([1, 0, 1], np.int32)
    k0 = np.array([0, 2, 1], np.int32)
    traj = np.zeros((K, S, V, 7))
    for s in range(S):
        rows = np.minimum(k0[s] + np.arange(K) + 1, T - 1)
        traj[:, s] = tables[table_of[s]][:, rows].transpose(1, 0, 2)
    traj[..., 0:2] += rng.normal(0.0, 0.5, (K, S, V, 2))
    traj[..., 2] += rng.uniform(-1.0, 1.0, (K, S, V)) + 2 * np.pi * rng.integers(-1, 2, (K, S, V))
    sign = np.where(np.cumsum(rng.random((K, S, V)) < 0.3, axis=0) % 2 == 0, 1.0, -1.0) * rng.choice([-1.0, 1.0], (S, V))
    traj[..., 3] = np.where(rng.random((K, S, V)) < 0.3, rng.uniform(-TOL["v_tol"], TOL["v_tol"], (K, S, V)), sign * rng.uniform(0.2, 2.0, (K, S, V)))
    traj[..., 4] = rng.uniform(-0.8, 0.8, (K, S, V))
    traj[..., 5] = rng.uniform(-1.5, 1.5, (K, S, V))
    traj[..., 6] = rng.uniform(-1.0, 1.0, (K, S, V))
    if V > 1:  # two bodies through each other, 0.3 m apart sideways
        traj[:, 1, 0, 0] = np.linspace(5.0, 17.0, K); traj[:, 1, 1, 0] = np.linspace(17.0, 5.0, K)
        traj[:, 1, 0, 1] = 10.0; traj[:, 1, 1, 1] = 10.3
    goal = tables[table_of, :, -1]  # [S, V, 7]
    d = np.hypot(traj[..., 0] - goal[None, ..., 0], traj[..., 1] - goal[None, ..., 1])
    traj[..., 0] += np.where(d < 1.0, 3.0, 0.0)  # nobody arrives by chance
    arrivals = [(0, 0, 0), (1, 0, K - 1)] + ([(2, V - 1, K // 2)] if V > 1 else [])
    for s, v, t in arrivals:
        traj[t, s, v, 0:3] = goal[s, v, 0:3] + (0.05, -0.05, 0.02)
        traj[t, s, v, 3] = 0.03
    status = (rng.random((K, S, V)) < 0.5).astype(np.int32) * rng.integers(1, 6, (K, S, V)).astype(np.int32)
    status[:, 0, V - 1] = 2
    status[:, 1, V - 1] = 0
    iters = rng.integers(1, 60, (K, S, V)).astype(np.int32)
    out = dict(traj=traj, status=status, iters=iters, tables=tables, table_of=table_of, k0=k0)
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def synthetic_reference(V, K):
    """The numpy statement on synthetic(V, K): computed once, shared by the tests of both modules."""
    d = synthetic(V, K)
    out = score(d["traj"], d["status"], d["iters"], d["tables"], d["table_of"], d["k0"])
    for a in out.values():
        a.setflags(write=False)
    return out


def check_against_statement(out, ref, rtol=1e-12):
    """Integers equal; doubles within rtol (sums of non-negative terms: the summation error is at most (K + 6) 2^-53, 1.5e-14 at K = 130;
    1e-12 leaves two orders for the different tree); a sum that is exactly 0 in the statement is exactly 0."""
    assert np.array_equal(out["cnt"], ref["cnt"]), np.argwhere(out["cnt"] != ref["cnt"])[:5]
    assert (np.abs(out["val"] - ref["val"]) <= rtol * np.abs(ref["val"])).all()
