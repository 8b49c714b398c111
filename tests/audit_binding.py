"""The audit of a realised trajectory, twice: a ctypes binding of the test-only CPU build of the kernel source
(tests/emu/cfz_audit_emu.cpp over conflict_rez_amd/csrc/cfz_audit.inl), and an independent numpy statement of the same
definitions (vertex-edge distances, separating-axis overlaps) that both the CPU build and the GPU kernel are checked against."""
import ctypes as C

import numpy as np

from emu_build import load, ptr

_i, _d, _vp = C.c_int, C.c_double, C.c_void_p
PROTOTYPES = {  # of tests/emu/cfz_audit_emu.cpp
    "cfz_emu_signed_distance": (_d, [_vp, _vp]),
    "cfz_emu_audit": (_i, [_i, _i, _i, _vp, _vp, _i, _vp, _vp, _d, _d, _d, _i, _vp, _vp, _vp, _vp]),
}


def lib():
    return load("cfz_audit_emu", ("tests/emu/cfz_audit_emu.cpp", "conflict_rez_amd/csrc/cfz_audit.inl", "conflict_rez_amd/csrc/cfz_wave.inl"), PROTOTYPES)


def emu_signed_distance(P, Q):
    P = np.ascontiguousarray(P, float).reshape(4, 2); Q = np.ascontiguousarray(Q, float).reshape(4, 2)
    return float(lib().cfz_emu_signed_distance(ptr(P), ptr(Q)))


def emu_audit(traj, goal, obs, g, pos_tol, psi_tol, v_tol, lanes=64):
    traj = np.ascontiguousarray(traj, float); goal = np.ascontiguousarray(goal, float)
    obs = np.ascontiguousarray(np.asarray(obs, float).reshape(-1, 4, 2)); g = np.ascontiguousarray(g, float)
    K, S, V = traj.shape[:3]
    out = dict(clear=np.empty((S, 2)), where=np.empty((S, 6), np.int32), first_contact=np.empty(S, np.int32), arrive=np.empty((S, V), np.int32))
    rc = lib().cfz_emu_audit(K, S, V, ptr(traj), ptr(goal), len(obs), ptr(obs) if len(obs) else None, ptr(g), pos_tol, psi_tol, v_tol, lanes,
                             ptr(out["clear"]), ptr(out["where"]), ptr(out["first_contact"]), ptr(out["arrive"]))
    assert rc == 0
    return out


# ---- numpy reference ---------------------------------------------------------------------------------------------------------
def body(g, x, y, psi):
    """[..., 4, 2] corners of the rectangle g = (front, left, rear, right) at (x, y, psi)."""
    x, y, psi = np.asarray(x, float), np.asarray(y, float), np.asarray(psi, float)
    BV = np.array([[g[0], g[1]], [-g[2], g[1]], [-g[2], -g[3]], [g[0], -g[3]]], float)
    c, s = np.cos(psi)[..., None], np.sin(psi)[..., None]
    return np.stack([x[..., None] + c * BV[:, 0] - s * BV[:, 1], y[..., None] + s * BV[:, 0] + c * BV[:, 1]], -1)


def obstacle_vertices(A, b):
    """Corners of {p: A p <= b} (four half-planes), in order around the polygon."""
    A, b = np.asarray(A, float), np.asarray(b, float)
    ang = np.argsort(np.arctan2(A[:, 1], A[:, 0]))
    return np.array([np.linalg.solve(A[[ang[i], ang[(i + 1) % 4]]], b[[ang[i], ang[(i + 1) % 4]]]) for i in range(4)])


def _vertex_edge(A, B):  # [...] smallest distance of a vertex of A to an edge of B
    e = np.roll(B, -1, axis=-2) - B
    w = A[..., :, None, :] - B[..., None, :, :]
    ee = (e * e).sum(-1)[..., None, :]
    t = np.clip(np.where(ee > 0, (w * e[..., None, :, :]).sum(-1) / np.where(ee > 0, ee, 1.0), 0.0), 0.0, 1.0)
    d = w - t[..., None] * e[..., None, :, :]
    return np.sqrt((d * d).sum(-1).min((-1, -2)))


def _overlap(P, Q):  # [...] smallest projection overlap over the unit face normals of both polygons
    best = None
    for F in (P, Q):
        e = np.roll(F, -1, axis=-2) - F
        n = np.stack([e[..., 1], -e[..., 0]], -1) / np.linalg.norm(e, axis=-1)[..., None]  # [..., 4, 2]
        hp = np.einsum("...vk,...ek->...ev", P, n); hq = np.einsum("...vk,...ek->...ev", Q, n)
        o = np.minimum(hp.max(-1) - hq.min(-1), hq.max(-1) - hp.min(-1)).min(-1)
        best = o if best is None else np.minimum(best, o)
    return best


def signed_distance(P, Q):
    """Signed distance of convex quadrilaterals P, Q [..., 4, 2]: distance if disjoint, else minus the penetration depth."""
    P, Q = np.broadcast_arrays(np.asarray(P, float), np.asarray(Q, float))
    o = _overlap(P, Q)
    d = np.minimum(_vertex_edge(P, Q), _vertex_edge(Q, P))
    return np.where(o >= 0.0, -np.maximum(o, 0.0) + 0.0, d)


def audit(traj, goal, obs, g, pos_tol, psi_tol, v_tol):
    """The audit's outputs (include/confrez_hip.h, cfz_audit) from their definitions."""
    traj = np.asarray(traj, float)
    K, S, V = traj.shape[:3]
    obs = np.asarray(obs, float).reshape(-1, 4, 2)
    W = body(g, traj[..., 0], traj[..., 1], traj[..., 2])  # [K, S, V, 4, 2]
    out = dict(clear=np.full((S, 2), np.inf), where=np.full((S, 6), -1, np.int32), first_contact=np.full(S, -1, np.int32),
               arrive=np.full((S, V), -1, np.int32))
    pairs = [(u, w) for u in range(V) for w in range(u + 1, V)]
    for s in range(S):
        first = K
        if pairs:
            D = np.stack([signed_distance(W[:, s, u], W[:, s, w]) for u, w in pairs], 1)  # [K, npair]
            t, p = np.unravel_index(np.argmin(D), D.shape)  # row-major: lowest step, then lowest pair
            out["clear"][s, 0] = D[t, p]; out["where"][s, :3] = (t, *pairs[p])
            neg = np.flatnonzero((D < 0).any(1))
            first = min(first, neg[0]) if len(neg) else first
        if len(obs):
            D = signed_distance(W[:, s, :, None], obs[None, None])  # [K, V, n_obs]
            t, v, j = np.unravel_index(np.argmin(D), D.shape)
            out["clear"][s, 1] = D[t, v, j]; out["where"][s, 3:] = (t, v, j)
            neg = np.flatnonzero((D < 0).any((1, 2)))
            first = min(first, neg[0]) if len(neg) else first
        out["first_contact"][s] = first if first < K else -1
        z, gl = traj[:, s], np.asarray(goal, float)[s]
        e = z[..., 2] - gl[:, 2]
        e = e - 2 * np.pi * np.rint(e / (2 * np.pi))
        ok = ((z[..., 0] - gl[:, 0]) ** 2 + (z[..., 1] - gl[:, 1]) ** 2 <= pos_tol ** 2) & (np.abs(e) <= psi_tol) & (np.abs(z[..., 3]) <= v_tol)
        for v in range(V):
            hit = np.flatnonzero(ok[:, v])
            out["arrive"][s, v] = hit[0] if len(hit) else -1
    return out
