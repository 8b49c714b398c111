"""LQ stage data for the Newton step's backward sweeps and lane scans, chosen by us, with their solutions to extended precision.

The interior-point solvers compute every Newton step with four functions that exist in the device pass only: the MPC step's backward sweep
on the matrix cores (`cfz::riccati_backward_mfma`), its forward and costate scans over the lanes (`cfz::forward_scan`, `cfz::costate_scan`)
and the `state_ws` sweep (`cfzp::riccati_backward_mfma`).  This module states the SYSTEM those functions see, in the product's own packing,
and solves it in the textbook form -- not the homogeneous form the kernels use, so that the tables `ric_T` / `ric_H` / `pl_T` / `pl_H` are
checked against something that was not read off them.

MPC step (`MpcSystem`, N stages, 2 <= N <= 32), variables w_k = (z_k (5), u_k (2)):
    min  sum_k  w_k' H_k w_k / 2 + g_k' w_k,   z_0 = x0 - p0,   z_{k+1} = A_k z_k + B_k u_k + d_k  (k < N - 1),
stage N - 1 without dynamics, its input free.  Packing (cfz_solver.inl): `ab[k]` 15 sensitivities, rows 0..2 of [A - I | B] five a row:
(r, 0..2) = A[r][2..4], (r, 3..4) = B[r][0..1], with ab[k][10] the entry s20 = 1 that nothing reads and ab[k][11..12] = A[2][3..4];
rows 3, 4 of A are the identity's and B[3][0] = B[4][1] = dt.  `hc[k]` 11 Hessian entries: the diagonal h0..h6, h7 (0,1), h8 (0,2), h9 (1,2)
and h10 (3,6); `gk[k]` the gradient; `d[k]` the defect.  Multipliers: pi0 of the row z_0 - (x0 - p0) = 0, pi_k of A_k z_k + B_k u_k + d_k -
z_{k+1} = 0; the step's outputs are dp = w, dpi0 = lambda_0 - pi0, dpi_k = lambda_{k+1} - pi_k.  Gains: kk[k] = K (2 x 5 by rows), then the two
feed-forward terms; value function of stage 0: P (5 x 5 by rows), p (5).

`state_ws` sweep (`PlanSystem`, T stages of kSt = 33 words, terminal data at index T): st[k] = a02 a03 a12 a13 a23 a24 | q0..q4 q23 q34 | r0 r1 |
gz[5] gu[2] | c[5] | q0 q1 q2 with the pose block E of a cell end added | E01 E02 E12; z+ = A z + dt (e_3 u0 + e_4 u1) + c.  The sweep runs
k = T - 1 .. 1 from P_T = Q_T + E_T, p1_T = gz_T, p2_T = -e_psi when `has_final`, else 0; fb[k] = K (2 x 5) kk[2] kl[2] (kl answers the border
vector p2), vf[k] = P's upper triangle by rows (15), p1, p2.

References: `mpc_kkt` assembles the dense KKT system of the LQ problem and solves it with LAPACK, refined with residuals in longdouble;
`mpc_recursion` / `plan_recursion` are the Riccati recursions, in longdouble (the reference of the gains and value functions) or in float64
(a model: what the ALGORITHM costs in accuracy, whatever the order of its sums).  `plan_homogeneous` is the float64 recursion in the
homogeneous form of the matrix-core sweep, with the accumulator used as it stands (`transposed`) and the per-stage symmetrisation that
this use needs (`symmetrise`): without it the antisymmetric part of the rounding grows over a long horizon, and the `long` family shows it.

`yardstick(system, cpu_build)`: per output group the relative error max |x - ref| / max |ref| of two float64 models on THAT system, the CPU
build of the product source (passed in: tests/sweeps_binding.py) and the plain numpy recursion; the bound of a group is 32 x max(those
errors, 2^-52).  No bound may exceed BOUND_CAP and no yardstick YARD_CAP: conditions on the generator."""
import numpy as np

LD = np.longdouble
KST, KFB, KVF = 33, 14, 25
MPC_FAMILIES = ("benign", "barrier", "flat")
PLAN_FAMILIES = ("benign", "barrier", "flat", "long")
MPC_GROUPS = ("kk", "vf", "dp", "dpi0", "dpi")
PLAN_GROUPS = ("fb", "vf")
BOUND_CAP, YARD_CAP = 1e-9, 3e-11
EPS = 2.0 ** -52
LONG_T = 300
_FAMILY_ID = {"benign": 1, "barrier": 2, "flat": 3, "long": 4}


def rel_err(x, ref):
    x, ref = np.asarray(x, LD), np.asarray(ref, LD)
    if not np.isfinite(np.asarray(x, float)).all():
        return np.inf
    if not np.abs(ref).max() > 0:  # (a group nothing writes: state_ws' fb at T = 1)
        return 0.0 if not np.abs(x).max() > 0 else np.inf
    return float(np.abs(x - ref).max() / np.abs(ref).max())


# ---------------------------------------------------------------------------------------------------------------- MPC step
class MpcSystem:
    def __init__(self, ab, d, hc, gk, x0, p0, pi0, pi, dt, family, seed):
        self.ab, self.d, self.hc, self.gk, self.x0, self.p0, self.pi0, self.pi = ab, d, hc, gk, x0, p0, pi0, pi
        self.dt, self.family, self.seed, self.N = dt, family, seed, len(hc)
        self.z0 = x0 - p0  # one float64 subtraction, as forward_scan forms it
        for a in (ab, d, hc, gk, x0, p0, pi0, pi):
            a.setflags(write=False)

    def A(self, k, dtype=float):
        s, A = self.ab[k], np.eye(5, dtype=dtype)
        A[0, 2:5] += s[0:3]; A[1, 2:5] += s[5:8]; A[2, 3:5] += s[11:13]
        return A

    def B(self, k, dtype=float):
        s, B = self.ab[k], np.zeros((5, 2), dtype)
        B[0], B[1], B[2] = s[3:5], s[8:10], s[13:15]
        B[3, 0] = B[4, 1] = self.dt
        return B

    def H(self, k, dtype=float):
        h, H = self.hc[k], np.zeros((7, 7), dtype)
        H[np.arange(7), np.arange(7)] = h[:7]
        for (i, j), v in zip(((0, 1), (0, 2), (1, 2), (3, 6)), h[7:11]):
            H[i, j] = H[j, i] = v
        return H


def _pose_offdiag(rng, h, c):
    """h7 h8 h9 = c_ij sqrt(h_i h_j) with |c_ij| <= c < 1/2: the pose block stays positive definite (Gershgorin on the scaled block)."""
    r = rng.uniform(-c, c, 3)
    return np.array([r[0] * np.sqrt(h[0] * h[1]), r[1] * np.sqrt(h[0] * h[2]), r[2] * np.sqrt(h[1] * h[2])])


def generate_mpc(family, N, seed):
    """The stage data of an MPC step of `family`; the same (family, N, seed) gives the same system."""
    assert family in MPC_FAMILIES and 2 <= N <= 32
    rng = np.random.default_rng([11, _FAMILY_ID[family], N, seed])
    dt = 0.1
    ab = np.zeros((N, 15))
    # dt v cos, dt sin, ... of the model: a few tenths.  (`barrier` a third of that: the sweep takes its accumulator as it stands, which is its
    # transpose, and does not symmetrise it; what the two triangles differ by grows with the sensitivities, and with the model's it takes the
    # CPU build of the sweep past YARD_CAP at N = 32 -- 2e-10 in the gains, the value function 1e-10 from symmetric.)
    sens = 0.1 if family == "barrier" else 0.3
    ab[:, [0, 1, 2, 5, 6, 7, 11, 12]] = rng.uniform(-sens, sens, (N, 8))
    ab[:, [3, 4, 8, 9, 13, 14]] = rng.uniform(-0.02, 0.02, (N, 6))      # the inputs' second-order reach into the pose
    ab[:, 10] = 1.0
    d = 1e-2 * rng.standard_normal((N, 5))
    hc = np.zeros((N, 11))
    for k in range(N):
        if family == "benign":
            h = rng.uniform(0.5, 5.0, 7)
        elif family == "barrier":  # late interior-point iterations: some rows' barrier terms are huge, others have died away
            h = 10.0 ** rng.uniform(-4.0, 8.0, 7)
            h[5:7] = 10.0 ** rng.uniform(-1.0, 8.0, 2)  # (tamed: inputs without curvature of their own are the `flat` family's)
        else:  # flat: the inputs' own curvature a fraction of dt^2 P, which M_ee then lives on (tamed: from 1e-6 down the drift above passes YARD_CAP)
            h = rng.uniform(0.5, 5.0, 7)
            h[5:7] = 10.0 ** rng.uniform(-2.0, -1.0, 2)
        hc[k, :7] = h
        hc[k, 7:10] = _pose_offdiag(rng, h, 0.3)
        hc[k, 10] = rng.uniform(-0.5, 0.5) * np.sqrt(h[3] * h[6])
    gk = rng.standard_normal((N, 7)) * np.sqrt(hc[:, :7]) if family == "barrier" else rng.standard_normal((N, 7))
    x0, p0 = rng.standard_normal(5), rng.standard_normal(5)
    return MpcSystem(ab, d, hc, gk, x0, x0 - 0.1 * p0, 0.1 * rng.standard_normal(5), 0.1 * rng.standard_normal((N, 5)), dt, family, seed)


def mpc_recursion(s, dtype=LD):
    """Backward Riccati recursion, forward pass and costates in the textbook form, every operation in `dtype` -> dict of the output groups."""
    N = s.N
    f = lambda a: np.asarray(a, dtype)
    P, p = np.zeros((5, 5), dtype), np.zeros(5, dtype)
    kk = np.zeros((N, 12), dtype)
    for k in range(N - 1, -1, -1):
        H, g = s.H(k, dtype), f(s.gk[k])
        if k < N - 1:
            A, B = s.A(k, dtype), s.B(k, dtype)
            h = p + P @ f(s.d[k])
            Hzz, Huz, Huu = H[:5, :5] + A.T @ P @ A, H[5:, :5] + B.T @ P @ A, H[5:, 5:] + B.T @ P @ B
            hz, hu = g[:5] + A.T @ h, g[5:] + B.T @ h
        else:
            Hzz, Huz, Huu, hz, hu = H[:5, :5], H[5:, :5], H[5:, 5:], g[:5], g[5:]
        det = Huu[0, 0] * Huu[1, 1] - Huu[0, 1] * Huu[1, 0]
        inv = np.array([[Huu[1, 1], -Huu[0, 1]], [-Huu[1, 0], Huu[0, 0]]], dtype) / det
        K, kf = -inv @ Huz, -inv @ hu
        kk[k, :10], kk[k, 10:] = K.ravel(), kf
        P, p = Hzz + Huz.T @ K, hz + Huz.T @ kf
        P = (P + P.T) / 2
    dp = np.zeros((N, 7), dtype)
    z = f(s.z0)
    dpi0 = -(P @ z + p) - f(s.pi0)
    for k in range(N):
        u = kk[k, :10].reshape(2, 5) @ z + kk[k, 10:]
        dp[k, :5], dp[k, 5:] = z, u
        if k < N - 1:
            z = s.A(k, dtype) @ z + s.B(k, dtype) @ u + f(s.d[k])
    lam = np.zeros((N - 1, 5), dtype)
    nxt = np.zeros(5, dtype)
    for k in range(N - 1, 0, -1):
        q = (s.H(k, dtype) @ dp[k] + f(s.gk[k]))[:5]
        lam[k - 1] = q + (s.A(k, dtype).T @ nxt if k < N - 1 else 0)
        nxt = lam[k - 1]
    return dict(kk=kk, vf=np.concatenate([P.ravel(), p]), dp=dp, dpi0=dpi0, dpi=lam - f(s.pi[: N - 1]))


def mpc_kkt(s):
    """The LQ problem's KKT system [[H G'], [G 0]] [w; lam] = [-g; r], assembled densely and solved by LAPACK; -> (float64 solution as LAPACK
    leaves it, the same refined with longdouble residuals), each as dict(dp, dpi0, dpi).  The primal variables are scaled by 1 / sqrt(H_ii)
    first: the barrier family's spread of magnitudes is a matter of units, not of conditioning."""
    N = s.N
    n, m = 7 * N, 5 * N
    Kd, rhs = np.zeros((n + m, n + m)), np.zeros(n + m)
    for k in range(N):
        Kd[7 * k : 7 * k + 7, 7 * k : 7 * k + 7] = s.H(k)
        rhs[7 * k : 7 * k + 7] = -s.gk[k]
    Kd[n : n + 5, :5] = np.eye(5)
    rhs[n : n + 5] = s.z0
    for k in range(N - 1):
        r = n + 5 * (k + 1)
        Kd[r : r + 5, 7 * k : 7 * k + 5], Kd[r : r + 5, 7 * k + 5 : 7 * k + 7] = s.A(k), s.B(k)
        Kd[r : r + 5, 7 * (k + 1) : 7 * (k + 1) + 5] = -np.eye(5)
        rhs[r : r + 5] = -s.d[k]
    Kd[:n, n:] = Kd[n:, :n].T
    sc = np.ones(n + m)
    sc[:n] = 1.0 / np.sqrt(np.diag(Kd)[:n])
    Ks = Kd * sc[:, None] * sc[None, :]
    Kl, bl = Ks.astype(LD), (rhs * sc).astype(LD)
    y0 = np.linalg.solve(Ks, rhs * sc)
    y, best = y0.astype(LD), np.inf
    for _ in range(12):
        r = bl - Kl @ y
        rn = float(np.abs(r).max())
        if not rn < 0.5 * best:
            break
        best = rn
        y = y + np.linalg.solve(Ks, r.astype(float)).astype(LD)

    def unpack(v):
        x = v * sc.astype(v.dtype)
        lam = x[n:].reshape(N, 5)
        return dict(dp=x[:n].reshape(N, 7), dpi0=lam[0] - s.pi0.astype(v.dtype), dpi=lam[1:] - s.pi[: N - 1].astype(v.dtype))

    return unpack(y0), unpack(y)


# ---------------------------------------------------------------------------------------------------------------- state_ws sweep
class PlanSystem:
    def __init__(self, st, has_final, dt, family, seed):
        self.st, self.has_final, self.dt, self.family, self.seed, self.T = st, int(has_final), dt, family, seed, len(st) - 1
        st.setflags(write=False)

    def ce(self):
        """The pose blocks as the one-lane sweep reads them with a cell of one stage (PSpec.N = 1, n_chk = T): ce[k - 1] = E00 E01 E02 E11 E12 E22."""
        s = self.st[1:]
        return np.ascontiguousarray(np.stack([s[:, 27] - s[:, 6], s[:, 30], s[:, 31], s[:, 28] - s[:, 7], s[:, 32], s[:, 29] - s[:, 8]], 1))

    def A(self, k, dtype=float):
        s, A = self.st[k], np.eye(5, dtype=dtype)
        A[0, 2], A[0, 3], A[1, 2], A[1, 3], A[2, 3], A[2, 4] = s[0:6]
        return A

    def Q(self, k, dtype=float):
        s, Q = self.st[k], np.zeros((5, 5), dtype)
        Q[np.arange(5), np.arange(5)] = [s[27], s[28], s[29], s[9], s[10]]
        for (i, j), v in zip(((0, 1), (0, 2), (1, 2), (2, 3), (3, 4)), (s[30], s[31], s[32], s[11], s[12])):
            Q[i, j] = Q[j, i] = v
        return Q


def generate_plan(family, T, seed, has_final=1):
    """The stage data of a `state_ws` Newton step of `family`, built as riccati_prepare builds it from an iterate: headings, speeds and steering
    angles of a drive through a parking lot."""
    assert family in PLAN_FAMILIES and T >= 1 and (family != "long" or T == LONG_T)
    rng = np.random.default_rng([13, _FAMILY_ID[family], T, seed, int(has_final)])
    dt, wb = 0.1, 2.7
    st = np.zeros((T + 1, KST))
    psi = np.cumsum(rng.uniform(-0.05, 0.05, T + 1)) + rng.uniform(-np.pi, np.pi)
    v, dl = rng.uniform(0.5, 2.0, T + 1) * rng.choice([-1.0, 1.0]), rng.uniform(-0.5, 0.5, T + 1)
    tn = np.tan(dl)
    st[:, 0], st[:, 1], st[:, 2], st[:, 3] = -dt * v * np.sin(psi), dt * np.cos(psi), dt * v * np.cos(psi), dt * np.sin(psi)
    st[:, 4], st[:, 5] = dt * tn / wb, dt * v / wb * (1 + tn * tn)
    if family == "barrier":
        q = 10.0 ** rng.uniform(-4.0, 8.0, (T + 1, 7))
        q[:, 5:] = 10.0 ** rng.uniform(-1.0, 8.0, (T + 1, 2))  # (tamed as the MPC family is: with 1e-4 the models reach 3e-11 at T = 300)
    else:
        q = rng.uniform(0.5, 5.0, (T + 1, 7))
        if family == "flat":
            q[:, 5:] = 10.0 ** rng.uniform(-7.0, -6.0, (T + 1, 2))
        if family == "long":  # a damped plan: weights on the state of the inputs' size keep the closed loop's memory short over 300 stages
            q[:, 5:] = rng.uniform(0.05, 0.5, (T + 1, 2))
    st[:, 6:11], st[:, 13:15] = q[:, :5], q[:, 5:]
    st[:, 11] = rng.uniform(-0.3, 0.3, T + 1) * np.sqrt(q[:, 2] * q[:, 3])
    st[:, 12] = rng.uniform(-0.3, 0.3, T + 1) * np.sqrt(q[:, 3] * q[:, 4])
    sq = np.sqrt(q) if family == "barrier" else np.ones_like(q)
    st[:, 15:22] = rng.standard_normal((T + 1, 7)) * sq
    st[:, 22:27] = 1e-2 * rng.standard_normal((T + 1, 5))
    # the pose block of a cell end, at every stage (the sweep on the matrix cores reads it wherever it stands): E = G' S G, positive semidefinite
    G = rng.standard_normal((T + 1, 3, 3)) * np.sqrt(0.3 * q[:, None, :3])
    E = np.einsum("kri,krj->kij", G, G) / 3.0
    st[:, 27], st[:, 28], st[:, 29] = q[:, 0] + E[:, 0, 0], q[:, 1] + E[:, 1, 1], q[:, 2] + E[:, 2, 2]
    st[:, 30], st[:, 31], st[:, 32] = E[:, 0, 1], E[:, 0, 2], E[:, 1, 2]
    for a in (slice(0, 6), slice(11, 15), slice(20, 27)):  # the terminal stage has no input, no dynamics and no cross terms (riccati_prepare)
        st[T, a] = 0.0
    return PlanSystem(st, has_final, dt, family, seed)


def singular_plan(T, seed):
    """A `benign` system whose M_ee is exactly singular at stage T - 1: no input curvature there, and a terminal value function without v, delta."""
    s = generate_plan("benign", T, seed)
    st = s.st.copy()
    st[T - 1, 13:15] = 0.0
    st[T, 9:11] = 0.0
    return PlanSystem(st, s.has_final, s.dt, "singular", seed)


def plan_recursion(s, dtype=LD):
    """The sweep in the textbook form, every operation in `dtype` -> dict(fb [T + 1, 14], vf [T + 1, 25], flag); rows 0 of fb, vf and row T
    of fb are not written by any sweep and stay zero."""
    T, dt = s.T, dtype(s.dt)
    f = lambda a: np.asarray(a, dtype)
    iu = np.triu_indices(5)
    fb, vf = np.zeros((T + 1, KFB), dtype), np.zeros((T + 1, KVF), dtype)
    B = np.zeros((5, 2), dtype)
    B[3, 0] = B[4, 1] = dt
    P, p1, p2 = s.Q(T, dtype), f(s.st[T, 15:20]), np.zeros(5, dtype)
    if s.has_final:
        p2[2] = -1
    vf[T] = np.concatenate([P[iu], p1, p2])
    for k in range(T - 1, 0, -1):
        A, st = s.A(k, dtype), f(s.st[k])
        h = p1 + P @ st[22:27]
        Huu, Huz, hu = np.diag(st[13:15]) + B.T @ P @ B, B.T @ P @ A, st[20:22] + B.T @ h
        det = Huu[0, 0] * Huu[1, 1] - Huu[0, 1] * Huu[1, 0]
        if not (det != 0 and np.isfinite(float(det))):
            return dict(fb=fb, vf=vf, flag=1)
        inv = np.array([[Huu[1, 1], -Huu[0, 1]], [-Huu[1, 0], Huu[0, 0]]], dtype) / det
        K, kk, kl = -inv @ Huz, -inv @ hu, -inv @ (B.T @ p2)
        fb[k] = np.concatenate([K.ravel(), kk, kl])
        p1, p2 = st[15:20] + A.T @ h + Huz.T @ kk, A.T @ p2 + Huz.T @ kl
        P = s.Q(k, dtype) + A.T @ P @ A + Huz.T @ K
        P = (P + P.T) / 2
        vf[k] = np.concatenate([P[iu], p1, p2])
    return dict(fb=fb, vf=vf, flag=0)


_VAR = (0, 1, 2, 3, 4, 5, 6, 8, 9)  # the sweep's variables [z (5), 1, e, -, u0, u1] without the unused one


def plan_homogeneous(s, transposed=True, symmetrise=True):
    """The sweep in float64 in the homogeneous form of cfzp::riccati_backward_mfma, stated here from its comment and not from pl_T / pl_H:
    [z+; 1; e] = Tm [z; 1; e; u],  Pt = [[P p1 p2], [p1' . .], [p2' . .]],  M = Tm' Pt Tm + Ht,  Pt <- M_kk - M_ke M_ee^-1 M_ek.  `transposed`:
    the accumulator is used as the first operand as it stands, which is its transpose, and M_ke is read from M_ek's rows; `symmetrise`:
    Pt <- (Pt + Pt') / 2 after every stage."""
    T, dt = s.T, s.dt
    iu = np.triu_indices(5)
    fb, vf = np.zeros((T + 1, KFB)), np.zeros((T + 1, KVF))

    def Ht(k):
        st, H = s.st[k], np.zeros((9, 9))
        H[:5, :5] = s.Q(k)
        H[:5, 5] = H[5, :5] = st[15:20]
        H[7, 7], H[8, 8] = st[13:15]
        H[5, 7:] = H[7:, 5] = st[20:22]
        return H

    P = Ht(T)[:7, :7]
    if s.has_final:
        P[2, 6] = P[6, 2] = -1.0
    vf[T] = np.concatenate([P[:5, :5][iu], P[5, :5], P[6, :5]])
    for k in range(T - 1, 0, -1):
        Tm = np.zeros((7, 9))
        Tm[:5, :5], Tm[:5, 5] = s.A(k), s.st[k, 22:27]
        Tm[5, 5] = Tm[6, 6] = 1.0
        Tm[3, 7] = Tm[4, 8] = dt
        M = Tm.T @ ((P.T if transposed else P) @ Tm) + Ht(k)
        det = M[7, 7] * M[8, 8] - M[7, 8] * M[8, 7]
        if not (det != 0.0 and np.isfinite(det)):
            return dict(fb=fb, vf=vf, flag=1)
        V = np.array([[M[8, 8], -M[7, 8]], [-M[8, 7], M[7, 7]]]) / det @ M[7:, :7]
        fb[k] = np.concatenate([-V[:, :5].ravel(), -V[:, 5], -V[:, 6]])
        P = M[:7, :7] - (M[7:, :7].T if transposed else M[:7, 7:]) @ V
        if symmetrise:
            P = 0.5 * (P + P.T)
        vf[k] = np.concatenate([P[:5, :5][iu], P[5, :5], P[6, :5]])
    return dict(fb=fb, vf=vf, flag=0)


# ---------------------------------------------------------------------------------------------------------------- yardsticks
def mpc_reference(s):
    """dict over MPC_GROUPS in longdouble: gains and value function from the recursion, the step from the refined KKT solution; `kkt_gap`: how far
    the recursion's own step is from the KKT solution (two routes to one answer: a check of both, far below any bound)."""
    rec, (_, kkt) = mpc_recursion(s, LD), mpc_kkt(s)
    ref = dict(kk=rec["kk"], vf=rec["vf"], dp=kkt["dp"], dpi0=kkt["dpi0"], dpi=kkt["dpi"])
    ref["kkt_gap"] = max(rel_err(rec[g], kkt[g]) for g in ("dp", "dpi0", "dpi"))
    return ref


def _yard(groups, ref, models):
    y = dict(ref=ref)
    for name, out in models.items():
        y["err_" + name] = {g: rel_err(out[g], ref[g]) for g in groups}
    y["yard"] = {g: max([EPS] + [y["err_" + name][g] for name in models]) for g in groups}
    y["bound"] = {g: 32.0 * y["yard"][g] for g in groups}
    return y


def yardstick_mpc(s, cpu_build):
    """cpu_build(system) -> dict over MPC_GROUPS: the CPU build of the product source (sweep, forward scan, costate scan on one workspace)."""
    return _yard(MPC_GROUPS, mpc_reference(s), dict(cpu=cpu_build(s), model=mpc_recursion(s, np.float64)))


def yardstick_plan(s, cpu_build):
    """cpu_build(system) -> dict(fb, vf, flag): the CPU build of cfzp::riccati_backward_dense as the matrix-core sweep runs it."""
    return _yard(PLAN_GROUPS, plan_recursion(s, LD), dict(cpu=cpu_build(s), model=plan_homogeneous(s)))


def yardstick(system, cpu_build):
    return (yardstick_mpc if isinstance(system, MpcSystem) else yardstick_plan)(system, cpu_build)
