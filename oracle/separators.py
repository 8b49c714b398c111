"""Separator systems of the joint plan's structured elimination, chosen by us, and their solutions to extended precision.

`cfz_jstruct.inl` solves the joint separators by block cyclic reduction (`jbcr_*`), a code path that exists in the device pass only.  This module
states the SYSTEM those functions see -- in their storage layout -- and solves it three ways on the CPU:

* `lapack_and_reference`: a float64 LU of the assembled block-tridiagonal matrix (LAPACK's dense `getrf`, or SuperLU for the long systems) --
  its solution as it stands: what an ordinary solver makes of the system -- and the same refined with residuals formed in `numpy.longdouble`
  until the residual stops falling: the solution the kernel is compared with;
* `bcr_model`: the cyclic reduction as the comment above `jbcr_lu_all` states it, in plain numpy with `numpy.linalg.solve` for the blocks:
  what the ALGORITHM costs in accuracy (no pivoting across blocks) whatever the order of its sums.

The larger of the two float64 errors is the yardstick of a system (`yardstick`): the kernel may differ from the reference by a small multiple
of it (another order of the sums, another pivot among equals), never by the 1e-3 a wrong entry makes.

Layout (kJB = 64, kJU = 32, kJL = 28 of cfz_jstruct.inl): blocks 0 .. Nm of 64 rows, 16 per vehicle; `Ds[i]` is block i column-major
(`Ds[i, c * 64 + r]`); `Us[i]` holds 32 columns of 64: columns 0..27 the link with block i + 1, `Us[i, f * 64 + P_i[p]] = C_i[p, f]` with
`K[i: P_i[p], i + 1: F[f]] = C_i[p, f]`, columns 28, 29 the two right-hand sides, 30, 31 spare.  F = {16 b + be} are a block's right-coupled
rows, P_i = {16 a + p0 + c} its pt0 rows (p0 = 7 in block 0, 8 elsewhere; be, c < 7).

Also single 64-row blocks for `lu64_build` (`block_cases`, `tie_block`) with `serial_solve`, block_solve_serial in numpy."""
import numpy as np

KJB, KJU, KJL = 64, 32, 28
FAMILIES = ("spd", "kkt", "ragged")
LINK = 0.5      # size of a link's entries
KKT_REG = 1e-7  # the regularised zero block of the multiplier rows (as the block elimination test's: tests/test_colloc.py)


def rows_F():
    return np.array([16 * (q // 7) + q % 7 for q in range(KJL)])


def rows_P(i):
    p0 = 7 if i == 0 else 8
    return np.array([16 * (q // 7) + p0 + q % 7 for q in range(KJL)])


class System:
    """D[i] (64 x 64, symmetric), C[i] (28 x 28: block i's pt0 rows against block i + 1's right-coupled rows; C[Nm] is unused and zero),
    R[i] (64 x 2).  `present[i, a]`: vehicle a has rows in block i (else identity rows)."""

    def __init__(self, D, C, R, present, family, seed):
        self.D, self.C, self.R, self.present, self.family, self.seed = D, C, R, present, family, seed
        self.Nm = len(D) - 1

    def kernel_arrays(self, spare=0.0):
        """(Ds, Us) as the device functions read them; `spare` fills the columns 30, 31 of every Us block."""
        Nm = self.Nm
        Ds = np.stack([d.T.ravel() for d in self.D])  # column-major
        Us = np.zeros((Nm + 1, KJU, KJB))
        F = rows_F()
        for i in range(Nm + 1):
            if i < Nm:
                Us[i][np.ix_(np.arange(KJL), rows_P(i))] = self.C[i].T  # Us[i][f][P[p]] = C[p][f]
            Us[i][28], Us[i][29] = self.R[i][:, 0], self.R[i][:, 1]
            Us[i][30:] = spare
        assert F.max() < KJB
        return Ds.copy(), Us.reshape(Nm + 1, KJU * KJB).copy()

    def dense(self):
        n = KJB * (self.Nm + 1)
        K = np.zeros((n, n))
        F = rows_F()
        for i in range(self.Nm + 1):
            K[KJB * i : KJB * (i + 1), KJB * i : KJB * (i + 1)] = self.D[i]
            if i < self.Nm:
                r, c = KJB * i + rows_P(i), KJB * (i + 1) + F
                K[np.ix_(r, c)] = self.C[i]
                K[np.ix_(c, r)] = self.C[i].T
        return K

    def sparse(self):
        import scipy.sparse as sps

        F = rows_F()
        rr, cc, vv = [], [], []
        for i in range(self.Nm + 1):
            r, c = np.meshgrid(np.arange(KJB), np.arange(KJB), indexing="ij")
            rr.append(KJB * i + r.ravel()); cc.append(KJB * i + c.ravel()); vv.append(self.D[i].ravel())
            if i < self.Nm:
                r, c = np.meshgrid(KJB * i + rows_P(i), KJB * (i + 1) + F, indexing="ij")
                rr += [r.ravel(), c.ravel()]; cc += [c.ravel(), r.ravel()]; vv += [self.C[i].ravel(), self.C[i].ravel()]
        n = KJB * (self.Nm + 1)
        return sps.csc_matrix((np.concatenate(vv), (np.concatenate(rr), np.concatenate(cc))), shape=(n, n))

    def rhs(self):
        return np.concatenate(self.R, 0)

    def residual(self, x):
        """R - K x block by block in numpy.longdouble (x: [64 (Nm + 1), 2], any float type)."""
        ld = np.longdouble
        x = np.asarray(x, ld).reshape(self.Nm + 1, KJB, 2)
        F = rows_F()
        out = np.empty_like(x)
        for i in range(self.Nm + 1):
            r = self.R[i].astype(ld) - self.D[i].astype(ld) @ x[i]
            if i < self.Nm:
                r[rows_P(i)] -= self.C[i].astype(ld) @ x[i + 1][F]
            if i > 0:
                r[F] -= self.C[i - 1].T.astype(ld) @ x[i - 1][rows_P(i - 1)]
            out[i] = r
        return out.reshape(-1, 2)


def _sym(rng, n, scale):
    a = rng.uniform(-scale, scale, (n, n))
    return 0.5 * (a + a.T)


def _spd_block(rng):
    return _sym(rng, KJB, 0.25) + np.diag(rng.uniform(6.0, 10.0, KJB))


def _kkt_vehicle(rng, i):
    """16 rows of one vehicle: a positive 9 x 9 primal block on rows {0, 8..15}, 7 multiplier rows {1..7} with a full-rank Jacobian and
    -KKT_REG on their diagonal.  (Block 0, whose pt0 rows begin at 7: the multiplier rows are {0..6} and the primal rows {7..15}, as the
    first separator's initial rows and pt0 lie -- so that in every block the pt0 rows, links and pose coupling included, are primal rows.)"""
    prim, mult = (np.arange(7, 16), np.arange(0, 7)) if i == 0 else (np.array([0] + list(range(8, 16))), np.arange(1, 8))
    B = np.zeros((16, 16))
    B[np.ix_(prim, prim)] = _sym(rng, 9, 0.5) + np.diag(rng.uniform(6.0, 10.0, 9))
    # the Jacobian: a well-conditioned 7 x 7 part (identity-dominant) beside two more columns
    J = rng.uniform(-0.5, 0.5, (7, 9))
    J[:, :7] += 2.0 * np.eye(7)[:, rng.permutation(7)]
    B[np.ix_(mult, prim)] = J
    B[np.ix_(prim, mult)] = J.T
    B[mult, mult] = -KKT_REG
    return B


def _kkt_block(rng, i, present):
    D = np.eye(KJB)
    p0 = 7 if i == 0 else 8
    for a in range(4):
        if present[a]:
            D[16 * a : 16 * a + 16, 16 * a : 16 * a + 16] = _kkt_vehicle(rng, i)
    # the pair blocks: a symmetric coupling of the present vehicles' pose rows (x, y, psi of pt0)
    pose = np.array([16 * a + p0 + c for a in range(4) if present[a] for c in range(3)])
    D[np.ix_(pose, pose)] += _sym(rng, len(pose), 0.3)
    return D


def generate(family, Nm, seed, zero_link=None):
    """A separator system of `family` with blocks 0 .. Nm.  `zero_link`: index of a link that is entirely zero (default: every third seed
    of a system with Nm >= 3 has one, in the middle)."""
    assert family in FAMILIES and Nm >= 1
    rng = np.random.default_rng([FAMILIES.index(family), Nm, seed])
    if family == "ragged":
        V = 2 + seed % 2
        N = np.array([Nm] + [int(rng.integers(1, Nm + 1)) for _ in range(V - 1)])  # unequal where Nm allows; the longest plan has Nm intervals
        if Nm >= 2 and (N == Nm).all():
            N[-1] = Nm - 1
        N = N[rng.permutation(V)]
        present = np.array([[a < V and i <= N[a] for a in range(4)] for i in range(Nm + 1)])
        linked = np.array([[a < V and i < N[a] for a in range(4)] for i in range(Nm + 1)])  # the vehicle's plan goes on beyond block i
    else:
        present = np.ones((Nm + 1, 4), bool)
        linked = np.ones((Nm + 1, 4), bool)
        linked[Nm] = False
    if zero_link is None and Nm >= 3 and seed % 3 == 1:
        zero_link = Nm // 2
    D, C, R = [], [], []
    for i in range(Nm + 1):
        D.append(_spd_block(rng) if family == "spd" else _kkt_block(rng, i, present[i]))
        c = rng.uniform(-LINK, LINK, (KJL, KJL))
        for a in range(4):
            if not linked[i, a]:  # (a vehicle's plan that goes on to block i + 1 is present there)
                c[7 * a : 7 * a + 7, :] = 0.0
                c[:, 7 * a : 7 * a + 7] = 0.0
        if i == Nm or i == zero_link:
            c[:] = 0.0
        C.append(c)
        r = rng.standard_normal((KJB, 2))
        r[np.repeat(~present[i], 16)] = 0.0
        R.append(r)
    return System(D, C, R, present, family, seed)


DENSE_MAX_BLOCKS = 18  # longer systems go to the sparse LU


def _factor(sys_):
    if sys_.Nm + 1 <= DENSE_MAX_BLOCKS:
        import scipy.linalg as sla

        lu = sla.lu_factor(sys_.dense())  # LAPACK getrf; lu_solve = getrs: together numpy.linalg.solve's gesv
        return lambda b: sla.lu_solve(lu, b)
    import scipy.sparse.linalg as spla

    lu = spla.splu(sys_.sparse())
    return lambda b: lu.solve(np.ascontiguousarray(b))


def lapack_and_reference(sys_, max_refine=8):
    """(x_lapack, x_ref, residual): the float64 LU's solution as it stands, and the same refined with longdouble residuals until the residual
    stops falling (x_ref: the last longdouble iterate rounded to float64; residual: max |R - K x| of that iterate, in longdouble)."""
    solve = _factor(sys_)
    x0 = solve(sys_.rhs())
    x = x0.astype(np.longdouble)
    best = float(np.abs(sys_.residual(x)).max())
    for _ in range(max_refine):
        xn = x + solve(np.asarray(sys_.residual(x), np.float64))
        rn = float(np.abs(sys_.residual(xn)).max())
        if not rn < best:
            break
        x, best = xn, rn
    return x0, np.asarray(x, np.float64), best


def bcr_model(sys_):
    """The cyclic reduction of cfz_jstruct.inl in numpy (float64): levels of stride 1, 2, 4, ..; the blocks st, 3 st, 5 st, .. leave at
    once, each with the columns F and P of its inverse G = D_i^-1:
        D_l[P, P] -= C_l G[F, F] C_l',  r_l[P] -= C_l (G r_i)[F];   D_r[F, F] -= C_i' G[P, P] C_i,  r_r[F] -= C_i' (G r_i)[P];
        C_l <- -C_l G[F, P] C_i  (the link of l with r)
    block 0 remains; back through the levels  x_i = G r_i - G[:, F] (C_l' x_l[P]) - G[:, P] (C_i x_r[F])."""
    Nm = sys_.Nm
    D = [d.copy() for d in sys_.D]
    C = [c.copy() for c in sys_.C]  # C[l]: the link of block l with its CURRENT right neighbour
    R = [r.copy() for r in sys_.R]
    F, P8 = rows_F(), rows_P(1)
    keep = {}
    st, top = 1, 1
    while st <= Nm:
        top = st
        for i in range(st, Nm + 1, 2 * st):
            l, r = i - st, (i + st if i + st <= Nm else None)
            Pl = rows_P(l)
            E = np.zeros((KJB, 2 * KJL))
            E[F, np.arange(KJL)] = 1.0
            E[P8, KJL + np.arange(KJL)] = 1.0
            Z = np.linalg.solve(D[i], np.concatenate([E, R[i]], 1))
            GF, GP, g = Z[:, :KJL], Z[:, KJL : 2 * KJL], Z[:, 2 * KJL :]
            Cl, Ci = C[l].copy(), C[i].copy()
            keep[i] = (GF, GP, g, Cl, Ci, l, r)
            D[l][np.ix_(Pl, Pl)] -= Cl @ (GF[F] @ Cl.T)
            R[l][Pl] -= Cl @ g[F]
            if r is not None:
                D[r][np.ix_(F, F)] -= Ci.T @ (GP[P8] @ Ci)
                R[r][F] -= Ci.T @ g[P8]
                C[l] = -Cl @ (GP[F] @ Ci)
        st *= 2
    x = [None] * (Nm + 1)
    x[0] = np.linalg.solve(D[0], R[0])
    st = top
    while st >= 1:
        for i in range(st, Nm + 1, 2 * st):
            GF, GP, g, Cl, Ci, l, r = keep[i]
            xi = g - GF @ (Cl.T @ x[l][rows_P(l)])
            if r is not None:
                xi = xi - GP @ (Ci @ x[r][F])
            x[i] = xi
        st //= 2
    return np.concatenate(x, 0)


def rel_err(x, x_ref):
    return float(np.abs(np.asarray(x) - x_ref).max() / np.abs(x_ref).max())


def yardstick(sys_):
    """dict: x_ref, residual, err_lapack, err_model, bound = 32 max(err_model, err_lapack, 2^-52) -- what a float64 cyclic reduction with
    another order of its sums may differ from the reference by."""
    x0, x_ref, res = lapack_and_reference(sys_)
    el, em = rel_err(x0, x_ref), rel_err(bcr_model(sys_), x_ref)
    return dict(x_ref=x_ref, residual=res, err_lapack=el, err_model=em, bound=32.0 * max(em, el, 2.0 ** -52))


# ---- single 64-row blocks for lu64_build -----------------------------------------------------------------------------------------------
def block_cases(n, rb, seed=0):
    """n blocks [A | B] (A 64 x 64, B 64 x rb) of the spd and the kkt kind and identity-padded ones (two or three vehicles' rows, the rest
    identity), in turn."""
    rng = np.random.default_rng([77, rb, seed])
    A, B = [], []
    for k in range(n):
        kind = k % 3
        if kind == 0:
            a = _spd_block(rng)
        else:
            present = np.ones(4, bool) if kind == 1 else np.arange(4) < 2 + (k // 3) % 2
            a = _kkt_block(rng, 1 + k % 2, present)
        A.append(a)
        B.append(rng.standard_normal((KJB, rb)))
    return np.stack(A), np.stack(B)


def block_reference(A, B, max_refine=8):
    """(x_ref, err_lapack) of one block: numpy.linalg.solve refined with longdouble residuals; LAPACK's own error against that."""
    import scipy.linalg as sla

    ld = np.longdouble
    lu = sla.lu_factor(A)
    x0 = sla.lu_solve(lu, B)
    Al, Bl = A.astype(ld), B.astype(ld)
    x = x0.astype(ld)
    best = float(np.abs(Bl - Al @ x).max())
    for _ in range(max_refine):
        xn = x + sla.lu_solve(lu, np.asarray(Bl - Al @ x, np.float64))
        rn = float(np.abs(Bl - Al @ xn).max())
        if not rn < best:
            break
        x, best = xn, rn
    x_ref = np.asarray(x, np.float64)
    return x_ref, rel_err(x0, x_ref)


def serial_solve(A, B, last_of_equals=False):
    """cfz_struct.inl block_solve_serial in numpy: partial pivoting, the FIRST of equal candidates wins (`last_of_equals`: the other choice,
    to show what it would cost).  None = singular."""
    n = len(A)
    M = np.concatenate([A, B], 1).astype(float)
    for k in range(n):
        col = np.abs(M[k:, k])
        best = col.max()
        if not best > 0.0:
            return None
        cand = np.flatnonzero(col == best)
        p = k + (cand[-1] if last_of_equals else cand[0])
        if p != k:
            M[[k, p]] = M[[p, k]]
        l = M[k + 1 :, k] / M[k, k]
        M[k + 1 :, k + 1 :] -= np.outer(l, M[k, k + 1 :])
    x = np.zeros((n, B.shape[1]))
    for k in range(n - 1, -1, -1):
        x[k] = (M[k, n:] - M[k, k + 1 : n] @ x[k + 1 :]) / M[k, k]
    return x


def tie_block(rb, seed=0, big=1e7):
    """A block whose first column has its two largest entries equal in magnitude, in row 5 (+2) and row 40 (-2).  Row 5 is an ordinary row;
    row 40 is `big` times larger beyond the first column.  With row 5 as the first pivot (the first of equals: block_solve_serial, LAPACK)
    only row 40 takes a multiple of it; with row 40 every row takes a multiple of ITS entries and loses log10(big) digits."""
    rng = np.random.default_rng([78, rb, seed])
    A = _spd_block(rng)
    A[:, 0] = rng.uniform(-1.0, 1.0, KJB)
    A[5, 0], A[40, 0] = 2.0, -2.0
    A[40, 1:] = big * rng.uniform(0.5, 1.0, KJB - 1) * rng.choice([-1.0, 1.0], KJB - 1)
    return A, rng.standard_normal((KJB, rb))
