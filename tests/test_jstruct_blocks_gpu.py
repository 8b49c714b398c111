"""The joint plan's separator recursion (cfz_jstruct.inl jbcr_lu_all / jbcr_update_all / jbcr_back_all / jbcr_triple) and the 64-row eliminations
on the matrix cores under it (cfz_struct.inl lu64_build), run ALONE on an MI355X by tests/hip/jstruct_blocks.hip -- a stand-alone program over
the product's own sources -- on systems chosen in oracle/separators.py, against solutions refined with longdouble residuals.

This code exists in the device pass only (the CPU build runs a serial chain), and the end-to-end tests forgive a slightly wrong Newton step: the
interior-point iteration still converges.  Here a wrong entry of a link, a skipped update or an operand read beyond 28 moves a solution by 1e-3
and more, against bounds of 1e-14 .. 1e-13.

The bound of a system: 32 x max(error of the numpy cyclic reduction, error of LAPACK, 2^-52) on THAT system (oracle/separators.py `yardstick`):
another order of the sums and another pivot among equals are as valid as the model's; no bound may exceed 1e-9 and no yardstick 3e-11.

Measured on an MI355X (error = max |x - x_ref| / max |x_ref| over both right-hand sides; ratio = error / max(model, LAPACK, 2^-52)):
  recursion, spd:     largest kernel error 1.69e-15, largest ratio 3.00   (model at most 6.5e-16, LAPACK at most 7.6e-16)
  recursion, kkt:     largest kernel error 5.79e-15, largest ratio 1.83   (model at most 6.2e-15, LAPACK at most 3.2e-15)
  recursion, ragged:  largest kernel error 4.23e-15, largest ratio 2.60   (model at most 3.0e-15, LAPACK at most 1.6e-15)
  lu64_build<16>:     largest error 2.06e-15, largest ratio to LAPACK's 4.00; the tie block 1.05e-15 (the other pivot: 1.7e-9)
  lu64_build<32>:     largest error 2.03e-15, largest ratio to LAPACK's 4.00; the tie block 1.53e-15 (the other pivot: 4.6e-10)
  jbcr_triple:        largest entrywise error 9.29 x 2^-53 (|A| |G| |B|), against the bound's 60
The recursion's bounds were between 1.0e-14 and 2.0e-13.  One, two and eight wavefronts and NaN-filled workspaces: the same bits.  What the first run
found: the copy of block 0's solution to xs took two wavefronts (`if (wv < 2)`), so a workgroup of one left the second right-hand side of block 0
unwritten; the product launches eight, and the loop now strides over the wavefronts there are.
"""
import functools

import numpy as np
import pytest

from emu_build import build_hip_program, run_program
from oracle import separators as sep

pytestmark = pytest.mark.gpu

NMS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 31, 50, 51, 255)  # every level count from one to eight, a last block with and without a right neighbour, the product's limit
SEEDS = (0, 1)
BOUND_CAP, YARD_CAP = 1e-9, 3e-11
N_BLOCKS = 256


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """tests/hip/jstruct_blocks.hip built once for gfx950; `run(header, *arrays)` = one invocation, its output as float64."""
    d = tmp_path_factory.mktemp("jstruct_blocks")
    exe = build_hip_program("tests/hip/jstruct_blocks.hip", d / "jstruct_blocks")
    count = [0]

    def run(header, *arrays):
        count[0] += 1
        fin, fout = str(d / f"in{count[0]}.bin"), str(d / f"out{count[0]}.bin")
        with open(fin, "wb") as f:
            f.write(np.array(list(header) + [0] * (8 - len(header)), np.int64).tobytes())
            for a in arrays:
                f.write(np.ascontiguousarray(a).tobytes())
        run_program(exe, [fin, fout])
        return np.fromfile(fout, np.float64)

    return run


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


@functools.lru_cache(maxsize=None)
def _case(family, Nm, seed):
    """A system with its reference and yardstick: computed once, shared by the tests, never changed."""
    s = sep.generate(family, Nm, seed)
    y = sep.yardstick(s)
    y["x_ref"].setflags(write=False)
    return s, y


def _recursion(run, systems, threads=512, fill=0):
    """One invocation of the `recursion` kernel on `systems`: list over runs of (xs per system as [64 (Nm + 1), 2], flags)."""
    arrs = [s.kernel_arrays() for s in systems]
    nblk = sum(s.Nm + 1 for s in systems)
    out = run([3, len(systems), threads, fill], np.array([s.Nm for s in systems], np.int64), np.concatenate([a[0].ravel() for a in arrs]),
              np.concatenate([a[1].ravel() for a in arrs]))
    per = nblk * 128 + len(systems)
    assert out.size % per == 0
    runs = []
    for r in range(out.size // per):
        o = out[r * per : (r + 1) * per]
        xs, at = [], 0
        for s in systems:
            x = o[at * 128 : (at + s.Nm + 1) * 128].reshape(s.Nm + 1, 2, 64)  # xs[i][rhs][row]
            xs.append(np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(-1, 2))
            at += s.Nm + 1
        runs.append((xs, o[nblk * 128 :]))
    return runs


@pytest.mark.parametrize("family", sep.FAMILIES)
def test_recursion_against_the_refined_reference(harness, family):
    """Phase 3 on 32 systems of a family (sixteen lengths, two seeds), eight wavefronts: no fail flag, and every solution within the bound of
    its own system."""
    cases = [_case(family, Nm, seed) for Nm in NMS for seed in SEEDS]
    (xs, flags), = _recursion(harness, [c[0] for c in cases])
    worst_err = worst_ratio = 0.0
    bad = []
    for (s, y), x, fl in zip(cases, xs, flags):
        yard = max(y["err_model"], y["err_lapack"], 2.0 ** -52)
        err = sep.rel_err(x, y["x_ref"]) if np.isfinite(x).all() else np.inf
        print(f"{family} Nm {s.Nm} seed {s.seed}: flag {fl:g} kernel {err:.2e} model {y['err_model']:.2e} LAPACK {y['err_lapack']:.2e} bound {y['bound']:.2e} ratio {err / yard:.2f}")
        worst_err, worst_ratio = max(worst_err, err), max(worst_ratio, err / yard)
        assert yard <= YARD_CAP and y["bound"] == 32.0 * yard <= BOUND_CAP  # a condition on the generator, not a measurement
        if fl != 0.0 or not err <= y["bound"]:
            bad.append((s.Nm, s.seed, fl, err, y["bound"]))
    print(f"{family}: largest kernel error {worst_err:.2e}, largest ratio to the yardstick {worst_ratio:.2f}")
    assert not bad, bad


def test_recursion_is_independent_of_the_workgroup_shape(harness):
    """One, two and eight wavefronts split the tasks of a level differently and compute the same bits: a missing barrier, or arithmetic that
    depends on the split, shows here."""
    cases = [_case(f, Nm, 0) for f in sep.FAMILIES for Nm in (5, 16, 51)]
    runs = _recursion(harness, [c[0] for c in cases], threads=0)
    assert len(runs) == 3
    for xs, flags in runs:
        assert not flags.any()
        for (s, y), x, x8 in zip(cases, xs, runs[2][0]):
            assert sep.rel_err(x, y["x_ref"]) <= y["bound"], (s.family, s.Nm)
            assert _same_bits(x, x8), (s.family, s.Nm)


def test_recursion_reads_nothing_it_has_not_written(harness):
    """Zs, Zb, Lc, xs and the spare columns 30, 31 of every Us block full of NaN before the launch: the same bits as from zeros."""
    cases = [_case(f, Nm, 1) for f in sep.FAMILIES for Nm in (1, 2, 5, 16, 51)]
    (x0, f0), (xn, fn) = _recursion(harness, [c[0] for c in cases], fill=2)
    assert not f0.any() and not fn.any()
    for (s, y), a, b in zip(cases, x0, xn):
        assert np.isfinite(b).all(), (s.family, s.Nm, np.argwhere(~np.isfinite(b))[:8])
        assert _same_bits(a, b), (s.family, s.Nm)
        assert sep.rel_err(a, y["x_ref"]) <= y["bound"]


def test_recursion_flags_a_singular_block_and_solves_the_system_beside_it(harness):
    """Block 3 with a zero row and column: the flag of that system is 1, a status; the system in the next workgroup is solved."""
    s, y = _case("spd", 5, 0)
    D = [d.copy() for d in s.D]
    D[3][20, :] = 0.0
    D[3][:, 20] = 0.0
    broken = sep.System(D, s.C, s.R, s.present, s.family, s.seed)
    (xs, flags), = _recursion(harness, [broken, s])
    assert flags.tolist() == [1.0, 0.0] and sep.rel_err(xs[1], y["x_ref"]) <= y["bound"]


def _triple_sets():
    rng = np.random.default_rng(5)
    sets = []
    for k in range(5):
        A, G, B = (np.full((32, 32), np.nan) for _ in range(3))
        vec = np.full((32, 2), np.nan)
        for M in (A, G, B):
            M[:28, :28] = rng.uniform(-1.0, 1.0, (28, 28)) * 10.0 ** rng.integers(-3, 4, (28, 28))  # entries of mixed size: an entrywise bound has to hold
        vec[:28] = rng.standard_normal((28, 2))
        if k == 4:  # one row of A and one column of B exactly zero
            A[5, :28] = 0.0
            B[:28, 9] = 0.0
        sets.append((A, G, B, vec))
    return sets


def test_triple_product_on_the_matrix_cores(harness):
    """jbcr_triple: X = A (G B) of 28 x 28 operands and the two `vec` columns against the product in longdouble, entrywise within
    60 x 2^-53 x (|A| |G| |B|)[i][j] (two chained products of inner length 28: (28 + 28 + a few) roundings of relative size 2^-53); storage beyond
    index 27 holds NaN and is masked by the element functions; every entry of the 32 x 32 output is reported exactly once, zero where an
    index is beyond 27; exact zeros in, exact zeros out."""
    sets = _triple_sets()
    out = harness([2, len(sets)], np.concatenate([np.concatenate([m.ravel() for m in s_]) for s_ in sets]))
    n = len(sets)
    X, cnt = out[: n * 2048].reshape(n, 2, 32, 32), out[n * 2048 :].reshape(n, 2, 32, 32)
    assert np.array_equal(cnt, np.ones_like(cnt)), np.argwhere(cnt != 1.0)[:8]
    ld = np.longdouble
    worst = 0.0
    for k, (A, G, B, vec) in enumerate(sets):
        a, g, b, v = A[:28, :28], G[:28, :28], B[:28, :28], vec[:28]
        want = np.zeros((2, 32, 32), ld)
        scale = np.zeros((2, 32, 32))
        want[:, :28, :28] = a.astype(ld) @ (g.astype(ld) @ b.astype(ld))
        scale[:, :28, :28] = np.abs(a) @ (np.abs(g) @ np.abs(b))
        want[0, :28, 28:30] = a.astype(ld) @ v.astype(ld)
        scale[0, :28, 28:30] = np.abs(a) @ np.abs(v)
        err = np.abs(X[k].astype(ld) - want).astype(float)
        assert np.isfinite(X[k]).all() and (err <= 60.0 * 2.0 ** -53 * scale).all(), (k, np.argwhere(~(err <= 60.0 * 2.0 ** -53 * scale))[:8])
        worst = max(worst, float((err[scale > 0] / scale[scale > 0]).max() / 2.0 ** -53))
        assert not X[k][:, 28:, :].any() and not X[k][0, :, 30:].any() and not X[k][1, :, 28:].any()
    print(f"jbcr_triple: largest entrywise error {worst:.2f} x 2^-53 (|A| |G| |B|)")
    assert not X[4][:, 5, :].any() and not X[4][:, :, 9].any()
    assert X[4][0, :28, 28:30].any() and X[3][:, 5, :28].all() and X[3][:, :28, 9].all()


@functools.lru_cache(maxsize=None)
def _block_refs(rb):
    A, B = sep.block_cases(N_BLOCKS, rb)
    refs = [sep.block_reference(A[k], B[k]) for k in range(N_BLOCKS)]
    return A, B, refs


@pytest.mark.parametrize("rb", (16, 32))
def test_block_elimination_of_the_product_source(harness, rb):
    """lu64_build<16> / <32> as the product compiles them: 256 blocks (spd, kkt, identity-padded) against the refined reference within
    32 x max(LAPACK's error on that block, 2^-52); a column with two candidates of equal magnitude, where the first must win (the other
    choice costs five digits: oracle/separators.py tie_block); a block with a zero row and a block with a NaN return flag 1, and the
    blocks after them are solved."""
    A, B, refs = _block_refs(rb)
    At, Bt = sep.tie_block(rb)
    xt, elt = sep.block_reference(At, Bt)
    # the construction does what it says, on the CPU: first of equals = as good as LAPACK, last of equals = orders above the bound
    bound_t = 32.0 * max(elt, 2.0 ** -52)
    assert sep.rel_err(sep.serial_solve(At, Bt), xt) <= bound_t and sep.rel_err(sep.serial_solve(At, Bt, last_of_equals=True), xt) > 1000.0 * bound_t
    Az = A[0].copy()
    Az[17, :] = 0.0
    An = A[1].copy()
    An[10, 3] = np.nan
    assert sep.serial_solve(Az, B[0]) is None
    allA = np.concatenate([A, [At, Az, An, A[2]]])
    allB = np.concatenate([B, [Bt, B[0], B[1], B[2]]])
    n = len(allA)
    blocks = np.concatenate([allA, allB], 2).transpose(0, 2, 1)  # [A | B] column-major
    out = harness([1, n, rb], blocks)
    X, flags = out[: n * 64 * rb].reshape(n, rb, 64).transpose(0, 2, 1), out[n * 64 * rb :]
    assert flags.tolist() == [0.0] * N_BLOCKS + [0.0, 1.0, 1.0, 0.0]
    worst_err = worst_ratio = 0.0
    bad = []
    for k in list(range(N_BLOCKS)) + [N_BLOCKS, N_BLOCKS + 3]:
        x_ref, el = (xt, elt) if k == N_BLOCKS else refs[k if k < N_BLOCKS else 2]
        yard = max(el, 2.0 ** -52)
        err = sep.rel_err(X[k], x_ref) if np.isfinite(X[k]).all() else np.inf
        assert 32.0 * yard <= BOUND_CAP
        worst_err, worst_ratio = max(worst_err, err), max(worst_ratio, err / yard)
        if not err <= 32.0 * yard:
            bad.append((k, err, 32.0 * yard))
    print(f"lu64_build<{rb}>: largest error {worst_err:.2e}, largest ratio to LAPACK's {worst_ratio:.2f}; tie block {sep.rel_err(X[N_BLOCKS], xt):.2e} (LAPACK {elt:.2e})")
    assert not bad, bad
    assert _same_bits(X[N_BLOCKS + 3], X[2])  # the same block after the two that failed
