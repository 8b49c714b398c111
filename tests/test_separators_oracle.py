"""oracle/separators.py by itself (no GPU): the generator of joint separator systems in the kernel's layout, the extended-precision reference
and the two float64 solves that make the yardstick of tests/test_jstruct_blocks_gpu.py.

Bounds and where they come from.  `CAP` = 3e-11 is the generator's own condition: a system whose float64 solves (LAPACK, the numpy cyclic
reduction) are further than that from the reference is too badly conditioned to tell a bug from rounding, and 32 x CAP stays below the 1e-9
the GPU test allows any bound.  The reference must be a reference: its residual, formed in longdouble, lies below one float64 rounding of the
largest term of a row (the refinement's fixed point is at longdouble level, 2^-64, times the condition)."""
import functools

import numpy as np
import pytest

from oracle import separators as sep

NMS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 31, 50, 51)
CAP = 3e-11


@functools.lru_cache(maxsize=None)
def _case(family, Nm, seed):
    s = sep.generate(family, Nm, seed)
    return s, sep.yardstick(s)


@pytest.mark.parametrize("family", sep.FAMILIES)
def test_cyclic_reduction_model_and_lapack_against_the_refined_reference(family):
    worst = dict(model=0.0, lapack=0.0, ratio=0.0)
    for Nm in NMS:
        for seed in (0, 1):
            s, y = _case(family, Nm, seed)
            K, x = s.dense(), y["x_ref"]
            # the reference solves the system: residual below a float64 rounding of a row's largest term
            assert y["residual"] <= 2.0 ** -53 * (np.abs(K) @ np.abs(x)).max(), (family, Nm, seed, y["residual"])
            assert y["err_model"] <= CAP and y["err_lapack"] <= CAP, (family, Nm, seed, y["err_model"], y["err_lapack"])
            assert y["bound"] == 32.0 * max(y["err_model"], y["err_lapack"], 2.0 ** -52) <= 1e-9
            worst["model"], worst["lapack"] = max(worst["model"], y["err_model"]), max(worst["lapack"], y["err_lapack"])
            worst["ratio"] = max(worst["ratio"], y["err_model"] / max(y["err_lapack"], 2.0 ** -53))
    print(f"{family}: numpy cyclic reduction at most {worst['model']:.1e}, LAPACK at most {worst['lapack']:.1e}, model / LAPACK at most {worst['ratio']:.1f}")


def test_long_system_through_the_sparse_factorisation():
    """Nm = 255 (the product's limit; 16384 unknowns): the sparse LU with longdouble refinement, and the model, as for the short ones."""
    s = sep.generate("kkt", 255, 0)
    y = sep.yardstick(s)
    assert s.Nm + 1 > sep.DENSE_MAX_BLOCKS and y["err_model"] <= CAP and y["err_lapack"] <= CAP
    assert y["residual"] <= 2.0 ** -53 * (abs(s.sparse()) @ np.abs(y["x_ref"])).max()
    # the sparse and the dense path are the same reference: a system both can take
    s2 = sep.generate("kkt", 17, 0)
    _, xd, _ = sep.lapack_and_reference(s2)
    old, sep.DENSE_MAX_BLOCKS = sep.DENSE_MAX_BLOCKS, 4
    try:
        _, xs, _ = sep.lapack_and_reference(s2)
    finally:
        sep.DENSE_MAX_BLOCKS = old
    assert sep.rel_err(xs, xd) <= 2.0 ** -51  # (both rounded from longdouble iterates at their fixed points)


@pytest.mark.parametrize("family", sep.FAMILIES)
def test_a_wrong_link_entry_is_far_above_the_yardstick(family):
    """What the GPU test's bound can see: one entry of one link set to zero moves the solution by more than a thousand bounds."""
    s, y = _case(family, 5, 0)
    C = [c.copy() for c in s.C]
    p, f = np.argwhere(np.abs(C[2]) > 0.25)[0]
    C[2][p, f] = 0.0
    wrong = sep.bcr_model(sep.System(s.D, C, s.R, s.present, s.family, s.seed))
    assert sep.rel_err(wrong, y["x_ref"]) > 1000.0 * y["bound"]


@pytest.mark.parametrize("family", sep.FAMILIES)
@pytest.mark.parametrize("Nm", (1, 4, 7))
def test_layout_of_the_generated_systems(family, Nm):
    s = sep.generate(family, Nm, 1)
    K = s.dense()
    n, F = sep.KJB, sep.rows_F()
    assert np.array_equal(K, K.T)
    assert np.array_equal(K, s.sparse().toarray())
    Ds, Us = s.kernel_arrays(spare=np.nan)
    Us = Us.reshape(Nm + 1, sep.KJU, n)
    for i in range(Nm + 1):
        for j in range(Nm + 1):
            blk = K[n * i : n * i + n, n * j : n * j + n]
            if abs(i - j) > 1:
                assert not blk.any()
            elif j == i + 1:  # links only in P x F ...
                P = sep.rows_P(i)
                mask = np.zeros((n, n), bool)
                mask[np.ix_(P, F)] = True
                assert not blk[~mask].any()
                # ... stored as Us[i][f * 64 + P[p]], zero in every other row of the 28 columns
                assert np.array_equal(Us[i][:28][:, P], blk[np.ix_(P, F)].T)
                assert not np.delete(Us[i][:28], P, axis=1).any()
                assert (np.abs(blk[np.ix_(P, F)]) <= sep.LINK).all()
        assert np.array_equal(Ds[i].reshape(n, n).T, K[n * i : n * i + n, n * i : n * i + n])  # column-major
        assert np.array_equal(Us[i][28:30].T, s.R[i]) and np.isnan(Us[i][30:]).all()
    assert not Us[Nm][:28].any()
    assert sorted(set(sep.rows_P(0)) - set(sep.rows_P(1))) == [7, 23, 39, 55] and len(set(F) & set(sep.rows_P(1))) == 0


def test_some_links_are_entirely_zero_and_most_are_not():
    zero = [not sep.generate(f, Nm, seed).C[Nm // 2].any() for f in sep.FAMILIES for Nm in (5, 16) for seed in (0, 1)]
    assert any(zero) and not all(zero)
    s = sep.generate("spd", 8, 0, zero_link=3)
    assert not s.C[3].any() and all(s.C[i].any() for i in range(8) if i != 3)


@pytest.mark.parametrize("seed", (0, 1))
def test_identity_rows_of_the_ragged_family(seed):
    """V = 2 or 3 vehicles with plans of unequal length: absent vehicles' rows, and a vehicle's rows beyond the end of its plan, are identity
    rows with zero right-hand sides and no links -- the padding jstruct_sep_base writes."""
    Nm = 9
    s = sep.generate("ragged", Nm, seed)
    last = [int(np.flatnonzero(s.present[:, a]).max()) if s.present[:, a].any() else -1 for a in range(4)]
    V = sum(l >= 0 for l in last)
    assert V == 2 + seed % 2 and max(last) == Nm and len({l for l in last if l >= 0}) > 1
    K, x = s.dense(), sep.yardstick(s)["x_ref"]
    n = sep.KJB
    for i in range(Nm + 1):
        for a in range(4):
            rows = n * i + 16 * a + np.arange(16)
            if s.present[i, a]:
                assert i <= last[a] and np.abs(K[rows][:, rows]).sum() > 16.0
                continue
            assert np.array_equal(K[rows], np.eye(K.shape[0])[rows]) and np.array_equal(K[:, rows], np.eye(K.shape[0])[:, rows])
            assert not s.R[i][16 * a : 16 * a + 16].any() and not x[rows].any()
    # a vehicle in its last block is linked to the left and not to the right
    for a in range(4):
        if 0 <= last[a] < Nm:
            i = last[a]
            assert not s.C[i][7 * a : 7 * a + 7].any() and (i == 0 or s.C[i - 1][:, 7 * a : 7 * a + 7].any() or not s.C[i - 1].any())


def test_the_harness_runs_the_products_level_loop():
    """tests/hip/jstruct_blocks.hip carries a copy of jstruct_solve's phase 3 (moving the loop into a function changed the product's register
    allocation): statement for statement the product's, but for the names of the LDS window and of the early return."""
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prod = open(os.path.join(root, "conflict_rez_amd", "csrc", "cfz_jstruct.inl")).read()
    harn = open(os.path.join(root, "tests", "hip", "jstruct_blocks.hip")).read()
    a = prod.index("  {  // block cyclic reduction (round 6)")
    mine = prod[a : prod.index("#else", a)]
    b = harn.index("// ---- the copy of jstruct_solve's phase 3 begins ----")
    copy = harn[b : harn.index("// ---- the copy ends ----")]

    def statements(text):
        lines = [re.sub(r"//.*$", "", l).strip() for l in text.splitlines()]
        return [l.replace("return 1;", "return;").replace("(cfzb::lds_f64 *)wlds)", "(cfzb::lds_f64 *)lds)") for l in lines if l]

    assert statements(mine) == statements(copy) and len(statements(mine)) > 20
