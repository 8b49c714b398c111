"""The Newton step's backward sweeps and scans as the CPU build of the product source runs them (tests/emu/cfz_emu.cpp, cfz_plan_emu.cpp), ALONE,
against the references of oracle/sweeps.py: the textbook Riccati recursion in longdouble and the dense KKT system solved by LAPACK and refined.
tests/test_sweeps_gpu.py holds the device functions to the same systems, with these CPU results as one half of every bound.

Also here: the conditions on the generator (no yardstick above 3e-11, no bound above 1e-9), the two routes to the step agreeing with each
other far below any bound, and the demonstration that the `long` family sees a sweep that takes its accumulator transposed without
symmetrising it."""
import functools
import os

import numpy as np
import pytest

import sweeps_binding as sb
from oracle import sweeps as sw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MPC_NS = (2, 3, 4, 5, 6, 7, 16, 30, 31, 32)
LAYOUTS = ((9, 3), (4, 0))
PLAN_TS = (1, 2, 3, 30, 299, 300, 434, 510)  # 434: the longest plan cfz_state_ws keeps in LDS on gfx950 (tests/test_sweeps_gpu.py)
SEEDS = (0, 1)


@functools.lru_cache(maxsize=None)
def mpc_case(family, N, seed):
    """A system with its reference and yardstick: computed once, shared by the tests of both modules, never changed."""
    s = sw.generate_mpc(family, N, seed)
    return s, sw.yardstick(s, sb.cpu_mpc)


@functools.lru_cache(maxsize=None)
def plan_case(family, T, seed, has_final):
    s = sw.generate_plan(family, T, seed, has_final)
    return s, sw.yardstick(s, sb.cpu_plan)


def plan_cases(family):
    return [plan_case(family, T, seed, hf) for T in ((sw.LONG_T,) if family == "long" else PLAN_TS) for seed in SEEDS for hf in (0, 1)]


def caps_hold(y):
    return all(y["yard"][g] <= sw.YARD_CAP and y["bound"][g] == 32.0 * y["yard"][g] <= sw.BOUND_CAP for g in y["yard"])


def test_tables_agree_with_their_sources():
    """The prototype tables of the two CPU builds against the `extern "C"` definitions of their sources (tests/c_decls.py)."""
    import c_decls

    for source, table in ((sb.SOURCE, sb.PROTOTYPES), (sb.PLAN_SOURCE, sb.PLAN_PROTOTYPES)):
        decls = c_decls.declarations(open(os.path.join(ROOT, source)).read())
        assert len(decls) == len(table) and not c_decls.mismatches(table, decls, sb.STRUCTS), (source, c_decls.mismatches(table, decls, sb.STRUCTS))


def test_layout_aliases_the_value_function_as_the_issue_of_the_scans_assumes():
    """What the scan tests rest on: rP stands in the step's slots from N = 6 and in the cos / sin slots below, dpi on d."""
    for nb, nn in LAYOUTS:
        for N in MPC_NS:
            L = sb.layout(N, nb, nn)
            assert L["rP"] == (L["dp"] + 7 if N >= 6 else L["cs"]) and L["dpi"] == L["d"]
            assert L["rP"] + 30 <= (L["dp"] + 7 * N if N >= 6 else L["cs"] + 32)


@pytest.mark.parametrize("family", sw.MPC_FAMILIES)
def test_mpc_cpu_build_against_the_references(family):
    """riccati_backward_dense, forward_scan and costate_scan of the CPU build on one workspace (the composite): gains, value function, dp, dpi0
    and dpi within the system's bound, in both layouts with the same bits; the generator's caps; the recursion's step and the KKT
    solution within 64 x 2^-52 of each other."""
    worst = {g: 0.0 for g in sw.MPC_GROUPS}
    for N in MPC_NS:
        for seed in SEEDS:
            s, y = mpc_case(family, N, seed)
            assert caps_hold(y), (N, seed, y["yard"])
            assert y["ref"]["kkt_gap"] <= 64.0 * sw.EPS, (N, seed, y["ref"]["kkt_gap"])
            for g in sw.MPC_GROUPS:
                assert max(y["err_cpu"][g], y["err_model"][g]) <= y["bound"][g]
                worst[g] = max(worst[g], y["yard"][g])
            a, b = sb.cpu_mpc(s, *LAYOUTS[0], fill=np.nan), sb.cpu_mpc(s, *LAYOUTS[1])
            for g in sw.MPC_GROUPS:  # NaN in every word that is no input, the other layout: the same bits as the yardstick's run
                assert np.isfinite(a[g]).all() and np.array_equal(a[g], b[g]) and sw.rel_err(a[g], y["ref"][g]) == y["err_cpu"][g], (N, seed, g)
    print(f"{family}: largest yardstick per group " + " ".join(f"{g} {v:.1e}" for g, v in worst.items()))


@pytest.mark.parametrize("family", sw.MPC_FAMILIES)
def test_scans_of_the_cpu_build_from_reference_gains(family):
    """forward_scan and costate_scan alone, from the reference's gains and value function rounded to float64: the KKT solution within the bound."""
    for N in MPC_NS:
        s, y = mpc_case(family, N, 0)
        out = sb.cpu_mpc(s, *LAYOUTS[0], fill=np.nan, gains=(y["ref"]["kk"], y["ref"]["vf"]))
        for g in ("dp", "dpi0", "dpi"):
            assert sw.rel_err(out[g], y["ref"][g]) <= y["bound"][g], (N, g)


@pytest.mark.parametrize("family", sw.PLAN_FAMILIES)
def test_state_ws_cpu_builds_against_the_recursion(family):
    """cfzp::riccati_backward_dense as the matrix-core sweep runs it (-DCFZP_DENSE_SWEEP -DCFZP_DENSE_TRANSPOSED), the same loops untransposed
    and the default one-lane riccati_backward (a cell end at every stage: PSpec.N = 1) within the bound of the longdouble recursion;
    flag 0; NaN in fb and vf beforehand changes no bit."""
    for s, y in plan_cases(family):
        assert caps_hold(y), (s.T, s.seed, y["yard"])
        outs = dict(transposed=sb.cpu_plan(s, fill=np.nan), plain=sb.cpu_plan(s, dense_transposed=False), one_lane=sb.cpu_plan(s, one_lane=True, fill=np.nan))
        for name, o in outs.items():
            assert o["flag"] == 0
            for g in sw.PLAN_GROUPS:
                assert sw.rel_err(o[g], y["ref"][g]) <= y["bound"][g], (name, s.T, s.seed, s.has_final, g)
        for g in sw.PLAN_GROUPS:
            assert sw.rel_err(outs["transposed"][g], y["ref"][g]) == y["err_cpu"][g]


def test_the_long_family_sees_a_missing_symmetrisation():
    """The homogeneous recursion with the accumulator taken as it stands: symmetrised per stage it is a yardstick; unsymmetrised it is beyond
    1000 x the bound at T = 300 (the antisymmetric part of the rounding, undamped), while the untransposed recursion needs no symmetrisation."""
    for s, y in plan_cases("long"):
        bad, plain = sw.plan_homogeneous(s, transposed=True, symmetrise=False), sw.plan_homogeneous(s, transposed=False, symmetrise=False)
        for g in sw.PLAN_GROUPS:
            assert sw.rel_err(bad[g], y["ref"][g]) > 1000.0 * y["bound"][g]
            assert sw.rel_err(plain[g], y["ref"][g]) <= y["bound"][g]


def test_singular_stage_is_a_status():
    """M_ee exactly zero at stage T - 1: every build and the models return flag 1."""
    s = sw.singular_plan(30, 0)
    assert sw.plan_recursion(s)["flag"] == 1 and sw.plan_homogeneous(s)["flag"] == 1
    assert sb.cpu_plan(s)["flag"] == 1 and sb.cpu_plan(s, one_lane=True)["flag"] == 1
