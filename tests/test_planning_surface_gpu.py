"""`engine.state_ws`, `colloc` and `joint_colloc_batch` on the synthetic four-vehicle strategy (strategy lengths 11, 7, 7, 9) against
what the build before the restatement of their host code returned (tests/golden/planning_surface_parent.npz, recorded on the GPU by
tests/golden/make_planning_surface.py, whose `run_cases` this module runs): status and iteration count equal, trajectories, dt and
cost equal BIT FOR BIT -- the kernels are the same instructions, the host hands them the same bytes, and tests/test_determinism_gpu.py
holds these kernels to repeatable bits.  Every recorded plan converged (asserted first, so that equal garbage cannot pass)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conflict_rez_amd import engine, scenarios

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_planning_surface as surface  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lot():
    return surface.lot()


@pytest.fixture(scope="module")
def recorded():
    d = np.load(os.path.join(HERE, "golden", "planning_surface_parent.npz"))
    for k in surface.STORED:
        assert (d[f"{k}_status"] == 0).all(), k
    return d


@pytest.fixture(scope="module")
def results(lot):
    return surface.run_cases(engine, lot)


def _same(results, recorded, case):
    got = surface.flatten(results)
    assert got["status"].tolist() == recorded[f"{case}_status"].tolist() and got["iters"].tolist() == recorded[f"{case}_iters"].tolist(), case
    for f in ("traj", "cost") + (("dt",) if "dt" in got else ()):
        assert got[f].shape == recorded[f"{case}_{f}"].shape and np.array_equal(got[f], recorded[f"{case}_{f}"]), (case, f)


@pytest.mark.parametrize("case", surface.STORED)
def test_plans_equal_the_parent_builds_bit_for_bit(results, recorded, case):
    _same(results[case], recorded, case)


def test_explicit_pairs_equal_the_default_pairs(results, recorded):
    """Two vehicles: pairs = [(0, 1)] is the default list."""
    a, b = surface.flatten(results["joint2"]), surface.flatten(results["joint2_pairs"])
    assert all(np.array_equal(a[f], b[f]) for f in a)
    _same(results["joint2_pairs"], recorded, "joint2")


def test_workspace_entry_points_equal_the_fixture(lot, recorded):
    """`cfz_state_ws_w`, `cfz_colloc_w` on an explicit workspace."""
    ws = engine.PlanWorkspace()
    res = surface.run_cases(engine, lot, ws=ws)
    ws.close()
    for case in ("state_ws", "colloc"):
        _same(res[case], recorded, case)


def test_refused_calls_keep_their_text_and_leave_the_workspace_usable(lot, recorded):
    ws = engine.PlanWorkspace()
    sp = scenarios.parking_lot_spec(n_nbr=0, N=2)
    tubes, init, fh = lot["tubes"], [p[0] for p in lot["paths"]], lot["fh"]
    guess = lambda a, nps=5: np.zeros((nps * len(tubes[a]) * 6, 7))

    def joint(vs, **kw):
        sc = dict(init_poses=[init[a] for a in vs], tubes=[tubes[a] for a in vs], guesses=[guess(a) for a in vs], dt0=0.5, final_headings=[fh[a] for a in vs])
        return engine.joint_colloc_batch(sp, [sc], ws=ws, **kw)

    def one_cell_plan():  # n_sets = 1 has no tube to pack: straight through the C ABI
        po = engine._options(engine._CPlanOptions, "cfz_default_plan_options", "plan", {})
        n_sets, pose, cell, traj = np.ones(1, np.int32), np.zeros(3), np.zeros(24), np.zeros((1, 7))
        engine._ck(ws.lib.cfz_state_ws_w(ws._w, 1, C.byref(po), engine._ptr(n_sets), engine._ptr(pose), None, engine._ptr(cell), None,
                                         engine._ptr(traj), None, None, None), "cfz_state_ws")

    refused = [
        (one_cell_plan, "a plan needs at least two strategy steps"),
        (lambda: engine.state_ws(init[:1], tubes[:1], ws=ws, kernel=3), r"cfz_plan_options\.kernel: 0 \(by batch size\), 1 \(wide\) or 2 \(narrow\)"),
        (lambda: engine.colloc(sp, init[:1], tubes[:1], [guess(0)], [0.5], fh[:1], ws=ws, kernel=1), "retired"),
        (lambda: engine.colloc(sp, init[:1], tubes[:1], [guess(0)], [0.5], fh[:1], ws=ws, structured=2), r"cfz_colloc_options\.structured must be 0 \(band\) or 1"),
        (lambda: engine.colloc(sp, init[:1], tubes[:1], [guess(0, 0)], [0.5], fh[:1], ws=ws, N_per_set=0), "problem size outside compiled limits"),
        (lambda: joint((2, 3), pairs=[(1, 0)]), "bad vehicle pair"),
        (lambda: joint((2,), pairs=[(0, 0)]), "vehicle pairs need at least two vehicles"),
        (lambda: joint((0, 1, 2, 3, 1)), "problem size outside compiled limits"),
    ]
    for call, text in refused:
        with pytest.raises(RuntimeError, match=text):
            call()
    _same(surface.state_ws_case(engine, lot, ws)[0], recorded, "state_ws")
    ws.close()
