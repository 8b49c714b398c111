"""The hand-off between the items of the persistent closed loop (`cfz_loop_run`, cfz_loop_body.inl): what an item leaves for other
workgroups of the same launch -- its prediction row (the ring slot under a lossy exchange), its state and, when the solve converged,
its carry record -- is stored write-through at agent scope (`cfz::store_shared`), every storing wavefront waits for its stores, the
workgroup meets and one lane signals; no item writes the L2 back.

The stepwise path (`cfz_loop_step`) gets its visibility from kernel boundaries, so it does not depend on that protocol: one persistent
launch of K iterations must equal K x `cfz_loop_step` bit for bit in state, pred, status and iters (and over the record of every
iteration).  A stale read shows as a difference, not as a fault.

Shapes: 2 scenarios x 4 vehicles, K = 4 -- eight workgroups dealt over the eight XCDs, so every hand-off crosses an L2, and with K >= 3
a prediction parity buffer is rewritten after it has been read; 320 x 4, K = 6 -- 1,280 items of an iteration, more than are resident
at once, so consumers pop on compute units whose L1 and L2 have seen the lines before.  `carry_duals` is on in both: the record is the
largest published object (8.8 KB) and its reader is another workgroup one iteration later.  Kernels: Jacobi, sequential exchange,
disturbed, lossy exchange with max_age 3 (the ring slots), problem pool (problem D stops at 5 iterations, so records are invalidated
too).  The smallest case runs three times in one process and must give the same bits each time.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from disturbance_binding import SIGMA  # noqa: E402
from loop_cases import orders, planned, run, same  # noqa: E402
from problem_pool_binding import problems  # noqa: E402

SHAPES = ((2, 4), (320, 6))
KEYS = ("state", "pred", "status", "iters")


def _setting(kernel, S, V):
    """(order, setup) of loop_cases.run for one kernel variant."""
    if kernel == "jacobi":
        return None, None
    if kernel == "sequential":
        return orders(S, V, seed=5), None
    if kernel == "disturbed":
        return None, lambda e: e.loop_set_disturbance(2024, **SIGMA)
    if kernel == "comm":
        return None, lambda e: e.loop_set_comm(2024, 0.3, max_age=3)
    if kernel == "pool":
        return None, lambda e: e.loop_set_problems(problems(e.spec), np.arange(S) % 4)
    raise ValueError(kernel)


KERNELS = ("jacobi", "sequential", "disturbed", "comm", "pool")


@pytest.fixture(scope="module")
def world():
    from conflict_rez_amd import engine, scenarios

    spec = scenarios.parking_lot_spec()
    S = max(s for s, _ in SHAPES)
    e = engine.Engine(spec, max_batch=S * 4, carry_duals=1)
    table, k0, noise = planned(e, S)
    assert table.shape[0] == 4
    yield e, table, k0, noise
    e.close()


_stepped = {}


def _stepwise(world, kernel, S, K):
    """K x loop_step: computed once per case, shared and read-only."""
    key = (kernel, S, K)
    if key not in _stepped:
        e, table, k0, noise = world
        order, setup = _setting(kernel, S, table.shape[0])
        ref = run(e, (table, k0[:S], noise[:S]), K, "step", order, setup)
        for v in ref.values():
            v.setflags(write=False)
        _stepped[key] = ref
    return _stepped[key]


def _persistent(world, kernel, S, K):
    e, table, k0, noise = world
    order, setup = _setting(kernel, S, table.shape[0])
    return run(e, (table, k0[:S], noise[:S]), K, "run", order, setup)


@pytest.mark.parametrize("S,K", SHAPES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_one_launch_equals_the_steps(world, kernel, S, K):
    ref = _stepwise(world, kernel, S, K)
    assert set(KEYS) <= set(ref) and ref["rec_traj"].shape == (K, S, 4, 7)
    assert (ref["rec_status"] == 0).any()  # converged solves: carry records were written and read
    assert ref["rec_iters"].sum() > 0
    got = _persistent(world, kernel, S, K)
    assert got.keys() == ref.keys()
    same(got, ref, (kernel, S, K))


def test_problem_pool_case_invalidates_records(world):
    """The pool case does take the other path of the record: some solves end unconverged and store `valid = 0`."""
    S, K = SHAPES[1]
    assert (_stepwise(world, "pool", S, K)["rec_status"] != 0).any()


def test_the_smallest_case_repeats(world):
    S, K = SHAPES[0]
    ref = _stepwise(world, "jacobi", S, K)
    for i in range(3):
        same(_persistent(world, "jacobi", S, K), ref, ("repeat", i))
