"""The issue priority of the persistent closed loop (`cfz_loop_run`, cfz_loop_body.inl) only reorders instruction issue between the
wavefronts that share a SIMD: whatever is prioritised, every bit of the result stays what it is without priority.

`cfz_loop_run` reads CFZ_LOOP_PRIO_LAG / CFZ_LOOP_PRIO_TAIL at every call, so one process runs the same closed loop under every
setting: off (lag -1), the iteration criterion alone (tail 0), the rank criterion with it (a tail of B / 16 items at the large shape)
and without it (a lag no iteration exceeds), and the built-in default (neither variable set).  Compared with the run without priority:
`loop_get` (state, pred, status, iters) and the record of every iteration (`loop_history`), bit for bit.

Shapes: 320 scenarios x 4 vehicles, 6 iterations -- 1,280 items of an iteration on at most 1,024 resident workgroups, so the compute
units are full, items queue, and both sides of the rank condition occur (positions below and above 1,280 - 80); and 2 scenarios, 4
iterations -- 8 items, fewer than the tail, so every position qualifies.  Kernels: the Jacobi kernel, the sequential-exchange kernel
and the disturbed Jacobi kernel.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from disturbance_binding import SIGMA  # noqa: E402
from loop_cases import orders as _orders  # noqa: E402

VARS = ("CFZ_LOOP_PRIO_LAG", "CFZ_LOOP_PRIO_TAIL")
TAIL = 80  # 1,280 / 16
OFF = {"CFZ_LOOP_PRIO_LAG": "-1"}
SETTINGS = {
    "iteration only": {"CFZ_LOOP_PRIO_LAG": "0", "CFZ_LOOP_PRIO_TAIL": "0"},
    "iteration and rank": {"CFZ_LOOP_PRIO_LAG": "0", "CFZ_LOOP_PRIO_TAIL": str(TAIL)},
    "rank only": {"CFZ_LOOP_PRIO_LAG": "1000", "CFZ_LOOP_PRIO_TAIL": str(TAIL)},
    "built-in": {},
}
SHAPES = ((320, 6), (2, 4))
KERNELS = ("jacobi", "sequential", "disturbed")


class _Env:
    """The two variables set to exactly `values` (the others unset), and put back afterwards."""

    def __init__(self, values):
        self.values = values

    def __enter__(self):
        self.saved = {k: os.environ.pop(k, None) for k in VARS}
        os.environ.update(self.values)

    def __exit__(self, *exc):
        for k in VARS:
            os.environ.pop(k, None)
            if self.saved[k] is not None:
                os.environ[k] = self.saved[k]


@pytest.fixture(scope="module")
def world():
    from conflict_rez_amd import engine, scenarios

    spec = scenarios.parking_lot_spec()
    table, _ = scenarios.load_reference_table(kind="planned")
    S = max(s for s, _ in SHAPES)
    k0, noise = scenarios.sample_scenarios(S, table, seed=2024, spec=spec)
    e = engine.Engine(spec, max_batch=S * table.shape[0])
    yield e, table, k0, noise
    e.close()


def _run(world, kernel, S, K, env):
    e, table, k0, noise = world
    V = table.shape[0]
    e.loop_init(table, k0[:S], noise[:S])
    if kernel == "sequential":
        e.loop_set_order(_orders(S, V, seed=5))
    elif kernel == "disturbed":
        e.loop_set_disturbance(2024, **SIGMA)
    e.loop_record(K)
    with _Env(env):
        its = e.loop_run(K)
    out = {**e.loop_get(), **{"history_" + k: v for k, v in e.loop_history().items()}}
    out["ipm_iterations"] = np.asarray(its, np.int64)
    return out


_reference = {}


def _without_priority(world, kernel, S, K):
    key = (kernel, S, K)
    if key not in _reference:
        ref = _run(world, kernel, S, K, OFF)
        for v in ref.values():
            v.setflags(write=False)
        _reference[key] = ref
    return _reference[key]


@pytest.mark.parametrize("S,K", SHAPES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_results_do_not_depend_on_the_priority_setting(world, kernel, S, K):
    ref = _without_priority(world, kernel, S, K)
    assert ref["history_traj"].shape == (K, S, 4, 7) and int(ref["ipm_iterations"]) == int(ref["history_iters"].sum()) > 0
    assert (ref["status"] == 0).any()  # the loop did solve something
    for name, env in SETTINGS.items():
        got = _run(world, kernel, S, K, env)
        assert got.keys() == ref.keys()
        for k in ref:
            assert np.array_equal(got[k], ref[k]), (kernel, S, K, name, k, int((np.asarray(got[k]) != np.asarray(ref[k])).sum()))
