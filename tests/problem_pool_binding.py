"""Shared by the problem-pool tests (tests/test_problem_pool_gpu.py, tests/test_problem_pool_host.py): the four test problems of
`cfz_loop_set_problems` over the `parking_lot_spec()` handle and their form for the host replay (oracle/closed_loop.replay).

  A  the handle's own problem
  B  dmin 0.2 (the handle: 0.05)
  C  the v box and the input boxes tightened: v in [-1.8, 1.8], a in [-0.8, 0.8], w in [-0.5, 0.5]
  D  other weights (20, 20, 50, 2, 2, 5) and max_iter 5

Not a test module: no test_ prefix."""
import dataclasses

import numpy as np

C_BOUNDS = {4: -1.8, 5: 1.8, 8: -0.8, 9: 0.8, 10: -0.5, 11: 0.5}  # index into cfz_spec.bounds (lo, hi of x, y, v, delta, a, w)
D_WEIGHTS = (20.0, 20.0, 50.0, 2.0, 2.0, 5.0)
D_OPTIONS = dict(max_iter=5)
NAMES = "ABCD"


def problems(spec):
    """[A, B, C, D] as `Engine.loop_set_problems` takes them, over the handle's ProblemSpec."""
    bc = np.array(spec.bounds, float)
    for i, v in C_BOUNDS.items():
        bc[i] = v
    return [spec, dataclasses.replace(spec, dmin=0.2), dataclasses.replace(spec, bounds=bc),
            (dataclasses.replace(spec, weights=np.array(D_WEIGHTS)), dict(D_OPTIONS))]


def spec_of(item):
    return item[0] if isinstance(item, tuple) else item


def options_of(item):
    return item[1] if isinstance(item, tuple) else {}


def oracle_problem(ospec, item):
    """(MpcSpec, IpmOptions) of one entry of `problems` for the host replay, from the MpcSpec of the handle's problem."""
    from oracle.ipm import IpmOptions

    sp = spec_of(item)
    return (dataclasses.replace(ospec, dmin=sp.dmin, bounds=np.array(sp.bounds, float), weights=np.array(sp.weights, float)),
            IpmOptions(**options_of(item)))

