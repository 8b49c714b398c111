"""Shared by the map-pool tests (tests/test_map_pool_gpu.py, tests/test_map_pool_host.py): the four test maps of `cfz_loop_set_maps`
over the `parking_lot_spec()` handle and their form for the host replay (oracle/closed_loop.replay, which takes one MpcSpec per scenario).

  A  the handle's own obstacles
  B  every face moved outwards by 0.10 m (`scenarios.grow_obstacles`)
  C  every face moved outwards by 0.20 m
  D  every obstacle shifted by (0.15, -0.15) m (`scenarios.shift_obstacles`)

Not a test module: no test_ prefix."""
import dataclasses

import numpy as np

NAMES = "ABCD"
GROW_B, GROW_C, SHIFT_D = 0.10, 0.20, (0.15, -0.15)


def maps(spec):
    """[A, B, C, D] as (A_obs [n_obs,4,2], b_obs [n_obs,4]) pairs, as `Engine.loop_set_maps` takes them, over the handle's ProblemSpec."""
    from conflict_rez_amd import scenarios

    return [(np.array(spec.A_obs, float), np.array(spec.b_obs, float)), scenarios.grow_obstacles(spec, GROW_B),
            scenarios.grow_obstacles(spec, GROW_C), scenarios.shift_obstacles(spec, *SHIFT_D)]


def vertices(A, b):
    """[n_obs, 4, 2] corners of a map's obstacles (tests/audit_binding.obstacle_vertices)."""
    import audit_binding as ab

    return np.stack([ab.obstacle_vertices(A[j], b[j]) for j in range(len(A))])


def oracle_spec(ospec, m):
    """The MpcSpec of the handle's problem on the map m = (A_obs, b_obs), for the host replay."""
    A, b = m
    return dataclasses.replace(ospec, A_obs=np.array(A, float), b_obs=np.array(b, float))
