"""Shared by the map-pool tests (tests/test_map_pool_gpu.py, tests/test_map_pool_host.py): the four test maps of `cfz_loop_set_maps`
over the `parking_lot_spec()` handle and the host replay (oracle/closed_loop.replay) of a batch whose scenarios stand on different maps.

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


def replay_mixed(ospec, maps_, map_of, table, k0, noise, steps, dt, wb, order=None, scenarios_=None):
    """The host replay of a batch on mixed maps, scenario by scenario with the scenario's own obstacles in the MpcSpec (scenarios do not
    interact); scenarios_ (default: all) are the ones replayed, the others stay zero.
    -> per step (state [S,V,5], status [S,V], iters [S,V])."""
    from oracle.closed_loop import replay

    S, V = len(k0), table.shape[0]
    out = [(np.zeros((S, V, 5)), np.zeros((S, V), int), np.zeros((S, V), int)) for _ in range(steps)]
    for s in (range(S) if scenarios_ is None else scenarios_):
        A, b = maps_[map_of[s]]
        osp = dataclasses.replace(ospec, A_obs=np.array(A, float), b_obs=np.array(b, float))
        gen = replay(osp, table, k0[s : s + 1], noise[s : s + 1], steps, dt=dt, wb=wb, order=None if order is None else order[s : s + 1])
        for t, (state, _, status, iters) in enumerate(gen):
            out[t][0][s], out[t][1][s], out[t][2][s] = state[0], status[0], iters[0]
    return out
