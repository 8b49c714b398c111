#!/usr/bin/env python3
"""Records tests/golden/planning_surface_parent.npz: what `engine.state_ws`, `colloc` and `joint_colloc_batch` return on the synthetic
four-vehicle strategy (strategy lengths 11, 7, 7, 9), on the GPU, from the library and binding of the tree this script stands in.

    python tests/golden/make_planning_surface.py [OUT.npz]

The fixture was recorded with the commit BEFORE the planning entry points' host code was restated; the kernels are the same
instructions and the host hands them the same bytes, so tests/test_planning_surface_gpu.py holds every later build to it bit
for bit.  It runs `run_cases` below, as this script does, and refuses a fixture in which a plan did not converge.

Cases (unequal lengths are the smallest shape at which per-plan offsets, pair indices and the choice of elimination can go wrong):
  state_ws           B = 4: vehicle 0 without a guess (the reference's `spline_ws_config`), vehicle 1 without a terminal heading
  colloc             B = 4 from those warm starts
  colloc_one_pivot   vehicle 1 alone with one_pivot = 1 (the band elimination one pivot at a time)
  joint2             B = 2 plans of vehicles 2 and 3 (the second from a 5 % longer dt0); the same with pairs = [(0, 1)] must equal it
  joint4_structured, joint4_band   all four vehicles, six pairs, through either elimination"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

TAU = np.array([0.0, 0.05710419611451768, 0.2768430136381238, 0.5835904323689168, 0.8602401356562195, 1.0])
NO_GUESS, NO_HEADING = 0, 1  # the vehicle without a guess / without a terminal heading in every case
STORED = ("state_ws", "colloc", "colloc_one_pivot", "joint2", "joint4_structured", "joint4_band")


def lot():
    """Tubes, guessed paths and terminal headings of the four vehicles (as the `lot` fixture of tests/test_configs_gpu.py)."""
    from conflict_rez_amd import strategy as strat
    from conflict_rez_amd.control.compute_sets import compute_sets, interp_along_sets
    from conflict_rez_amd.vehicle_types import VehicleBody

    hist = strat.generate_strategy(4)
    with tempfile.TemporaryDirectory() as d:
        fn = os.path.join(d, "4v_rl_traj")
        strat.write_strategy(fn, hist)
        sets, paths = compute_sets(fn), interp_along_sets(fn, VehicleBody(), 30)
    agents = sorted(hist)
    tubes = [[((s["back"].A, s["back"].b), (s["front"].A, s["front"].b)) for s in sets[a][1:]] for a in agents]
    return dict(tubes=tubes, paths=[paths[a] for a in agents], fh=[float(paths[a][-1, 2]) for a in agents])


def guess_of(ws, n_sets, nps=5):
    """A state_ws result [T+1, 7] at the collocation points, and dt0 (as tests/test_configs_gpu.py)."""
    N = nps * (n_sets - 1)
    t = 0.1 * np.arange(len(ws))
    ti = (np.arange(N)[:, None] + TAU[None, :]).ravel() / N * t[-1]
    return np.stack([np.interp(ti, t, ws[:, c]) for c in range(7)], 1), t[-1] / N


def state_ws_case(engine, L, ws=None):
    guesses, fh = list(L["paths"]), list(L["fh"])
    guesses[NO_GUESS], fh[NO_HEADING] = None, None
    return engine.state_ws([p[0] for p in L["paths"]], L["tubes"], guesses, fh, ws=ws, shrink_tube=0.5), fh


def run_cases(engine, L, ws=None):
    """{case: list of result dicts}; with a workspace only the first two cases (the `_w` entry points)."""
    from conflict_rez_amd import scenarios

    sp = scenarios.parking_lot_spec(n_nbr=0, N=2)
    tubes, init = L["tubes"], [p[0] for p in L["paths"]]
    out = {}
    out["state_ws"], fh = state_ws_case(engine, L, ws)
    gs = [guess_of(w["traj"], len(t) + 1) for w, t in zip(out["state_ws"], tubes)]
    out["colloc"] = co = engine.colloc(sp, init, tubes, [g[0] for g in gs], [g[1] for g in gs], fh, ws=ws, max_iter=400)
    if ws is not None:
        return out
    v = NO_HEADING
    out["colloc_one_pivot"] = engine.colloc(sp, [init[v]], [tubes[v]], [gs[v][0]], [gs[v][1]], [fh[v]], max_iter=400, one_pivot=1)

    def scenario(vs, stretch=1.0):
        return dict(init_poses=[init[a] for a in vs], tubes=[tubes[a] for a in vs], guesses=[co[a]["traj"].reshape(-1, 7) for a in vs],
                    dt0=stretch * float(np.mean([co[a]["dt"] for a in vs])), final_headings=[fh[a] for a in vs])

    two = [scenario((2, 3)), scenario((2, 3), 1.05)]
    out["joint2"] = engine.joint_colloc_batch(sp, two, max_iter=300)
    out["joint2_pairs"] = engine.joint_colloc_batch(sp, two, pairs=[(0, 1)], max_iter=300)
    four = [scenario((0, 1, 2, 3))]
    out["joint4_structured"] = engine.joint_colloc_batch(sp, four, max_iter=300, structured=1)
    out["joint4_band"] = engine.joint_colloc_batch(sp, four, max_iter=300, structured=0)
    return out


def flatten(results):
    """One case's results as arrays: status, iters, cost, dt (collocation plans), traj [points of all plans and vehicles, 7]."""
    trajs = [t for r in results for t in (r["traj"] if isinstance(r["traj"], list) else [r["traj"]])]
    a = dict(status=np.array([r["status"] for r in results], np.int32), iters=np.array([r["iters"] for r in results], np.int32),
             cost=np.array([r["cost"] for r in results]), traj=np.concatenate([np.asarray(t).reshape(-1, 7) for t in trajs]))
    if "dt" in results[0]:
        a["dt"] = np.array([r["dt"] for r in results])
    return a


def main():
    from conflict_rez_amd import engine

    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "planning_surface_parent.npz")
    res = {k: flatten(v) for k, v in run_cases(engine, lot()).items()}
    for k, a in res.items():
        print(k, "status", a["status"].tolist(), "iters", a["iters"].tolist(), "cost", a["cost"].tolist())
    assert all(np.array_equal(res["joint2"][f], res["joint2_pairs"][f]) for f in res["joint2"]), "explicit pairs differ from the default"
    assert all((res[k]["status"] == 0).all() for k in STORED), "a plan did not converge: take a neighbouring case"
    np.savez_compressed(out, **{f"{k}_{f}": res[k][f] for k in STORED for f in res[k]})
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
