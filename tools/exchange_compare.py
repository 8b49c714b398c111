#!/usr/bin/env python3
"""Jacobi against the sequential exchange (`Engine.loop_set_order`) on the same closed-loop workloads.

Workloads: the bench workload (planned table, feasible starts of `sample_scenarios(..., spec=spec)` with seeds 2024 / 2025 / 2026, 1,024
scenarios x 4 vehicles, 5 warm-up and 20 timed iterations in one persistent launch) and the same with 8,192 scenarios (seed 2024).
The sequential mode solves every scenario's vehicles in the strategy's planning priority (`strategy.DEFAULT_ORDER`, the order the
planned table was made in).  Per workload and mode: converged solves/s and all solves/s, interior-point iterations/s, the converged
share and the status counts, the longest chain (the most interior-point iterations summed over one scenario's timed solves: under the
sequential exchange they run one after another), and for the sequential mode the wall time of the persistent launch against the
stepwise loop (20 `loop_step`s, V solve launches each) on the same timed window.

usage: python tools/exchange_compare.py [--scenarios 1024 8192] [--warmup 5] [--steps 20] [--json OUT]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def run(eng, table, k0, noise, order, warmup, steps, stepwise=False):
    eng.loop_init(table, k0, noise)
    eng.loop_set_order(order)
    if warmup:
        eng.loop_run(warmup)
    eng.loop_record(steps)
    t0 = time.perf_counter()
    if stepwise:
        for _ in range(steps):
            eng.loop_step()
        its = None
    else:
        its = eng.loop_run(steps)  # returns after a device synchronise
    wall = time.perf_counter() - t0
    h = eng.loop_history()
    st, it = h["status"], h["iters"]  # [K, S, V]
    B = st.shape[1] * st.shape[2]
    out = dict(wall_s=wall, solves=int(st.size), converged=int((st == 0).sum()), ipm_iterations=int(it.sum()),
               status_counts=np.bincount(np.clip(st.ravel(), 0, 5), minlength=6).tolist(),
               longest_chain=int(it.sum(axis=(0, 2)).max()), mean_chain=float(it.sum(axis=(0, 2)).mean()))
    if its is not None:
        assert its == out["ipm_iterations"]
    out.update(converged_per_s=out["converged"] / wall, solves_per_s=out["solves"] / wall, ipm_iters_per_s=out["ipm_iterations"] / wall,
               converged_share=out["converged"] / out["solves"], ms_per_step=1e3 * wall / steps, B=B)
    return out, eng.loop_get()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--scenarios", type=int, nargs="+", default=[1024, 8192])
    ap.add_argument("--seeds", type=int, nargs="+", default=[2024, 2025, 2026], help="sampler seeds of the first workload")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    from conflict_rez_amd import engine, scenarios
    from conflict_rez_amd import strategy as strat

    spec = scenarios.parking_lot_spec()
    table, _ = scenarios.load_reference_table(kind="planned")
    V = table.shape[0]
    prio = np.array([i for i in strat.DEFAULT_ORDER if i < V], np.int32)
    eng = engine.Engine(spec, max_batch=max(a.scenarios) * V)
    rows = []
    for i, S in enumerate(a.scenarios):
        for seed in (a.seeds if i == 0 else a.seeds[:1]):
            k0, noise = scenarios.sample_scenarios(S, table, seed=seed, spec=spec)
            res = {}
            for mode, order in (("jacobi", None), ("sequential", prio)):
                res[mode], last = run(eng, table, k0, noise, order, a.warmup, a.steps)
                if mode == "sequential":
                    step, last_step = run(eng, table, k0, noise, order, a.warmup, a.steps, stepwise=True)
                    same = all(np.array_equal(last[k], last_step[k]) for k in last)
                    res[mode].update(stepwise_wall_s=step["wall_s"], stepwise_equal_bitwise=bool(same))
            for mode, r in res.items():
                rows.append(dict(scenarios=S, seed=seed, mode=mode, **r))
                extra = (f", stepwise {r['stepwise_wall_s'] * 1e3:.0f} ms ({'equal' if r['stepwise_equal_bitwise'] else 'DIFFERENT'} bit for bit)"
                         if mode == "sequential" else "")
                print(f"S={S:5d} seed={seed} {mode:10s}: {r['converged_per_s'] / 1e6:5.2f} M converged solves/s ({r['solves_per_s'] / 1e6:5.2f} M all), "
                      f"{r['ipm_iters_per_s'] / 1e6:5.2f} M IPM iterations/s, converged {r['converged_share']:.3f}, status {r['status_counts']}, "
                      f"longest chain {r['longest_chain']} (mean {r['mean_chain']:.0f}), {r['ms_per_step']:.2f} ms/step; "
                      f"persistent {r['wall_s'] * 1e3:.0f} ms{extra}", flush=True)
            j, s_ = res["jacobi"], res["sequential"]
            print(f"S={S:5d} seed={seed} sequential / jacobi: IPM iterations/s {s_['ipm_iters_per_s'] / j['ipm_iters_per_s']:.3f}, "
                  f"converged solves/s {s_['converged_per_s'] / j['converged_per_s']:.3f}", flush=True)
    eng.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
