#!/usr/bin/env python3
"""The price of a setting's persistent kernels: the same closed loop through loop_kernel / loop_kernel_seq and, with the setting switched
on at a neutral value (identical results, hence identical work), through the kernels compiled for it.  Kernel times (cfz_last_solve_ms)
of alternated launches in one process, their medians, the ratios and the spread of the plain launches alone.

  --setting disturbance  every sigma zero: loop_kernel_dist / loop_kernel_seq_dist; with --sigma also one launch under the base sigmas
                         (another workload: more iterations)
  --setting comm         p_drop = 0: loop_kernel_comm / loop_kernel_seq_comm and the ring of messages; then one launch each at the
                         --rates under both `compensate` settings (another workload), with the interior-point iterations per solve
  --setting pool         every problem the handle's own: loop_kernel_pool / loop_kernel_seq_pool, once with a pool of P = 1 problem that
                         every scenario reads, once with P = S copies at distinct addresses, one per scenario (the resident instances of
                         a CU then read different 2 KB blocks through one scalar cache)
  --setting maps         every map the handle's own: the same pool kernels, once with M = 1 map that every scenario reads, once with M = S
                         copies at distinct addresses, one per scenario (S blocks as under P = S, and S distinct 960-byte obstacle tables
                         read through vector loads where the plain kernels read one shared table)

usage: python tools/loop_price.py --setting disturbance|comm|pool|maps [--scenarios 1024,8192] [--steps 25] [--repeats 5]
                                  [--sigma] [--max-age 3] [--rates 0.1,0.3]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIGMA = dict(meas=(0.02, 0.02, 0.005, 0.02, 0.0), act=(0.05, 0.02), proc=(0.005, 0.005, 0.002, 0.01, 0.0))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--setting", required=True, choices=("disturbance", "comm", "pool", "maps"))
    ap.add_argument("--scenarios", default="1024,8192")
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sigma", action="store_true", help="disturbance: one more launch under the base sigmas")
    ap.add_argument("--max-age", type=int, default=3, help="comm")
    ap.add_argument("--rates", default="0.1,0.3", help="comm: drop rates of the extra launches")
    a = ap.parse_args()
    from conflict_rez_amd import engine, scenarios

    spec = scenarios.parking_lot_spec()
    table, _ = scenarios.load_reference_table(kind="planned")
    V, K = table.shape[0], a.steps
    rates = [float(r) for r in a.rates.split(",") if r]
    for S in (int(s) for s in a.scenarios.split(",")):
        k0, noise = scenarios.sample_scenarios(S, table, seed=2024, spec=spec)
        eng = engine.Engine(spec, max_batch=S * V)
        order = np.stack([np.random.default_rng(s).permutation(V) for s in range(S)]).astype(np.int32)
        # the neutral forms of the setting: name -> what switches it on (plain: nothing), and what an unequal result is called
        neutral, claim = {
            "disturbance": ({"zero": lambda e: e.loop_set_disturbance(2024, meas=np.zeros(5), act=np.zeros(2), proc=np.zeros(5))},
                            "all sigmas zero must reproduce the undisturbed loop"),
            "comm": ({"zero": lambda e: e.loop_set_comm(2024, 0.0, max_age=a.max_age)}, "p_drop = 0 must reproduce the lossless loop"),
            "pool": ({"P=1": lambda e: e.loop_set_problems([spec], np.zeros(S, np.int32)),
                      "P=S": lambda e: e.loop_set_problems([spec] * S, np.arange(S, dtype=np.int32))},
                     "a pool of the handle's own problem must reproduce the plain loop"),
            "maps": ({"M=1": lambda e: e.loop_set_maps([spec], np.zeros(S, np.int32)),
                      "M=S": lambda e: e.loop_set_maps([spec] * S, np.arange(S, dtype=np.int32))},
                     "a pool of the handle's own map must reproduce the plain loop")}[a.setting]
        forms = {"plain": None, **neutral}

        def launch(seq, setup):
            eng.loop_init(table, k0, noise)
            if seq:
                eng.loop_set_order(order)
            if setup is not None:
                setup(eng)
            its = eng.loop_run(K)
            return eng.last_solve_ms(), its, eng.loop_get()["state"], eng.loop_last_converged()

        for seq in (False, True):
            launch(seq, None)  # warm-up
            ms = {k: [] for k in forms}
            for _ in range(a.repeats):
                res = {k: launch(seq, setup) for k, setup in forms.items()}
                for k, r in res.items():
                    assert r[1] == res["plain"][1] and np.array_equal(r[2], res["plain"][2]), claim
                    ms[k].append(r[0])
            med = {k: float(np.median(v)) for k, v in ms.items()}
            mp, its = med["plain"], res["plain"][1]
            rng = {k: f"[{min(v):.2f}, {max(v):.2f}]" for k, v in ms.items()}
            head = f"S {S:5d} K {K} {'sequential' if seq else 'jacobi':10s}: plain {mp:8.2f} ms {rng['plain']}"
            spread = f" (spread x {min(ms['plain']) / mp:.4f} .. {max(ms['plain']) / mp:.4f})"
            if a.setting == "disturbance":
                line = head + f", disturbed kernels, sigma 0 {med['zero']:8.2f} ms {rng['zero']}, ratio {med['zero'] / mp:.4f}, {its} IPM iterations"
                if a.sigma:
                    t, n, *_ = launch(seq, lambda e: e.loop_set_disturbance(2024, **SIGMA))
                    line += f"; base sigmas {t:.2f} ms, {n} iterations"
                print(line, flush=True)
            elif a.setting == "comm":
                print(head + spread + f", comm kernels, p_drop 0 {med['zero']:8.2f} ms {rng['zero']}, ratio {med['zero'] / mp:.4f}, "
                      f"{its / (S * V * K):.2f} IPM iterations per solve", flush=True)
                for rate in rates:
                    for comp in (False, True):
                        t, n, _, conv = launch(seq, lambda e: e.loop_set_comm(2024, rate, max_age=a.max_age, compensate=comp))
                        print(f"    p_drop {rate:g} compensate {int(comp)}: {t:8.2f} ms (x {t / mp:.3f} of plain), {n / (S * V * K):.2f} IPM iterations per solve, "
                              f"{conv} of {S * V * K} solves converged", flush=True)
            else:
                print(head + spread + "; " + "; ".join(f"{a.setting} {k} {med[k]:8.2f} ms {rng[k]}, ratio {med[k] / mp:.4f}" for k in neutral)
                      + f"; {its / (S * V * K):.2f} IPM iterations per solve", flush=True)
        eng.close()


if __name__ == "__main__":
    main()
