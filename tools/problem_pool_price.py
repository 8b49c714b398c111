#!/usr/bin/env python3
"""The price of the problem-pool persistent kernels: the same closed loop through loop_kernel / loop_kernel_seq and, with every problem
of the pool equal to the handle's own (identical results, hence identical work), through loop_kernel_pool / loop_kernel_seq_pool: once with
a pool of P = 1 problem that every scenario reads, once with P = S copies at distinct addresses, one per scenario (the resident
instances of a CU then read different 2 KB blocks through one scalar cache).  Kernel times (cfz_last_solve_ms) of alternated launches in
one process, their medians, the ratios and the spread of the plain launches alone.
usage: python tools/problem_pool_price.py [--scenarios 1024,8192] [--steps 25] [--repeats 5]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--scenarios", default="1024,8192")
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    from conflict_rez_amd import engine, scenarios

    spec = scenarios.parking_lot_spec()
    table, _ = scenarios.load_reference_table(kind="planned")
    V, K = table.shape[0], a.steps
    for S in (int(s) for s in a.scenarios.split(",")):
        k0, noise = scenarios.sample_scenarios(S, table, seed=2024, spec=spec)
        eng = engine.Engine(spec, max_batch=S * V)
        order = np.stack([np.random.default_rng(s).permutation(V) for s in range(S)]).astype(np.int32)
        pools = {"plain": None, "P=1": ([spec], np.zeros(S, np.int32)), "P=S": ([spec] * S, np.arange(S, dtype=np.int32))}

        def launch(seq, pool):
            eng.loop_init(table, k0, noise)
            if seq:
                eng.loop_set_order(order)
            if pool is not None:
                eng.loop_set_problems(*pool)
            its = eng.loop_run(K)
            return eng.last_solve_ms(), its, eng.loop_get()["state"]

        for seq in (False, True):
            launch(seq, None)  # warm-up
            ms = {k: [] for k in pools}
            for _ in range(a.repeats):
                res = {k: launch(seq, pool) for k, pool in pools.items()}
                for k, r in res.items():
                    assert r[1] == res["plain"][1] and np.array_equal(r[2], res["plain"][2]), "a pool of the handle's own problem must reproduce the plain loop"
                    ms[k].append(r[0])
            med = {k: float(np.median(v)) for k, v in ms.items()}
            mp = med["plain"]
            name = "sequential" if seq else "jacobi"
            print(f"S {S:5d} K {K} {name:10s}: plain {mp:8.2f} ms [{min(ms['plain']):.2f}, {max(ms['plain']):.2f}] (spread x "
                  f"{min(ms['plain']) / mp:.4f} .. {max(ms['plain']) / mp:.4f}); "
                  + "; ".join(f"pool {k} {med[k]:8.2f} ms [{min(ms[k]):.2f}, {max(ms[k]):.2f}], ratio {med[k] / mp:.4f}" for k in ("P=1", "P=S"))
                  + f"; {res['plain'][1] / (S * V * K):.2f} IPM iterations per solve", flush=True)
        eng.close()


if __name__ == "__main__":
    main()
