#!/usr/bin/env python3
"""The price of the lossy-exchange persistent kernels: the same closed loop through loop_kernel / loop_kernel_seq and, with p_drop = 0
(identical results, hence identical work), through loop_kernel_comm / loop_kernel_seq_comm and the ring of messages.  Kernel times
(cfz_last_solve_ms) of alternated launches in one process, their medians, the ratio and the spread of the plain launches alone; then
one launch each at p_drop = 0.1 and 0.3 under both `compensate` settings (another workload), with the interior-point iterations per
solve beside the time.
usage: python tools/comm_price.py [--scenarios 1024,8192] [--steps 25] [--repeats 5] [--max-age 3] [--rates 0.1,0.3]"""
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
    ap.add_argument("--max-age", type=int, default=3)
    ap.add_argument("--rates", default="0.1,0.3")
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

        def launch(seq, p, compensate=True):
            eng.loop_init(table, k0, noise)
            if seq:
                eng.loop_set_order(order)
            if p is not None:
                eng.loop_set_comm(2024, p, max_age=a.max_age, compensate=compensate)
            its = eng.loop_run(K)
            return eng.last_solve_ms(), its, eng.loop_get()["state"], eng.loop_last_converged()

        for seq in (False, True):
            launch(seq, None)  # warm-up
            ms = {"plain": [], "zero": []}
            for _ in range(a.repeats):
                p, z = launch(seq, None), launch(seq, 0.0)
                assert p[1] == z[1] and np.array_equal(p[2], z[2]), "p_drop = 0 must reproduce the lossless loop"
                ms["plain"].append(p[0]); ms["zero"].append(z[0])
            mp, mz = float(np.median(ms["plain"])), float(np.median(ms["zero"]))
            name = "sequential" if seq else "jacobi"
            print(f"S {S:5d} K {K} {name:10s}: plain {mp:8.2f} ms [{min(ms['plain']):.2f}, {max(ms['plain']):.2f}] (spread x "
                  f"{min(ms['plain']) / mp:.4f} .. {max(ms['plain']) / mp:.4f}), comm kernels, p_drop 0 {mz:8.2f} ms [{min(ms['zero']):.2f}, "
                  f"{max(ms['zero']):.2f}], ratio {mz / mp:.4f}, {p[1] / (S * V * K):.2f} IPM iterations per solve", flush=True)
            for rate in rates:
                for comp in (False, True):
                    t, its, _, conv = launch(seq, rate, comp)
                    print(f"    p_drop {rate:g} compensate {int(comp)}: {t:8.2f} ms (x {t / mp:.3f} of plain), {its / (S * V * K):.2f} IPM iterations per solve, "
                          f"{conv} of {S * V * K} solves converged", flush=True)
        eng.close()


if __name__ == "__main__":
    main()
