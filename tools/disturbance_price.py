#!/usr/bin/env python3
"""The price of the disturbed persistent kernels: the same closed loop through loop_kernel / loop_kernel_seq and, with every sigma zero
(identical results, hence identical work), through loop_kernel_dist / loop_kernel_seq_dist.  Kernel times (cfz_last_solve_ms) of
alternated launches, their medians and the ratio; with --sigma also one launch under the base sigmas (another workload: more iterations).
usage: python tools/disturbance_price.py [--scenarios 1024,8192] [--steps 25] [--repeats 5] [--sigma]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIGMA = dict(meas=(0.02, 0.02, 0.005, 0.02, 0.0), act=(0.05, 0.02), proc=(0.005, 0.005, 0.002, 0.01, 0.0))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--scenarios", default="1024,8192")
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sigma", action="store_true")
    a = ap.parse_args()
    from conflict_rez_amd import engine, scenarios

    spec = scenarios.parking_lot_spec()
    table, _ = scenarios.load_reference_table(kind="planned")
    V, K = table.shape[0], a.steps
    zero = dict(meas=np.zeros(5), act=np.zeros(2), proc=np.zeros(5))
    for S in (int(s) for s in a.scenarios.split(",")):
        k0, noise = scenarios.sample_scenarios(S, table, seed=2024, spec=spec)
        eng = engine.Engine(spec, max_batch=S * V)
        order = np.stack([np.random.default_rng(s).permutation(V) for s in range(S)]).astype(np.int32)

        def launch(seq, sig):
            eng.loop_init(table, k0, noise)
            if seq:
                eng.loop_set_order(order)
            if sig is not None:
                eng.loop_set_disturbance(2024, **sig)
            its = eng.loop_run(K)
            return eng.last_solve_ms(), its, eng.loop_get()["state"]

        for seq in (False, True):
            launch(seq, None)  # warm-up
            ms = {"plain": [], "zero": []}
            for _ in range(a.repeats):
                p, z = launch(seq, None), launch(seq, zero)
                assert p[1] == z[1] and np.array_equal(p[2], z[2]), "all sigmas zero must reproduce the undisturbed loop"
                ms["plain"].append(p[0]); ms["zero"].append(z[0])
            mp, mz = float(np.median(ms["plain"])), float(np.median(ms["zero"]))
            line = (f"S {S:5d} K {K} {'sequential' if seq else 'jacobi':10s}: plain {mp:8.2f} ms [{min(ms['plain']):.2f}, {max(ms['plain']):.2f}], "
                    f"disturbed kernels, sigma 0 {mz:8.2f} ms [{min(ms['zero']):.2f}, {max(ms['zero']):.2f}], ratio {mz / mp:.4f}, {p[1]} IPM iterations")
            if a.sigma:
                t, its, _ = launch(seq, SIGMA)
                line += f"; base sigmas {t:.2f} ms, {its} iterations"
            print(line, flush=True)
        eng.close()


if __name__ == "__main__":
    main()
