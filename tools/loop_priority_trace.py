#!/usr/bin/env python3
"""What the issue priority of the persistent closed loop does to the launch's critical path, measured inside the launch.

Needs the diagnostic build of the library with the per-item trace:

    bash tools/build_variant.sh tools/_libcfz_trace.so -DCFZ_LOOP_TRACE
    CFZ_LIBRARY=tools/_libcfz_trace.so python tools/loop_priority_trace.py [--scenarios 1024 --steps 20 --warmup 5 --seed 2024]

It runs bench.py's headline launch (feasible starts, `warmup` iterations, then `steps` iterations in one `cfz_loop_run`) once per
priority setting (CFZ_LOOP_PRIO_LAG / CFZ_LOOP_PRIO_TAIL, read by cfz_loop_run at every call): off, the iteration criterion alone, and the
rank criterion with tails of B/4, B/16 and B/64 items (`--settings` chooses).  The trace gives, per item (t, b), the 100 MHz clock
after the pop, around the solve and after the release, and whether the item ran prioritised; `loop_history` gives its interior-point
iterations.

Reported per setting: the launch's length on the trace clock; the scenario with the longest chain (most interior-point iterations
summed over its vehicles' slowest solve per MPC iteration -- under the Jacobi exchange an iteration of a scenario lasts as long as its
slowest vehicle); and, for the items of that scenario, microseconds of solve per interior-point iteration by how full the GPU is
while the solve runs: the mean number of items in flight over the solve's interval as a share of the launch's resident workgroups (the
grid) -- full (at least 95 %), shared (25 to 95 %), sparse (below 25 %: with four workgroups per compute unit, mostly alone on its
SIMDs).  In brackets the interior-point iterations each figure rests on.  The same three figures over all items stand beside them, and
the time until which some solve still ran on a full GPU.

`--load NPZ` analyses traces kept with `--save` again (no GPU, no library)."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WORDS, TICK_US = 5, 0.01  # cfz_engine.hip kLoopTraceWords; the constant clock runs at 100 MHz


def in_flight_mean(start, end, a, b):
    """Mean number of intervals [start, end) open over each [a, b): from the cumulative integral of the in-flight count."""
    ev = np.concatenate([start, end])
    dv = np.concatenate([np.ones(len(start)), -np.ones(len(end))])
    o = np.argsort(ev, kind="stable")
    ev, cnt = ev[o], np.cumsum(dv[o])
    integ = np.concatenate([[0.0], np.cumsum(cnt[:-1] * np.diff(ev))])  # integral of the count up to ev[i]

    def upto(x):
        i = np.clip(np.searchsorted(ev, x, side="right") - 1, 0, len(ev) - 1)
        return integ[i] + cnt[i] * (x - ev[i])

    return (upto(b) - upto(a)) / np.maximum(b - a, 1)


def header():
    print("solve time per interior-point iteration in us, by the GPU's load during the solve (interior-point iterations in brackets)")
    print(f"{'setting':>8s} {'launch ms':>9s} {'prioritised':>11s} | {'chain of':>8s} {'its':>5s} {'full':>14s} {'shared':>14s} {'sparse':>14s} | "
          f"{'all: full':>9s} {'shared':>7s} {'sparse':>7s} {'full until ms':>13s}")


def report(name, tr, its, grid, V):
    """One line for one launch: tr [K, B, WORDS] the trace, its [K, B] the interior-point iterations of every item."""
    K, B = its.shape
    S = B // V
    assert (tr[..., 4] > 0).all(), "items without a record"
    t_origin = tr[..., 0].min()
    pop, s0, s1, rel = (tr[..., i] - t_origin for i in range(4))
    prio = tr[..., 4] == 2
    load = in_flight_mean(pop.ravel(), rel.ravel(), s0.ravel().astype(float), s1.ravel().astype(float)).reshape(K, B) / grid
    classes = (load >= 0.95, (load >= 0.25) & (load < 0.95), load < 0.25)
    solve_us = (s1 - s0) * TICK_US
    # the longest chain: per scenario and MPC iteration the slowest vehicle's iterations, summed over the launch
    chain = its.reshape(K, S, V).max(2).sum(0)
    sc = int(chain.argmax())
    sel = np.zeros((K, B), bool)
    sel[:, sc * V:(sc + 1) * V] = True

    def rate(mask):
        n = int(its[mask].sum())
        return (solve_us[mask].sum() / n if n else float("nan")), n

    full_until = rel[classes[0]].max() * TICK_US / 1e3 if classes[0].any() else 0.0
    print(f"{name:>8s} {rel.max() * TICK_US / 1e3:9.2f} {int(prio.sum()):11d} | {sc:8d} {int(chain[sc]):5d} "
          + " ".join("{:6.1f} ({:5d})".format(*rate(sel & c)) for c in classes) + " | "
          + " ".join(f"{rate(c)[0]:{w}.1f}" for c, w in zip(classes, (9, 7, 7))) + f" {full_until:13.2f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenarios", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--settings", default="off,iter,4,16,64", help="comma list of: off, iter, default, or a divisor d (tail of B/d items)")
    ap.add_argument("--save", metavar="NPZ", help="keep every setting's trace and iteration counts")
    ap.add_argument("--load", metavar="NPZ", help="analyse the traces of an earlier --save instead of running")
    a = ap.parse_args()
    if a.load:
        d = np.load(a.load)
        header()
        for name in [k[:-6] for k in d.files if k.endswith("_trace")]:
            report(name, d[name + "_trace"], d[name + "_iters"], int(d["grid"]), int(d["V"]))
        return
    from conflict_rez_amd import engine, scenarios

    lib = engine.load_library()
    if not hasattr(lib, "cfz_loop_trace_read"):
        sys.exit("this library has no trace: build it with -DCFZ_LOOP_TRACE and name it in CFZ_LIBRARY (see the module's docstring)")
    lib.cfz_loop_trace_read.restype = C.c_int
    lib.cfz_loop_trace_read.argtypes = [C.c_void_p, C.c_long]
    spec = scenarios.parking_lot_spec()
    table, _ = scenarios.load_reference_table(kind="planned")
    V, S, K = table.shape[0], a.scenarios, a.steps
    B = S * V
    k0, noise = scenarios.sample_scenarios(S, table, seed=a.seed, spec=spec)
    e = engine.Engine(spec, max_batch=B)
    keep = {}
    print(f"{S} scenarios x {V} vehicles, {a.warmup} + {K} MPC iterations, sampler seed {a.seed}")
    header()
    for name in a.settings.split(","):
        env = {"off": {"CFZ_LOOP_PRIO_LAG": "-1"}, "iter": {"CFZ_LOOP_PRIO_LAG": "0", "CFZ_LOOP_PRIO_TAIL": "0"}, "default": {}}.get(name)
        if env is None:
            env = {"CFZ_LOOP_PRIO_LAG": "0", "CFZ_LOOP_PRIO_TAIL": str(max(1, B // int(name)))}
        for k in ("CFZ_LOOP_PRIO_LAG", "CFZ_LOOP_PRIO_TAIL"):
            os.environ.pop(k, None)
        os.environ.update(env)
        e.loop_init(table, k0, noise)
        if a.warmup:
            e.loop_run(a.warmup)
        e.loop_record(K)
        e.loop_run(K)
        its = e.loop_history()["iters"].reshape(K, B).astype(np.int64)
        tr = np.zeros((K * B, WORDS), np.int64)
        grid = lib.cfz_loop_trace_read(tr.ctypes.data_as(C.c_void_p), K * B)
        if grid < 0:
            sys.exit("cfz_loop_trace_read failed: " + lib.cfz_last_error().decode())
        tr = tr.reshape(K, B, WORDS)
        report(name, tr, its, grid, V)
        keep[f"{name}_trace"], keep[f"{name}_iters"] = tr, its
    e.close()
    if a.save:
        np.savez_compressed(a.save, grid=grid, V=V, **keep)


if __name__ == "__main__":
    main()
