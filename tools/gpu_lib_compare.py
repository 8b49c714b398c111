#!/usr/bin/env python3
"""Two builds of the library on the same seeded MPC batch: are the results equal bit for bit?  Cold solves; a Jacobi persistent run of 6
steps; 3 `loop_step`s, Jacobi and under seeded orders; a sequential persistent run of 4; a disturbed persistent run of 4 (the sigmas of
tests/disturbance_binding.SIGMA); a lossy exchange (p_drop 0.3), Jacobi and sequential, run of 4; the pool of the four problems of
tests/problem_pool_binding.py under noise, run of 4 and stepped 3 times; and runs of 4 through the remaining persistent kernels
(sequential + noise, sequential + pool, pool + loss, sequential + pool + loss), so that all ten and both stepwise solve kernels are
compared; and, where both builds have cfz_loop_set_maps, the four maps of tests/map_pool_binding.py under noise, run of 4 and stepped 3
times, and together with the problems, the sequential order and loss, each with its audit; and the plan-set entry points
(plan_conflicts, plan_delays, delay_search, plan_coordination, plan_schedule on the cases of tests/conflict_binding.py, delay_binding.py
and schedule_binding.py; loop_plan_conflicts / _delays / _schedule on the packaged pool).  Every loop is compared at its end point and
over its record; the exit status is 1 when anything differs.  A key that only the second build has is listed, not compared.
usage: python tools/gpu_lib_compare.py <libA.so> <libB.so> [scenarios]     (each library runs in a process of its own)"""
import os, subprocess, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if len(sys.argv) > 1 and sys.argv[1] == "--child":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conflict_rez_amd import engine, scenarios
    from disturbance_binding import SIGMA
    from problem_pool_binding import problems
    from map_pool_binding import maps as test_maps
    lib, S, out = sys.argv[2], int(sys.argv[3]), sys.argv[4]
    engine._lib = engine.load_library(lib)
    spec = scenarios.parking_lot_spec()
    table, _ = scenarios.load_reference_table(kind="planned")
    k0, noise = scenarios.sample_scenarios(S, table, seed=11)  # raw draws: restorations, status 4 / 5 among them
    x0, ref, nbr, zu = scenarios.mpc_batch_from_table(spec, table, k0, noise)
    V = table.shape[0]
    e = engine.Engine(spec, max_batch=len(x0))
    r = e.solve(x0, ref, nbr, zu, want_duals=False)
    res = dict(status=r["status"], iters=r["iters"], zu=r["zu"], ms=r["solve_ms"])

    def loop(tag, setup, go):  # one closed loop from the same start; its end point and record under <tag>_*
        e.loop_init(table, k0, noise)
        setup()
        e.loop_record(8)
        res[tag + "_its"] = go() or 0
        res.update({f"{tag}_{k}": v for k, v in {**e.loop_get(), **e.loop_history()}.items()})

    def three_steps():
        for _ in range(3):
            e.loop_step()

    order = np.stack([np.random.default_rng(5).permutation(V) for _ in range(S)]).astype(np.int32)
    loop("loop", lambda: None, lambda: e.loop_run(6))
    loop("step", lambda: None, three_steps)
    loop("seq", lambda: e.loop_set_order(order), lambda: e.loop_run(4))
    loop("seqstep", lambda: e.loop_set_order(order), three_steps)
    loop("dist", lambda: e.loop_set_disturbance(2024, **SIGMA), lambda: e.loop_run(4))
    probs, pof = problems(spec), np.arange(S) % 4

    def setting(seq=False, noise=False, comm=False, pool=False, maps=False):
        def setup():
            if seq:
                e.loop_set_order(order)
            if noise:
                e.loop_set_disturbance(2024, **SIGMA)
            if comm:
                e.loop_set_comm(2024, 0.3, max_age=3)
            if pool:
                e.loop_set_problems(probs, pof)
            if maps:
                e.loop_set_maps(test_maps(spec), (np.arange(S) // 4) % 4)
        return setup

    loop("comm", setting(comm=True), lambda: e.loop_run(4))
    loop("seqcomm", setting(seq=True, comm=True), lambda: e.loop_run(4))
    loop("pool", setting(noise=True, pool=True), lambda: e.loop_run(4))
    loop("poolstep", setting(noise=True, pool=True), three_steps)
    loop("seqdist", setting(seq=True, noise=True), lambda: e.loop_run(4))
    loop("seqpool", setting(seq=True, pool=True), lambda: e.loop_run(4))
    loop("poolcomm", setting(comm=True, pool=True), lambda: e.loop_run(4))
    loop("seqpoolcomm", setting(seq=True, comm=True, pool=True), lambda: e.loop_run(4))
    res.update({"audit_" + k: v for k, v in e.loop_audit().items()})  # audit_kernel, on the handle's map
    if hasattr(e.lib, "cfz_loop_set_maps"):
        loop("maps", setting(noise=True, maps=True), lambda: e.loop_run(4))
        res.update({"maps_audit_" + k: v for k, v in e.loop_audit().items()})
        loop("mapsstep", setting(noise=True, maps=True), three_steps)
        loop("seqpoolmapscomm", setting(seq=True, comm=True, pool=True, maps=True), lambda: e.loop_run(4))
        res.update({"seqpoolmapscomm_audit_" + k: v for k, v in e.loop_audit().items()})
    # the plan-set entry points: the cases of the binding modules of tests/, and the packaged pool from the loop's copy on the device
    import conflict_binding as cb, delay_binding as db, schedule_binding as sb

    def keep(tag, d):
        res.update({f"{tag}_{k}": np.asarray(v) for k, v in d.items()})

    for V_, T_, D_ in cb.SHAPES:
        for P_ in cb.PS:
            tab = cb.synthetic(P_, V_, T_)
            keep(f"conf_{P_}_{V_}_{T_}_{D_}", e.plan_conflicts(tab, D_))
            keep(f"pdel_{P_}_{V_}_{T_}_{D_}", e.plan_delays(tab, D_, slack=1))
    for name in db.CASES:
        count, clear, slack, cap, _ = db.case(name)
        keep("dsearch_" + name, e.delay_search(dict(count=count, clear=clear), slack=slack, cap=cap))
    for name in sb.CASES:
        tables, hold, length, H, slack, orders, *_ = sb.case(name)
        keep("coord_" + name, e.plan_coordination(tables, length=length))
        keep("sched_" + name, e.plan_schedule(tables, hold, horizon=H, slack=slack, orders=orders, length=length))
    pool = cb.packaged_pool()
    length = scenarios.plan_lengths(pool)
    k0p, noisep = scenarios.sample_scenarios(6, pool[1], seed=5, spec=spec)
    e.loop_init(pool, k0p, noisep, table_of=(np.arange(6) % 3).astype(np.int32))
    keep("loopconf", e.loop_plan_conflicts(40))
    keep("loopdel", e.loop_plan_delays(40, slack=1))
    keep("loopsched", e.loop_plan_schedule(hold=scenarios.hold_points(pool, 0.1, length), slack=1, length=length))
    np.savez(out, **res)
    sys.exit(0)
S = int(sys.argv[3]) if len(sys.argv) > 3 else 256
res = []
with tempfile.TemporaryDirectory() as d:
    for i, lib in enumerate(sys.argv[1:3]):
        out = os.path.join(d, f"r{i}.npz")
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", os.path.abspath(lib), str(S), out])
        res.append(dict(np.load(out)))
a, b = res
differ = 0
print(f"{4 * S} cold solves: iterations {int(a['iters'].sum())} / {int(b['iters'].sum())}, kernel {float(a['ms']):.2f} / {float(b['ms']):.2f} ms")
for k in a:
    if k == "ms" or k.endswith("_its"):
        continue
    same = np.array_equal(a[k], b[k])
    differ += not same
    print(f"  {k}: {'equal bit for bit' if same else 'DIFFERENT: %d entries, max %.3e' % (int((a[k] != b[k]).sum()), float(np.abs(a[k].astype(float) - b[k].astype(float)).max()))}")
for k in a:
    if k.endswith("_its"):
        print(f"{k[:-4]}: IPM iterations {int(a[k])} / {int(b[k])}")
        differ += int(a[k]) != int(b[k])
only_b = sorted(k for k in b if k not in a)
if only_b:
    print(f"only in the second build, not compared: {len(only_b)} keys ({', '.join(sorted({k.split('_')[0] for k in only_b}))})")
print("closed loop iterations", int(a["loop_its"]), int(b["loop_its"]))
print(f"{sum(k in b for k in a)} arrays compared")
print("ALL EQUAL" if not differ else f"{differ} DIFFERENCES")
sys.exit(1 if differ else 0)
