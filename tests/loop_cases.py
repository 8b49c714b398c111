"""What the GPU tests of the closed loop's settings (exchange order, disturbances, lossy exchange, problem pool) share: the planned
workload, seeded exchange orders, one closed loop run stepwise or in persistent launches, and the bit-for-bit comparison of two runs.
Not a test module and not a conftest: the modules import what they use; their fixtures stay with them."""
import numpy as np


def planned(eng, S, seed=2024):
    """(table, k0, noise) of S scenarios on the planned reference table: the arguments of loop_init."""
    from conflict_rez_amd import scenarios

    table, _ = scenarios.load_reference_table(kind="planned")
    k0, noise = scenarios.sample_scenarios(S, table, seed=seed, spec=eng.spec)
    return table, k0, noise


def orders(S, V, seed):
    """Seeded per-scenario orders; scenario 0 the identity, scenario 1 the reversed order."""
    rng = np.random.default_rng(seed)
    o = np.stack([rng.permutation(V) for _ in range(S)]).astype(np.int32)
    o[0], o[1] = np.arange(V), np.arange(V)[::-1]
    return o


def run(eng, init, K, how, order=None, setup=None, between=None, record=True):
    """One closed loop of K steps from `init`, the arguments of loop_init or (arguments, keyword arguments): how = "step", "run" or a
    tuple of run lengths; `setup` is called with the engine after loop_init, `between` (how a tuple) between the launches.
    -> loop_get's dict with the record's arrays as rec_*."""
    args, kw = init if len(init) == 2 and isinstance(init[1], dict) else (init, {})
    eng.loop_init(*args, **kw)
    if order is not None:
        eng.loop_set_order(order)
    if setup is not None:
        setup(eng)
    if record:
        eng.loop_record(K)
    if how == "step":
        for _ in range(K):
            eng.loop_step()
    else:
        for i, k in enumerate((K,) if how == "run" else how):
            if i and between is not None:
                between(eng)
            eng.loop_run(k)
    out = eng.loop_get()
    if record:
        out.update({"rec_" + k: v for k, v in eng.loop_history().items()})
    return out


def same(a, b, what, rows=None):
    """Every array of a (rows: its scenarios `rows`) equals b's, bit for bit."""
    for k in a:
        x = a[k] if rows is None else (a[k][:, rows] if k.startswith("rec_") else a[k][rows])
        assert np.array_equal(x, b[k]), (what, k)
