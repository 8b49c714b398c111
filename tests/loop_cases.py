"""What the GPU tests of the closed loop's settings (exchange order, disturbances, lossy exchange, problem pool, map pool) share: the
planned workload, seeded exchange orders, one closed loop run stepwise or in persistent launches, the bit-for-bit comparison of two
runs, the comparison of a device run with the host replay, and the cases every per-scenario pool setting (`Pool`) has, which the pool
modules call from their own test functions (tests/test_loop_cases_host.py runs them against a stand-in engine with defects).
Not a test module and not a conftest: the modules import what they use; their fixtures stay with them."""
import dataclasses
from typing import Callable

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


def run(eng, init, K, how, order=None, setup=None, between=None, record=True, at=None):
    """One closed loop of K steps from `init`, the arguments of loop_init or (arguments, keyword arguments): how = "step", "run" or a
    tuple of run lengths; `setup` is called with the engine after loop_init, `between` between the launches (how a tuple) or before
    step `at` (how = "step").  -> loop_get's dict with the record's arrays as rec_*."""
    args, kw = init if len(init) == 2 and isinstance(init[1], dict) else (init, {})
    eng.loop_init(*args, **kw)
    if order is not None:
        eng.loop_set_order(order)
    if setup is not None:
        setup(eng)
    if record:
        eng.loop_record(K)
    if how == "step":
        for t in range(K):
            if between is not None and t == at:
                between(eng)
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


def stepwise(eng, K):
    """K x loop_step -> loop_get's dict after every step."""
    out = []
    for _ in range(K):
        eng.loop_step()
        out.append(eng.loop_get())
    return out


def rows(a, sel):
    """The scenarios `sel` of every array of a run."""
    return {k: (v[:, sel] if k.startswith("rec_") else v[sel]) for k, v in a.items()}


def same(a, b, what, rows=None):
    """Every array of a (rows: its scenarios `rows`) equals b's, bit for bit."""
    for k in a:
        x = a[k] if rows is None else (a[k][:, rows] if k.startswith("rec_") else a[k][rows])
        assert np.array_equal(x, b[k]), (what, k)


def goals(table, S):
    """[S, V, 3] goal poses: every scenario's are the last sample of the table."""
    return np.broadcast_to(table[:, -1, :3], (S,) + table[:, -1, :3].shape).copy()


def against_replay(got, ref, what=None):
    """A device run against the host replay, step for step.  got: loop_get's dict after every step, or loop_history's dict; ref: what
    `oracle.closed_loop.replay` yields.  Status and iterations are equal at every step (asserted here).
    -> (largest |state - replay| over the run, number of replayed solves that converged): the caller asserts its own bounds on both."""
    worst, n_conv = 0.0, 0
    for t, (state, _, status, iters) in enumerate(ref):
        g = {"state": got["traj"][t][..., :5], "status": got["status"][t], "iters": got["iters"][t]} if isinstance(got, dict) else got[t]
        assert np.array_equal(g["status"], status) and np.array_equal(g["iters"], iters), (what, t)
        worst = max(worst, float(np.abs(g["state"] - state).max()))
        n_conv += int((status == 0).sum())
    return worst, n_conv


def noise_and_loss(sigma, stream, seed=2024):
    """setup: the base disturbance and a lossy exchange (p_drop 0.3, max_age 3, compensated) on the stream ids `stream`."""
    def f(e):
        e.loop_set_disturbance(seed, stream=stream, **sigma)
        e.loop_set_comm(seed + 1, 0.3, max_age=3, compensate=True, stream=stream)
    return f


@dataclasses.dataclass(frozen=True)
class Pool:
    """A per-scenario pool setting of the closed loop (entries and a mapping scenario -> entry), as the cases below and the fixtures need it."""
    set: Callable      # set(eng, entries, mapping): the pool with its mapping [S]
    off: Callable      # off(eng): the setting switched off
    own: Callable      # own(eng) -> the entry that is the handle's own
    entries: Callable  # entries(spec) -> the four test entries [A, B, C, D] over the handle's spec; A is the handle's own
    plain: Callable    # plain(spec, entry, max_batch) -> a plain engine created on that entry: the code path without the setting
    names: str         # the entries' names


def off_is_off(pool, eng, init, K, how, order, under=None):
    """No call, a pool of one with the handle's own entry, three identical copies under a random mapping, and set-then-unset give equal
    state, prediction, status, iterations and record, bit for bit; under(eng) makes another setting first in every run.
    -> the run without a call."""
    S = len(init[1])
    of3 = np.random.default_rng(4).integers(0, 3, S)
    assert len(set(of3)) == 3
    then = lambda f: f if under is None else (lambda e: (under(e), f(e)))

    def set_unset(e):
        pool.set(e, pool.entries(e.spec), np.arange(S) % 4)
        pool.off(e)

    plain = run(eng, init, K, how, order, under)
    same(plain, run(eng, init, K, how, order, then(lambda e: pool.set(e, [pool.own(e)], np.zeros(S, int)))), "a pool of one, the handle's own")
    same(plain, run(eng, init, K, how, order, then(lambda e: pool.set(e, [pool.own(e)] * 3, of3))), "three identical copies")
    same(plain, run(eng, init, K, how, order, then(set_unset)), "set, then unset")
    return plain


def mixed_batch_equals_separate_handles(pool, eng, entries, plain_engines, init, K, order, settings):
    """mapping[s] = s % 4, stepped, in one launch and in a split launch (3, K - 3): the rows of entry p equal, bit for bit, what
    plain_engines[p], created on that entry, gives for p's scenarios alone; settings(stream) -> the setup of further settings on the
    stream ids of the (sub-)batch, or None.  -> {how: the mixed run}."""
    table, k0, noise = init
    S = len(k0)
    of = np.arange(S) % 4

    def mixed_setup(e):
        (settings(np.arange(S)) or (lambda e: None))(e)
        pool.set(e, entries, of)

    out = {}
    for how in ("step", "run", (3, K - 3)):
        out[how] = mixed = run(eng, init, K, how, order, mixed_setup)
        for p, pe in enumerate(plain_engines):
            sel = np.flatnonzero(of == p)
            alone = run(pe, (table, k0[sel], noise[sel]), K, how, None if order is None else order[sel], settings(sel))
            same(rows(mixed, sel), alone, (how, pool.names[p]))
    return out


def mapping_changes_between_calls(pool, eng, entries, init, K, order):
    """loop_run(3), another mapping, loop_run(K - 3) equals the same sequence stepped, bit for bit; the change matters."""
    S = len(init[1])
    first = lambda e: pool.set(e, entries, np.arange(S) % 4)
    change = lambda e: pool.set(e, entries, (np.arange(S) + 1) % 4)
    ran = run(eng, init, K, (3, K - 3), order, first, change)
    same(ran, run(eng, init, K, "step", order, first, change, at=3), "run / remap / run against the same sequence stepped")
    kept = run(eng, init, K, (3, K - 3), order, first)
    assert np.array_equal(kept["rec_traj"][:3], ran["rec_traj"][:3]) and not np.array_equal(kept["state"], ran["state"])


def refusals_change_nothing(pool, eng, entries, init, K, refused, rest):
    """loop_init, the pool under mapping[s] = s % 4, loop_run(2), then refused(eng), the module's refused calls: the loop's state is
    unchanged; the launches `rest` (run lengths, or "step") that complete the K steps give the bits of the same launches without the
    refused calls and of one launch of K steps, so the setting in force stayed; loop_init switches the setting off."""
    S = len(init[1])
    on = lambda e: pool.set(e, entries, np.arange(S) % 4)

    def start_and_finish(between=None):
        eng.loop_init(*init)
        on(eng)
        eng.loop_run(2)
        before = eng.loop_get()
        if between is not None:
            between(eng)
            same(before, eng.loop_get(), "state after the refusals")
        for k in rest:
            if k == "step":
                eng.loop_step()
            else:
                eng.loop_run(k)
        return eng.loop_get()

    end = start_and_finish(refused)
    same(end, start_and_finish(), "the setting in force stayed: the same launches without the refused calls")
    ref = run(eng, init, K, "run", None, on)
    same(end, {k: ref[k] for k in end}, "the setting in force stayed: one launch")
    eng.loop_init(*init)
    eng.loop_run(K)
    off = eng.loop_get()
    assert not np.array_equal(off["state"], end["state"])
    plain = run(eng, init, K, "run")
    same(off, {k: plain[k] for k in off}, "loop_init switches the setting off")
