"""The lossy prediction exchange of the closed loop (conflict_rez_amd/csrc/cfz_comm.inl) on the host: the CPU build of the kernel source
(tests/emu/cfz_comm_emu.cpp) against the numpy statement of the delivery bits and the plain-Python age rule of tests/comm_binding.py,
and oracle/closed_loop.replay under that file's settings: against itself where nothing is lost, against a recorded run where much is."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import comm_binding as cb  # noqa: E402


def test_delivery_bits_against_the_numpy_statement():
    """10^4 random (seed, stream, receiver, sender, tau, p), the corners included (tau + 1 = 0 and 2^31 - 1 in word 2, stream ids 0 and
    2^32 - 1): bits equal (u1 is an exact 53-bit value: an equality), counters equal, word 3 in 8..15: never a noise pair 0..5."""
    rng = np.random.default_rng(11)
    n = 10_000
    seed = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    stream = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    v, u = rng.integers(0, 8, n), rng.integers(0, 8, n)
    tau = rng.integers(0, 2 ** 31 - 1, n)
    tau[: n // 2] = rng.integers(0, 64, n // 2)
    p = rng.random(n)
    seed[0], stream[0], tau[0] = 0, 0, -1
    seed[1], stream[1], tau[1] = 2 ** 64 - 1, 2 ** 32 - 1, 2 ** 31 - 2
    bit, ctr = cb.emu_delivered(seed, stream, v, u, tau, p)
    assert np.array_equal(bit, cb.delivered_bits(seed, stream, v, u, tau, p))
    assert np.array_equal(ctr, cb.counters(stream, v, u, tau).astype(np.uint32))
    assert np.array_equal(ctr[:, 2].astype(np.int64), tau + 1) and np.array_equal(ctr[:, 1], v) and np.array_equal(ctr[:, 0], stream)
    assert ctr[:, 3].min() >= 8 and ctr[:, 3].max() <= 15
    assert 0.3 < bit.mean() < 0.7
    # a bit is u1 > p at that draw's own u1: equal just below, not at it
    u1 = cb.u1_of(seed, stream, v, u, tau)
    assert (u1 > 0).all() and (u1 <= 1).all()
    at, _ = cb.emu_delivered(seed, stream, v, u, tau, u1)
    below, _ = cb.emu_delivered(seed, stream, v, u, tau, np.nextafter(u1, 0))
    assert not at.any() and below.all()
    # the batch form of the export, message tau + 1 of a window is message tau of the next
    pd, st = np.array([0.0, 0.3, 0.3, 1.0]), np.array([4, 4, 2 ** 32 - 1, 0], np.uint32)
    full = cb.emu_comm(77, pd, st, 4, 0, 9)
    assert np.array_equal(full, cb.delivered(77, pd, st, 4, 0, 9)) and np.array_equal(full[3:], cb.emu_comm(77, pd, st, 4, 3, 6))
    assert full[:, :, np.arange(4), np.arange(4)].all()


def test_extreme_rates_and_frequencies():
    """p = 0 delivers everything and p = 1 nothing; at p = 0.1 and 0.5 the drop frequency of 10^5 draws lies within five binomial standard
    deviations."""
    n = 100_000
    rng = np.random.default_rng(5)
    stream = np.repeat(np.arange(1000, dtype=np.uint32), 100)
    tau = np.tile(np.arange(100), 1000)
    v, u = rng.integers(0, 4, n), rng.integers(0, 4, n)
    seed = np.full(n, 2024, np.uint64)
    assert cb.emu_delivered(seed, stream, v, u, tau, 0.0)[0].all()
    assert not cb.emu_delivered(seed, stream, v, u, tau, 1.0)[0].any()
    for p in (0.1, 0.5):
        drop = 1.0 - cb.emu_delivered(seed, stream, v, u, tau, p)[0].mean()
        sd = np.sqrt(p * (1 - p) / n)
        print(f"p = {p}: drop frequency {drop:.5f}, {abs(drop - p) / sd:.2f} standard deviations off")
        assert abs(drop - p) <= 5 * sd


@pytest.mark.parametrize("max_age", range(1, cb.MAX_AGE + 1))
def test_age_rule(max_age):
    """The CPU build's age over random bit arrays equals the plain-Python rule, for both wants (t - 1, and t of an earlier rank), with
    history starting 0 .. max_age + 2 messages back; the cap (nothing delivered: min(max_age, tau* - tau_on)) and age 0 are among them."""
    assert cb.lib().cfz_emu_max_age() == cb.MAX_AGE
    rng = np.random.default_rng(max_age)
    base, n = 3, 24  # bits[i] is message base + i
    seen = set()
    for trial in range(400):
        bits = rng.random(n) < (0.0, 0.3, 0.6, 1.0)[trial % 4]
        t = int(rng.integers(base + 10, base + n))
        for earlier in (False, True):
            tau_star = cb.want(t, earlier)
            assert cb.lib().cfz_emu_want(t, int(earlier)) == tau_star == t - (not earlier)
            tau_on = tau_star - int(rng.integers(0, max_age + 3))
            want = cb.age_rule(lambda tau: bool(bits[tau - base]), tau_star, max_age, tau_on)
            assert cb.emu_age(bits, base, tau_star, max_age, tau_on) == want
            assert 0 <= want <= min(max_age, tau_star - tau_on)
            if not bits.any():
                assert want == min(max_age, tau_star - tau_on)
            seen.add((want, tau_star - tau_on < max_age))
    assert {a for a, _ in seen} == set(range(max_age + 1)) and {lim for _, lim in seen} == {False, True}
    # over the loop's own draws: the same rule on the numpy bits
    pd, st = np.array([0.5, 0.8]), np.array([9, 2 ** 32 - 1], np.uint32)
    bits = cb.delivered(31, pd, st, 4, 0, 30)
    for s, v, u, tau_star, tau_on in ((0, 1, 2, 20, -1), (1, 3, 0, 29, 27), (1, 0, 3, 12, 12), (0, 2, 1, 7, 0)):
        want = cb.age_rule(lambda tau: bool(bits[tau, s, v, u]), tau_star, max_age, tau_on)
        assert cb.emu_age_drawn(31, pd, st, max_age, tau_on, s, v, u, tau_star) == want


def test_row_and_slot():
    """The read row is k + fresh + (compensate ? a : 0), clamped at N - 1; D = max_age + 2 consecutive messages take D different slots
    and message -1 (the seed) has slot 0."""
    for N in (2, 5, 20):
        for fresh in (0, 1):
            for comp in (0, 1):
                for a in range(cb.MAX_AGE + 1):
                    got = [cb.lib().cfz_emu_row(k, fresh, comp, a, N) for k in range(N)]
                    assert got == cb.rows(N, fresh, comp, a).tolist() == [min(k + fresh + comp * a, N - 1) for k in range(N)]
                    assert got[-1] == N - 1 and max(got) == N - 1
    for max_age in range(1, cb.MAX_AGE + 1):
        D = max_age + 2
        assert cb.lib().cfz_emu_slot(-1, max_age) == 0
        for t in range(max_age + 1, 40):  # (messages from -1 on)
            assert len({cb.lib().cfz_emu_slot(tau, max_age) for tau in range(t - 1 - max_age, t + 1)}) == D
            assert cb.lib().cfz_emu_slot(t, max_age) == cb.lib().cfz_emu_slot(t - D, max_age)


@pytest.mark.parametrize("exchange", ["jacobi", "sequential"])
def test_replay_without_loss_is_the_oracle_replay(ospec, exchange):
    """1 scenario x 3 steps: oracle/closed_loop.replay with history under p = 0 (every bit set) and under a `comm` that never gives a
    setting equals the replay with comm=None: state, prediction, status and iterations, exactly."""
    from conflict_rez_amd import scenarios
    from oracle.closed_loop import replay

    spec = scenarios.parking_lot_spec()
    table, _ = scenarios.load_reference_table(kind="planned")
    k0, noise = scenarios.sample_scenarios(1, table, seed=3, spec=spec)
    V, steps = table.shape[0], 3
    order = np.array([[2, 0, 3, 1]]) if exchange == "sequential" else None
    ref = list(replay(ospec, table, k0, noise, steps, dt=spec.dt, wb=spec.wb, order=order))
    every = cb.Setting(3, True, -1, bits=np.ones((steps, 1, V, V), bool))
    for comm in (lambda t: None, lambda t: every):
        ages = []
        got = list(replay(ospec, table, k0, noise, steps, dt=spec.dt, wb=spec.wb, order=order, comm=comm, ages=ages))
        for t in range(steps):
            for a, b in zip(ref[t], got[t]):
                assert np.array_equal(a, b), (exchange, t)
        assert all(a == 0 for *_, a in ages)
    assert sum(int((r[2] == 0).sum()) for r in ref) >= steps * V // 2


# ---- the recorded lossy replay (tests/golden/comm_replay_lossy.npz; tests/golden/make_fixtures.py: comm_replay_lossy) ------------------
LOSSY_CASES = (("jacobi", False, False), ("jacobi_comp", False, True), ("sequential", True, False), ("sequential_comp_d", True, True))


def lossy_replay_runs(ospec, replay):
    """The fixture's runs through `replay` (oracle.closed_loop.replay's signature): 2 scenarios x 4 steps at p_drop 0.5, max_age 2, both
    exchange rules x both `compensate` values, the last one under a disturbance d.  {name_key: array}, the ages as rows (t, s, v, u, a)."""
    from conflict_rez_amd import scenarios

    spec = scenarios.parking_lot_spec()
    table, _ = scenarios.load_reference_table(kind="planned")
    S, steps, V = 2, 4, table.shape[0]
    k0, noise = scenarios.sample_scenarios(S, table, seed=3, spec=spec)
    bits = cb.delivered(2024, np.full(S, 0.5), np.array([7, 2 ** 32 - 1], np.uint32), V, 0, steps)
    box = np.asarray(spec.bounds, float).reshape(6, 2)[4:6]
    sigma = np.array([0.02, 0.02, 0.005, 0.02, 0.002, 0.3, 0.1, 0.01, 0.01, 0.002, 0.01, 0.001])
    out = {"k0": np.asarray(k0), "noise": np.asarray(noise)}
    for name, sequential, compensate in LOSSY_CASES:
        setting = cb.Setting(2, compensate, -1, bits=bits)
        order = np.array([[2, 0, 3, 1], [1, 3, 0, 2]]) if sequential else None
        d = np.random.default_rng(9).normal(0.0, 1.0, (steps, S, V, 12)) * sigma if name.endswith("_d") else None
        ages = []
        run = list(replay(ospec, table, k0, noise, steps, dt=spec.dt, wb=spec.wb, order=order, d=d, box=box, comm=lambda t: setting, ages=ages))
        for i, key in enumerate(("state", "pred", "status", "iters")):
            out[f"{name}_{key}"] = np.stack([r[i] for r in run])
        out[f"{name}_ages"] = np.array(ages, np.int64)
    return out


def test_lossy_replay_reproduces_the_recorded_one(ospec):
    """oracle/closed_loop.replay under loss against the run recorded with the replay-with-history this module's binding used to carry
    (before the two host loops became one): state, prediction, status, iterations and every age read, bit for bit.  The record is
    worth comparing with: some message is read at an age above 0 and at least half of the solves converge."""
    from oracle.closed_loop import replay

    want = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "comm_replay_lossy.npz"))
    got = lossy_replay_runs(ospec, replay)
    assert sorted(got) == sorted(want.files)
    for key in want.files:
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key
    for name, *_ in LOSSY_CASES:
        assert (want[f"{name}_ages"][:, 4] > 0).any(), name
        assert 2 * int((want[f"{name}_status"] == 0).sum()) >= want[f"{name}_status"].size, name
