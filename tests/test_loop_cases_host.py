"""tests/loop_cases.py without a GPU: the cases shared by the pool modules pass on a stand-in engine (a few lines of deterministic
arithmetic behind the loop_* methods the cases call) and raise AssertionError when the stand-in is given the defect the case is there
to find.  This tests the cases, not the product."""
import types

import numpy as np
import pytest

import loop_cases as lc

S, K, V = 8, 6, 4


class StandIn:
    """Scenario s, step t: x <- 0.9 x + 0.01 (t + 1) c + what the order and the streams of the noise and of the lossy exchange add, c the
    scenario's pool entry (a number) or the handle's own.  `defect`: "residue", "split", "neighbour" or "remap" (below)."""

    def __init__(self, own=1.0, defect=None):
        self.spec, self.defect = types.SimpleNamespace(n_nbr=V - 1, own=own), defect

    def loop_init(self, table, k0, noise):
        self.x = table[:, 0, :5] + noise + k0[:, None, None]  # [S, V, 5]
        self.t, self.order, self.pool, self.streams, self.rec, self.residue = 0, None, None, {}, None, 0.0
        self.status = self.iters = np.zeros(self.x.shape[:2], int)

    def loop_set_order(self, order):
        self.order = np.asarray(order)

    def loop_set_disturbance(self, seed, stream=None, **sigma):
        self.streams["noise"] = (seed, np.arange(len(self.x)) if stream is None else np.asarray(stream))

    def loop_set_comm(self, seed, p_drop, max_age=1, compensate=False, stream=None):
        self.streams["comm"] = (seed + p_drop, np.arange(len(self.x)) if stream is None else np.asarray(stream))

    def set_pool(self, entries, mapping):
        if self.defect == "remap" and self.pool is not None and self.t > 0:
            return  # a mapping change between launches is ignored
        self.pool = np.asarray(entries, float)[np.asarray(mapping)]

    def unset_pool(self):
        self.pool, self.residue = None, 1e-9 if self.defect == "residue" else 0.0  # unset leaves a residue

    def loop_record(self, K):
        self.rec = []

    def _step(self, first_of_a_later_launch=False):
        c = np.full(len(self.x), self.spec.own) if self.pool is None else self.pool.copy()
        if self.pool is not None and self.defect == "neighbour":
            c += 1e-6 * np.roll(self.pool, 1)  # a scenario's result depends on another scenario's entry
        if self.pool is not None and self.defect == "split" and first_of_a_later_launch:
            c += 1e-6  # a split launch differs from a single one
        add = 0.01 * (self.t + 1) * (c + self.residue)
        if self.order is not None:
            add = add + 1e-3 * (self.order * np.arange(V)).sum(1)
        for seed, stream in self.streams.values():
            add = add + 1e-3 * np.sin(seed + 7.0 * stream + self.t)
        self.x = 0.9 * self.x + add[:, None, None]
        self.iters = (np.abs(self.x[..., 0]) * 1e3).astype(int) % 50
        self.status = self.iters % 2
        self.t += 1
        if self.rec is not None:
            self.rec.append((np.concatenate([self.x, self.x[..., :2]], -1), self.status, self.iters))

    def loop_step(self):
        self._step()

    def loop_run(self, k):
        for i in range(k):
            self._step(i == 0 and self.t > 0)

    def loop_get(self):
        return dict(state=self.x.copy(), pred=np.repeat(self.x[..., None], 2, -1), status=self.status.copy(), iters=self.iters.copy())

    def loop_history(self):
        return {k: np.stack(v) for k, v in zip(("traj", "status", "iters"), zip(*self.rec))}


POOL = lc.Pool(set=lambda e, entries, mapping: e.set_pool(entries, mapping), off=lambda e: e.unset_pool(), own=lambda e: e.spec.own,
               entries=lambda spec: [spec.own, 2.0, 3.0, 5.0], plain=lambda spec, entry, max_batch: StandIn(entry), names="ABCD")


def _init():
    rng = np.random.default_rng(0)
    return rng.normal(size=(V, 30, 7)), rng.integers(0, 20, S), 0.01 * rng.normal(size=(S, V, 5))


def _cases(defect):
    """name -> the shared case as a call without arguments, on a stand-in engine with `defect`."""
    eng, init, order = StandIn(defect=defect), _init(), lc.orders(S, V, 11)
    entries = POOL.entries(eng.spec)
    plain_engines = [POOL.plain(eng.spec, c, S * V) for c in entries]
    lossy = lambda e: e.loop_set_comm(7, 0.3, max_age=3, compensate=True)
    noisy = lambda stream: lc.noise_and_loss(dict(meas=[0.1]), stream)
    return {
        "off_is_off": lambda: [lc.off_is_off(POOL, eng, init, K, how, o, under) for how in ("step", "run") for o in (None, order) for under in (None, lossy)],
        "mixed_batch": lambda: [lc.mixed_batch_equals_separate_handles(POOL, eng, entries, plain_engines, init, K, o, st) for o in (None, order) for st in (lambda stream: None, noisy)],
        "mapping_changes": lambda: [lc.mapping_changes_between_calls(POOL, eng, entries, init, K, o) for o in (None, order)],
        "refusals": lambda: [lc.refusals_change_nothing(POOL, eng, entries, init, 4, lambda e: None, rest) for rest in ((2,), ("step", 1))],
    }


def test_the_shared_cases_pass_on_a_sound_stand_in():
    """Every shared case passes, and the stand-in is a workload on which they can fail: entries, orders and streams all move the state."""
    for case in _cases(None).values():
        case()
    eng, init = StandIn(), _init()
    base = lc.run(eng, init, K, "run")["state"]
    for what, kw in (("pool", dict(setup=lambda e: e.set_pool([1.0, 2.0], np.arange(S) % 2))), ("order", dict(order=lc.orders(S, V, 11))),
                     ("streams", dict(setup=lc.noise_and_loss({}, np.arange(S))))):
        assert not np.array_equal(base, lc.run(eng, init, K, "run", **kw)["state"]), what


@pytest.mark.parametrize("defect,found_by", [("residue", "off_is_off"), ("split", "mixed_batch"), ("split", "refusals"), ("neighbour", "mixed_batch"),
                                             ("remap", "mapping_changes")])
def test_a_defect_makes_its_case_fail(defect, found_by):
    """residue: unset leaves something behind; split: a split launch differs from a single one; neighbour: a scenario's result depends on
    another scenario's pool entry; remap: a mapping change between launches is ignored."""
    with pytest.raises(AssertionError):
        _cases(defect)[found_by]()


def test_against_replay():
    """Both forms of the device results give the same figures; a status or an iteration count that differs fails with its step."""
    eng, init = StandIn(), _init()
    eng.loop_init(*init)
    eng.loop_record(K)
    got = []
    for _ in range(K):
        eng.loop_step()
        got.append(eng.loop_get())
    h = eng.loop_history()
    ref = [(g["state"] + 1e-9 * (t == 2), None, g["status"], g["iters"]) for t, g in enumerate(got)]
    worst, n_conv = lc.against_replay(got, iter(ref))
    assert (worst, n_conv) == lc.against_replay(h, iter(ref)) and 0.5e-9 < worst < 2e-9
    assert n_conv == sum(int((g["status"] == 0).sum()) for g in got) and 0 < n_conv < K * S * V
    for k in (2, 3):  # status, iterations
        bad = [r[:k] + (r[k] + (t == 4),) + r[k + 1 :] for t, r in enumerate(ref)]
        for device in (got, h):
            with pytest.raises(AssertionError, match=r"\(None, 4\)"):
                lc.against_replay(device, iter(bad))
