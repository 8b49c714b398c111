"""One handle through a sequence of closed loops whose device buffers grow from nothing, shrink, grow again and go: every stage equals,
bit for bit (loop_get and loop_history; stage 2 loop_audit as well), a fresh engine that has not been through the stages before it.

  1  loop_init with S = 1, a record of 1 step, loop_run(1)
  2  loop_init with S = 3 on the same handle; the sequential order, the disturbance, the lossy exchange with max_age 3, the problem pool
     and the map pool; a record of 4 steps, loop_run(4): queue, scratch, record, ring and pool all grow from nothing
  3  still S = 3: loop_set_comm with max_age 1, then 5 (the ring shrinks, then grows), loop_record(0), then loop_record(2), loop_run(2).
     Its fresh engine repeats stage 2 (stage 3 continues that loop) and then takes the settings' last values directly: max_age 5 and a
     record of 2, no shrinking ring and no dropped record on the way
  4  loop_init with S = 1 again: every setting is back at its default, loop_run(1) equals stage 1
  5  close(); a second close() is harmless, and a new engine works afterwards"""
import numpy as np
import pytest

import loop_cases as lc
from disturbance_binding import SIGMA
from map_pool_binding import maps
from problem_pool_binding import problems

pytestmark = pytest.mark.gpu
V = 4
SEED = 2024


def _engine():
    from conflict_rez_amd import engine, scenarios

    return engine.Engine(scenarios.parking_lot_spec(), max_batch=3 * V)


def _out(eng, audit=False):
    out = {**eng.loop_get(), **{"rec_" + k: v for k, v in eng.loop_history().items()}}
    if audit:
        out.update({"audit_" + k: v for k, v in eng.loop_audit().items()})
    return out


def _stage1(eng):
    eng.loop_init(*lc.planned(eng, 1))
    eng.loop_record(1)
    eng.loop_run(1)
    return _out(eng)


def _stage2(eng):
    S = 3
    eng.loop_init(*lc.planned(eng, S))
    eng.loop_set_order(lc.orders(S, V, 5))
    eng.loop_set_disturbance(SEED, **SIGMA)
    eng.loop_set_comm(SEED + 1, 0.3, max_age=3)
    eng.loop_set_problems(problems(eng.spec), np.arange(S) % 4)
    eng.loop_set_maps(maps(eng.spec), (np.arange(S) + 1) % 4)
    eng.loop_record(4)
    eng.loop_run(4)
    return _out(eng, audit=True)


def _stage3(eng, direct):
    if not direct:
        eng.loop_set_comm(SEED + 1, 0.3, max_age=1)
    eng.loop_set_comm(SEED + 1, 0.3, max_age=5)
    if not direct:
        eng.loop_record(0)
    eng.loop_record(2)
    eng.loop_run(2)
    return _out(eng)


@pytest.fixture(scope="module")
def reused():
    """The stages on one handle -> {stage: its arrays}, 5: what a new engine gives after the handle is closed twice."""
    eng = _engine()
    got = {1: _stage1(eng), 2: _stage2(eng), 3: _stage3(eng, direct=False), 4: _stage1(eng)}
    eng.close()
    eng.close()
    after = _engine()
    got[5] = _stage1(after)
    after.close()
    return got


@pytest.fixture(scope="module")
def fresh():
    """Every stage on an engine of its own (3: after stage 2, whose loop it continues, with the last settings taken directly)."""
    want = {}
    eng = _engine()
    want[1] = _stage1(eng)
    eng.close()
    eng = _engine()
    want[2] = _stage2(eng)
    want[3] = _stage3(eng, direct=True)
    eng.close()
    return want


@pytest.mark.parametrize("stage", (1, 2, 3))
def test_stage_equals_a_fresh_engine(reused, fresh, stage):
    assert reused[stage].keys() == fresh[stage].keys() and ("audit_clear" in fresh[stage]) == (stage == 2)
    assert fresh[stage]["rec_traj"].shape[:2] == {1: (1, 1), 2: (4, 3), 3: (2, 3)}[stage]
    lc.same(reused[stage], fresh[stage], f"stage {stage}")


def test_settings_matter(fresh):
    """The comparisons are not between runs that the settings left alone: stage 2 is not the plain loop."""
    eng = _engine()
    eng.loop_init(*lc.planned(eng, 3))
    eng.loop_run(4)
    plain = eng.loop_get()
    eng.close()
    assert not np.array_equal(plain["state"], fresh[2]["state"])


def test_init_restores_every_default(reused, fresh):
    lc.same(reused[4], fresh[1], "stage 4: S = 1 again after every setting")
    lc.same(reused[4], reused[1], "stage 4 against stage 1 of the same handle")


def test_close_twice_then_a_new_engine(reused, fresh):
    lc.same(reused[5], fresh[1], "stage 5: a new engine after the handle is gone")
