"""The closed-loop score on the host: the CPU build of the kernel source (csrc/cfz_score.inl through tests/emu/cfz_score_emu.cpp)
against an independent numpy statement of its definitions, its ordered merges at every lane count, known answers, and the argument
handling of the Python layer and the C entry points (which refuse on the host, before any launch)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audit_binding as ab  # noqa: E402
import score_binding as sb  # noqa: E402

ICNT = {n: i for i, n in enumerate(sb.CNT)}
IVAL = {n: i for i, n in enumerate(sb.VAL)}


def _emu(d, **kw):
    return sb.emu_score(d["traj"], d["status"], d["iters"], d["tables"], d["table_of"], d["k0"], **kw)


@pytest.mark.parametrize("V", sb.VS)
def test_cpu_build_matches_the_numpy_statement(V):
    """Every K at the kernel's lane grouping: empty lanes (K < L), K = L, K = L + 1, a ragged last chunk, upto inside a chunk."""
    for K in sb.KS:
        d, ref = sb.synthetic(V, K), sb.synthetic_reference(V, K)
        sb.check_against_statement(_emu(d), ref)
        # the data are what the docstring of synthetic() promises
        c = ref["cnt"]
        assert c[0, 0, ICNT["arrive"]] == 0 and c[1, 0, ICNT["arrive"]] == K - 1 and c[0, 0, ICNT["steps"]] == 1
        if V > 1:
            assert c[2, 0, ICNT["arrive"]] == -1 and c[2, 0, ICNT["steps"]] == K and c[2, V - 1, ICNT["arrive"]] == K // 2
            assert c[0, V - 1, ICNT["failed"]] == c[0, V - 1, ICNT["fail_run"]] == c[0, V - 1, ICNT["steps"]]
            assert c[1, V - 1, ICNT["failed"]] == 0
            if K >= 7:
                assert c[1, 0, ICNT["near_steps"]] > 0 and c[1, 1, ICNT["near_steps"]] > 0
        if K >= 37:
            assert c[..., ICNT["reversals"]].max() > 0 and c[..., ICNT["waiting"]].max() > 0


def test_every_lane_count_gives_the_same_integers():
    """1, 2, 4, ..., 64 lanes per vehicle: the ordered merges do not depend on where the chunks are cut; the sums only in the last bits."""
    for V, K in ((1, 130), (3, 37), (4, 17), (8, 9), (2, 1)):
        d = sb.synthetic(V, K)
        one = _emu(d, lanes=1)
        sb.check_against_statement(one, sb.synthetic_reference(V, K))
        for L in (2, 4, 8, 16, 32, 64):
            out = _emu(d, lanes=L)
            assert np.array_equal(out["cnt"], one["cnt"]), (V, K, L)
            assert np.allclose(out["val"], one["val"], rtol=1e-12, atol=0.0), (V, K, L)
    assert [sb.group(V) for V in range(1, 9)] == [64, 32, 16, 16, 8, 8, 8, 8]


def _one_vehicle(v, status, lanes, v_tol=0.1):
    """cnt of one far-away vehicle with the speeds v and the status sequence given, which never arrives."""
    K = len(v)
    traj = np.zeros((K, 1, 1, 7)); traj[:, 0, 0, 3] = v
    tables = np.full((1, 1, 2, 7), 50.0)
    out = sb.emu_score(traj, np.asarray(status, np.int32).reshape(K, 1, 1), None, tables, [0], [0], lanes=lanes, v_tol=v_tol)
    return {n: int(out["cnt"][0, 0, i]) for n, i in ICNT.items()}


def test_fail_run_and_reversals_by_hand():
    """Eight steps on four lanes are chunks of two: the failed run over steps 1..5 spans three chunks, and the one change of sign,
    between steps 3 and 4, falls exactly on a chunk boundary (steps 2, 5, 6 are inside +-v_tol: waiting, and no sign)."""
    st = [0, 1, 2, 5, 1, 3, 0, 4]
    v = [1.0, 0.5, 0.05, 0.7, -0.6, -0.02, 0.03, -1.0]
    for L in (1, 2, 4, 8, 64):
        c = _one_vehicle(v, st, L)
        assert (c["failed"], c["fail_run"]) == (6, 5), L
        assert (c["reversals"], c["waiting"], c["steps"], c["arrive"]) == (1, 3, 8, -1), L
    # a vehicle creeping around zero changes no direction; one that pauses between two directions changes once
    for L in (1, 4, 8):
        assert _one_vehicle([0.05, -0.05, 0.09, -0.09, 0.0, 0.01, -0.01, 0.02], [0] * 8, L)["reversals"] == 0
        assert _one_vehicle([0.5, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -0.5], [0] * 8, L)["reversals"] == 1
        assert _one_vehicle([0.5, -0.5] * 4, [1] * 8, L)["reversals"] == 7
        c = _one_vehicle([0.5] * 8, [1, 1, 0, 1, 1, 1, 0, 1], L)
        assert (c["failed"], c["fail_run"]) == (6, 3)
        c = _one_vehicle([0.5] * 8, [1] * 8, L)
        assert (c["failed"], c["fail_run"]) == (8, 8)
        c = _one_vehicle([0.5] * 8, [0] * 8, L)
        assert (c["failed"], c["fail_run"]) == (0, 0)


def test_known_answers():
    from conflict_rez_amd import engine

    rng = np.random.default_rng(7)
    K, S, V, T = 21, 2, 3, 30
    tables = np.zeros((2, V, T, 7))
    tables[..., 0:2] = rng.uniform(3, 30, (2, V, T, 2)); tables[..., 2] = rng.uniform(-3, 3, (2, V, T)); tables[..., 3:] = rng.uniform(0.3, 1, (2, V, T, 4))
    tof, k0 = np.array([1, 0], np.int32), np.array([4, 0], np.int32)
    # following the plan exactly: the record's row t is the plan's row k0 + t + 1
    traj = np.stack([tables[tof[s]][:, k0[s] + 1 : k0[s] + 1 + K].transpose(1, 0, 2) for s in range(S)], 1)
    out = sb.emu_score(traj, None, None, tables, tof, k0)
    for n in ("dx2", "dy2", "psi2", "dev2_max"):
        assert (out["val"][..., IVAL[n]] == 0.0).all(), n
    assert (out["cnt"][..., ICNT["dev_max_step"]] == 0).all() and (out["cnt"][..., ICNT["iters_sum"]] == 0).all()
    sb.check_against_statement(out, sb.score(traj, None, None, tables, tof, k0))
    # one step off in the phase is not free
    assert (sb.emu_score(traj, None, None, tables, tof, k0 + 1)["val"][..., IVAL["dx2"]] > 0).all()
    # constant inputs
    flat = traj.copy(); flat[..., 5] = 0.7; flat[..., 6] = -0.2
    out = sb.emu_score(flat, None, None, tables, tof, k0)
    assert (out["val"][..., IVAL["da2"]] == 0.0).all() and (out["val"][..., IVAL["dw2"]] == 0.0).all()
    assert np.allclose(out["val"][..., IVAL["a2"]], 0.49 * out["cnt"][..., ICNT["steps"]], rtol=1e-13)
    # the derived values
    d = sb.synthetic(4, 37)
    out = _emu(d)
    w = np.array([100.0, 90, 80, 3, 2, 1])
    sm = engine.score_summary(out["val"], out["cnt"], 0.1, w)
    assert np.allclose(sm["cost"], out["val"][..., :6] @ w, rtol=1e-14)
    ws = np.stack([w, 2 * w, 3 * w])
    assert np.allclose(engine.score_summary(out["val"], out["cnt"], 0.1, ws)["cost"], sm["cost"] * np.array([1, 2, 3])[:, None], rtol=1e-14)
    assert np.array_equal(sm["time"], 0.1 * out["cnt"][..., 0]) and np.array_equal(sm["wait"], 0.1 * out["cnt"][..., ICNT["waiting"]])
    assert np.array_equal(sm["distance"], 0.1 * out["val"][..., IVAL["absv"]])
    assert np.allclose(sm["track_max"] ** 2, out["val"][..., IVAL["dev2_max"]]) and (sm["track_rms"] <= sm["track_max"] * (1 + 1e-15)).all()
    for i, n in enumerate(sb.VAL):
        assert np.array_equal(sm[n], out["val"][..., i])
    for i, n in enumerate(sb.CNT):
        assert np.array_equal(sm[n], out["cnt"][..., i])
    assert engine.SCORE_VAL == sb.VAL and engine.SCORE_CNT == sb.CNT
    # the arrival is the audit's
    for V, K in ((4, 37), (8, 16), (1, 9)):
        d = sb.synthetic(V, K)
        goal = d["tables"][d["table_of"], :, -1, :3]
        assert np.array_equal(_emu(d)["cnt"][..., ICNT["arrive"]], ab.audit(d["traj"], goal, [], sb.G, **sb.TOL)["arrive"])


def test_python_arguments():
    from conflict_rez_amd import engine

    val, cnt = np.zeros((2, 3, 10)), np.ones((2, 3, 11), np.int32)
    with pytest.raises(ValueError, match="weights"):
        engine.score_summary(val, cnt, 0.1, np.ones(5))
    with pytest.raises(ValueError, match="weights"):
        engine.score_summary(val, cnt, 0.1, np.ones((3, 6)))
    with pytest.raises(ValueError, match="expected val"):
        engine.score_summary(val[..., :9], cnt, 0.1, np.ones(6))
    with pytest.raises(TypeError, match="unknown tolerance"):
        engine._score_args(0.5, dict(vtol=0.1))
    assert engine._score_args(1, dict(v_tol=0.2)) == (0.3, 0.1, 0.2, 1.0)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from conflict_rez_amd import engine

    return engine.load_library()


def test_engine_score_checks_shapes_before_the_library(lib):
    """An Engine without a handle (no GPU needed): shape errors are raised by the Python layer, and what passes it reaches cfz_score,
    which refuses the null handle last."""
    from conflict_rez_amd import engine, scenarios

    e = engine.Engine.__new__(engine.Engine)
    e.lib, e.spec, e._h, e._S, e._V, e._rec_used = lib, scenarios.parking_lot_spec(), None, 0, 0, 0
    d = sb.synthetic(2, 7)
    args = (d["traj"], d["tables"], d["table_of"], d["k0"])
    with pytest.raises(ValueError, match="traj"):
        e.score(d["traj"][..., :5], *args[1:])
    with pytest.raises(ValueError, match="tables"):
        e.score(d["traj"], d["tables"][:, :1], d["table_of"], d["k0"])
    with pytest.raises(ValueError, match="table_of"):
        e.score(d["traj"], d["tables"], d["table_of"][:2], d["k0"])
    with pytest.raises(ValueError, match="status"):
        e.score(*args, status=d["status"][:3])
    with pytest.raises(TypeError, match="unknown tolerance"):
        e.score(*args, tol=0.1)
    with pytest.raises(RuntimeError, match="cfz_score: near"):
        e.score(*args, near=-1.0)
    with pytest.raises(RuntimeError, match=r"table_of\[s\] outside"):
        e.score(d["traj"], d["tables"], [0, 2, 1], d["k0"])
    with pytest.raises(RuntimeError, match="null handle"):
        e.score(*args, status=d["status"], iters=d["iters"])
    with pytest.raises(RuntimeError, match="cfz_loop_score: near"):
        e.loop_score(near=float("nan"))
    with pytest.raises(RuntimeError, match="cfz_loop_init has not been called"):
        e.loop_score()


def test_c_refusals(lib):
    """cfz_score / cfz_loop_score check their arguments on the host before they touch the handle or the device."""
    K, S, V, P, T = 3, 2, 2, 2, 5
    traj, tables = np.zeros((K, S, V, 7)), np.zeros((P, V, T, 7))
    tof, k0 = np.array([0, 1], np.int32), np.array([0, 1], np.int32)
    val, cnt = np.zeros((S, V, 10)), np.zeros((S, V, 11), np.int32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def call(K=K, S=S, V=V, traj=traj, P=P, T=T, tables=tables, tof=tof, k0=k0, near=0.5, val=val, cnt=cnt):
        rc = lib.cfz_score(None, K, S, V, p(traj), None, None, P, T, p(tables), p(tof), p(k0), 0.3, 0.1, 0.1, near, p(val), p(cnt))
        assert rc != 0
        return lib.cfz_last_error().decode()

    assert "null handle" in call()
    for kw, what in ((dict(near=-0.1), "near"), (dict(near=float("inf")), "near"), (dict(near=float("nan")), "near"), (dict(val=None), "null val or cnt"),
                     (dict(cnt=None), "null val or cnt"), (dict(K=0), "K, S must be positive"), (dict(S=0), "K, S must be positive"),
                     (dict(V=0), "V in 1..CFZ_MAX_NBR+1"), (dict(V=9), "V in 1..CFZ_MAX_NBR+1"), (dict(P=0), "P, T must be positive"),
                     (dict(T=0), "P, T must be positive"), (dict(traj=None), "null trajectory"), (dict(tables=None), "null trajectory"),
                     (dict(tof=None), "null trajectory"), (dict(k0=None), "null trajectory"), (dict(tof=np.array([0, 2], np.int32)), "table_of[s] outside [0, P)"),
                     (dict(tof=np.array([-1, 0], np.int32)), "table_of[s] outside [0, P)"), (dict(k0=np.array([0, -1], np.int32)), "k0[s] must not be negative")):
        assert what in call(**kw), kw
    for near, what in ((-1.0, "near"), (0.5, "cfz_loop_init has not been called")):
        assert lib.cfz_loop_score(None, 0, 1, 0.3, 0.1, 0.1, near, p(val), p(cnt)) != 0
        assert what in lib.cfz_last_error().decode()
    assert lib.cfz_loop_score(None, 0, 1, 0.3, 0.1, 0.1, 0.5, None, p(cnt)) != 0 and "null val or cnt" in lib.cfz_last_error().decode()
