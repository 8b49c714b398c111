"""The audit kernel's geometry and bookkeeping (conflict_rez_amd/csrc/cfz_audit.inl) in its CPU build, against the numpy statement of
the same definitions in tests/audit_binding.py: signed distances of random and hand-placed polygons, the tie-breaking of the minima
and the arrival rule on a hand-made record, and independence of how the items are dealt out over the lanes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audit_binding as ab  # noqa: E402

SQ = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])  # unit square, counter-clockwise
G = np.array([3.3, 0.9, 0.6, 0.9])  # the reference's body (VehicleBody)


def both(P, Q):
    d = ab.emu_signed_distance(P, Q)
    assert abs(d - float(ab.signed_distance(P, Q))) <= 1e-12
    assert abs(d - ab.emu_signed_distance(Q, P)) <= 1e-12  # symmetric
    return d


def test_known_answers():
    assert both(SQ, SQ + [1.5, 0.0]) == pytest.approx(0.5, abs=1e-15)
    assert both(SQ, SQ + [0.75, 0.0]) == pytest.approx(-0.25, abs=1e-15)
    assert both(SQ, SQ + [4.0, 5.0]) == pytest.approx(5.0, abs=1e-15)  # corner (1, 1) to corner (4, 5): gap (3, 4)
    assert both(SQ, SQ + [1.0, 0.0]) == 0.0  # sharing an edge
    assert both(SQ, SQ + [1.0, 1.0]) == 0.0  # corner to corner
    assert both(SQ, SQ) == pytest.approx(-1.0, abs=1e-15)  # identical
    assert both(SQ, 0.25 + 0.5 * SQ) == pytest.approx(-0.75, abs=1e-15)  # nested: shortest way out is 0.75 along an axis
    assert both(SQ, SQ[::-1] + [1.5, 0.0]) == pytest.approx(0.5, abs=1e-15)  # clockwise order is the same polygon
    diamond = np.array([[0.0, -1.0], [1.0, 0.0], [0.0, 1.0], [-1.0, 0.0]]) + [3.0, 0.5]
    assert both(SQ, diamond) == pytest.approx(1.0, abs=1e-15)  # diamond's left corner (2, 0.5) to the square's right edge


def test_random_pairs_against_numpy():
    rng = np.random.default_rng(7)
    n = 5000
    # body / body: centres in a 12 m x 6 m patch, so that about half of the pairs overlap
    A = ab.body(G, rng.uniform(0, 12, n), rng.uniform(0, 6, n), rng.uniform(-np.pi, np.pi, n))
    B = ab.body(G, rng.uniform(0, 12, n), rng.uniform(0, 6, n), rng.uniform(-np.pi, np.pi, n))
    # body / box: the parking lot's six obstacles and random boxes
    from conflict_rez_amd import scenarios

    spec = scenarios.parking_lot_spec()
    lot = [ab.obstacle_vertices(spec.A_obs[j], spec.b_obs[j]) for j in range(spec.n_obs)]
    boxes = []
    for i in range(n):
        if i % 2:
            boxes.append(lot[i % len(lot)])
        else:
            x0, y0, w, h = rng.uniform(0, 10), rng.uniform(0, 6), rng.uniform(0.2, 6), rng.uniform(0.2, 6)
            boxes.append(np.array([[x0, y0], [x0 + w, y0], [x0 + w, y0 + h], [x0, y0 + h]]))
    poses = np.stack([rng.uniform(0, 35, n), rng.uniform(0, 35, n), rng.uniform(-np.pi, np.pi, n)], 1)
    poses[::2, :2] = rng.uniform(0, 12, (len(poses[::2]), 2))
    Cb = ab.body(G, poses[:, 0], poses[:, 1], poses[:, 2])
    ref_bb = ab.signed_distance(A, B)
    ref_bo = ab.signed_distance(Cb, np.stack(boxes))
    emu_bb = np.array([ab.emu_signed_distance(A[i], B[i]) for i in range(n)])
    emu_bo = np.array([ab.emu_signed_distance(Cb[i], boxes[i]) for i in range(n)])
    assert np.abs(emu_bb - ref_bb).max() <= 1e-12 and np.abs(emu_bo - ref_bo).max() <= 1e-12
    for ref in (ref_bb, ref_bo):  # both signs well represented
        assert (ref < 0).sum() > n // 10 and (ref > 0).sum() > n // 10
    # the sign agrees with an exact intersection test (scenarios._quad_distance: 0 when touching or overlapping)
    qd = scenarios._quad_distance(A, B)
    assert np.array_equal(qd > 0, ref_bb > 0)
    assert np.abs(qd[ref_bb > 0] - ref_bb[ref_bb > 0]).max() <= 1e-12


def _row_record(K=4):
    """Three bodies of length 2 and width 1 in a row on the x-axis, gaps 1 and 1; vehicle 2 closes to 0.5 from step 2."""
    g = np.array([1.0, 0.5, 1.0, 0.5])
    traj = np.zeros((K, 1, 3, 7))
    traj[:, 0, :, 0] = [0.0, 3.0, 6.0]
    traj[2:, 0, 2, 0] = 5.5
    traj[..., 3] = 1.0  # moving: no arrival
    goal = np.zeros((1, 3, 3))
    return g, traj, goal


@pytest.mark.parametrize("lanes", [1, 2, 8, 64])
def test_tie_breaking(lanes):
    g, traj, goal = _row_record()
    tol = (0.1, 0.1, 0.1)
    # all gaps 1 at step 0 and 1: the minimum over pairs is 0.5, at step 2 (lowest of the tied steps 2, 3), pair (1, 2)
    out = ab.emu_audit(traj, goal, np.zeros((0, 4, 2)), g, *tol, lanes=lanes)
    assert out["clear"][0, 0] == 0.5 and out["where"][0, :3].tolist() == [2, 1, 2]
    assert np.isinf(out["clear"][0, 1]) and out["where"][0, 3:].tolist() == [-1, -1, -1]
    assert out["first_contact"][0] == -1 and out["arrive"][0].tolist() == [-1, -1, -1]
    # equal gaps everywhere: lowest step, then lowest pair
    traj[2:, 0, 2, 0] = 6.0
    out = ab.emu_audit(traj, goal, np.zeros((0, 4, 2)), g, *tol, lanes=lanes)
    assert out["clear"][0, 0] == 1.0 and out["where"][0, :3].tolist() == [0, 0, 1]
    # an obstacle touched by vehicles 0 and 1 alike at every step, overlapped by vehicle 2 from step 3 on
    box = np.array([[-1.0, 0.5], [8.0, 0.5], [8.0, 2.0], [-1.0, 2.0]])
    traj[3:, 0, 2, 1] = 0.25
    out = ab.emu_audit(traj, goal, box[None], g, *tol, lanes=lanes)
    assert out["clear"][0, 1] == -0.25 and out["where"][0, 3:].tolist() == [3, 2, 0]
    assert out["first_contact"][0] == 3
    ref = ab.audit(traj, goal, box[None], g, *tol)
    for k in ("where", "first_contact", "arrive"):
        assert np.array_equal(out[k], ref[k]), k
    assert np.allclose(out["clear"], ref["clear"], atol=1e-12, rtol=0)


def test_arrival_rule():
    K, g = 8, np.array([1.0, 0.5, 1.0, 0.5])
    traj = np.zeros((K, 2, 2, 7))
    goal = np.array([[[10.0, 0.0, 0.0], [-10.0, 20.0, np.pi]], [[0.0, 0.0, 0.0], [0.0, 50.0, 0.0]]])
    # scenario 0, vehicle 0: at the goal position from step 3, but still at speed until step 5
    traj[:, 0, 0, 0] = [4, 6, 8, 10, 10, 10, 10, 10]
    traj[:, 0, 0, 3] = [1, 1, 1, 0.5, 0.2, 0.05, 0.0, 0.0]
    # vehicle 1: heading -pi + 0.05 is within 0.1 of pi once wrapped; inside pos_tol = 0.1 at step 6 only
    traj[:, 0, 1, :3] = [-10.0, 20.5, -np.pi + 0.05]
    traj[6, 0, 1, 1] = 20.05
    # scenario 1: vehicle 0 sits on its goal from the start with a heading off by 2 pi (arrived at step 0); vehicle 1 never gets there
    traj[:, 1, 0, 2] = 2 * np.pi
    traj[:, 1, 1, :2] = [0.0, 40.0]
    for lanes in (1, 4, 64):
        out = ab.emu_audit(traj, goal, np.zeros((0, 4, 2)), g, 0.1, 0.1, 0.1, lanes=lanes)
        assert out["arrive"].tolist() == [[5, 6], [0, -1]], out["arrive"]
        ref = ab.audit(traj, goal, np.zeros((0, 4, 2)), g, 0.1, 0.1, 0.1)
        assert np.array_equal(out["arrive"], ref["arrive"])


def test_random_records_lane_independent():
    """Random records: the audit over 1, 3... lanes equals the numpy statement (integers equal, distances to 1e-12)."""
    rng = np.random.default_rng(11)
    from conflict_rez_amd import scenarios

    spec = scenarios.parking_lot_spec()
    obs = np.stack([ab.obstacle_vertices(spec.A_obs[j], spec.b_obs[j]) for j in (0, 3)])
    K, S, V = 9, 16, 3
    traj = np.zeros((K, S, V, 7))
    start = np.stack([rng.uniform(-20, 50, (S, V)), rng.uniform(-20, 50, (S, V)), rng.uniform(-np.pi, np.pi, (S, V))], -1)
    for t in range(K):
        traj[t, ..., :3] = start + t * rng.normal(0, 1.5, (S, V, 3))
    traj[..., 3] = rng.uniform(-0.2, 0.2, (K, S, V))
    goal = traj[-1, ..., :3] + rng.normal(0, 0.05, (S, V, 3))
    ref = ab.audit(traj, goal, obs, spec.g, 0.3, 0.1, 0.1)
    for lanes in (1, 2, 16, 64):
        out = ab.emu_audit(traj, goal, obs, spec.g, 0.3, 0.1, 0.1, lanes=lanes)
        for k in ("where", "first_contact", "arrive"):
            assert np.array_equal(out[k], ref[k]), (lanes, k)
        assert np.abs(out["clear"] - ref["clear"]).max() <= 1e-12
    assert (ref["first_contact"] >= 0).any() and (ref["first_contact"] < 0).any()
    assert (ref["arrive"] >= 0).any()
