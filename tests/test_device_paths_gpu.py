"""The device-resident entry points of the C ABI on one GPU (`pytest -m gpu`): `cfz_vsl_step` at the partitions a multi-GPU run of
partitioning B would produce (n_own < V, non-contiguous owners, scenario shards), and `cfz_mpc_solve_device` /
`cfz_mpc_set_carry_device` with their stream ordering and the deferred read of `cfz_last_solve_ms`.

The ranks of the vehicle-sharded loop are emulated inside this process (RCCL refuses two ranks on one device): one `Engine` and one
unchanged `distributed.VehicleShardedLoop` per rank, and in place of the all-gather a board that every rank reads.  The board is a
snapshot taken before the iteration, which is the Jacobi rule: every rank plans against the predictions of the iteration before.

What is compared with what: both `cfz_vsl_step` and `cfz_loop_step` run solve_kernel, prep_stage, loop_post and the same RK4 plant,
and an instance's solve does not depend on its batch (tests/test_determinism_gpu.py), so the sharded ranks must return the device
loop's bits; the device path of a solve must return the bits of the host-buffer path, which is pinned to the port and the goldens
(tests/test_gpu_parity.py).  Against the host replay with the C port: equal status and iteration counts, states and predictions to
the 1e-6 of `test_closed_loop_on_device`.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S, K = 16, 5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# The scenario samples, chosen with the host replay (no GPU) so that the run has a shift fallback and a reference window clamped at
# the table's last sample (T = 301).  `sample_scenarios(16, table, seed=2)` in both:
#   "v4": as drawn.  k0[12] = 269: 269 + K + 30 - 1 = 303 > 300; five solves per iteration end with status 4 or 5.
#   "v2": k0[2] = 286 and k0[13] = 295 written by hand (the sampler keeps 30 samples of margin, more than the horizon of 12):
#         scenario 2 reaches the last sample during the run (286 + 11 = 297, 290 + 11 = 301), scenario 13 is past it from the first
#         iteration; vehicle 0 of scenario 3 starts inside a clearance (status 4 in every iteration).
SAMPLES = {"v4": dict(n_nbr=3, N=30, seed=2, k0={}), "v2": dict(n_nbr=1, N=12, seed=2, k0={2: 286, 13: 295})}


class _Case:
    """One (V, N): the spec, the sample, the host replay and the device loop `cfz_loop_step`, each computed once."""

    def __init__(self, name, ospec):
        from conflict_rez_amd import engine, scenarios
        from oracle.closed_loop import replay
        from oracle.mpc_nlp import MpcSpec

        c = SAMPLES[name]
        self.V, self.N = c["n_nbr"] + 1, c["N"]
        self.spec = scenarios.parking_lot_spec(n_nbr=c["n_nbr"], N=self.N)
        table, _ = scenarios.load_reference_table()
        self.table = np.ascontiguousarray(table[: self.V])
        self.T = self.table.shape[1]
        k0, noise = scenarios.sample_scenarios(S, table, seed=c["seed"])
        for s, k in c["k0"].items():
            k0[s] = k
        self.k0, self.noise = k0, np.ascontiguousarray(noise[:, : self.V])
        if name != "v4":
            ospec = MpcSpec(N=self.N, dt=self.spec.dt, A_obs=self.spec.A_obs, b_obs=self.spec.b_obs, n_nbr=c["n_nbr"])
        self.replay = list(replay(ospec, self.table, self.k0, self.noise, K, dt=self.spec.dt, wb=self.spec.wb))
        e = engine.Engine(self.spec, max_batch=S * self.V)
        e.loop_init(self.table, self.k0, self.noise)
        self.device = []
        for _ in range(K):
            e.loop_step()
            self.device.append(e.loop_get())
        e.close()

    def check_sample(self):
        """The two conditions on the sample, on the replay's own output."""
        assert sum(int((r[2] != 0).sum()) for r in self.replay) >= 1  # a shift fallback runs
        assert (self.k0 + K + self.N - 1 > self.T - 1).any()  # a reference window is clamped at the last sample


@pytest.fixture(scope="module")
def cases(ospec):
    made = {}

    def get(name):
        if name not in made:
            made[name] = _Case(name, ospec)
        return made[name]

    return get


class _Board:
    """What stands in for the all-gather: allpred [S, V, 3, N], x, y, psi of every vehicle's last prediction, all scenarios."""

    def __init__(self, snapshot=True):
        self.snapshot, self.ranks, self.allpred = snapshot, [], None

    def collect(self):
        import torch

        first = self.ranks[0][1]
        out = torch.full((S, first.V, 3, first.N), float("nan"), dtype=torch.float64, device=first.pred.device)  # (NaN: a vehicle no rank owns)
        for ex, vl in self.ranks:
            own = torch.tensor(ex.owned, device=out.device)
            out[ex.scenarios(S), own] = vl.pred[:, :, :3, :]
        return out

    def post(self):
        """Before an iteration: every rank's prediction of the iteration before, copied."""
        self.allpred = self.collect().clone()


class _Exchange:
    """The three members `VehicleShardedLoop` uses of `VehicleShardedExchange`, for one emulated rank."""

    def __init__(self, board, owned, shard=0, n_shards=1):
        self.board, self.owned, self.shard, self.n_shards = board, list(owned), shard, n_shards

    def scenarios(self, n_scenarios):
        from conflict_rez_amd.distributed import scenario_shard

        return scenario_shard(n_scenarios, self.shard, self.n_shards)

    def gather(self, local):
        # (a board that is not a snapshot reads what the ranks hold NOW: those that stepped earlier in the iteration are one ahead)
        allpred = self.board.allpred if self.board.snapshot else self.board.collect()
        return allpred[self.scenarios(S)].contiguous()


def _grid(V, world):
    from conflict_rez_amd.distributed import vehicle_grid

    return [vehicle_grid(V, r, world)[:3] for r in range(world)]


def _ranks(case, parts, board):
    """One engine and one VehicleShardedLoop per (owned vehicles, shard, n_shards) of `parts`."""
    from conflict_rez_amd import engine
    from conflict_rez_amd.distributed import VehicleShardedLoop

    engines = []
    for owned, shard, n_shards in parts:
        ex = _Exchange(board, owned, shard, n_shards)
        sl = ex.scenarios(S)
        e = engine.Engine(case.spec, max_batch=(sl.stop - sl.start) * len(owned))
        engines.append(e)
        board.ranks.append((ex, VehicleShardedLoop(e, ex, case.table, case.k0, case.noise)))
    return engines


PARTITIONS = {
    "v4-world2": ("v4", lambda: _grid(4, 2)),  # own = [0, 2] and [1, 3]: non-contiguous d_own, n_own = 2
    "v4-world4": ("v4", lambda: _grid(4, 4)),  # n_own = 1: loop_post's b / V with V = 1
    "v4-world8": ("v4", lambda: _grid(4, 8)),  # BASELINE.json configs[4]: one vehicle and half the scenarios per rank
    "v4-uneven": ("v4", lambda: [([1, 2, 3], 0, 1), ([0], 0, 1)]),  # ranks of different sizes, not from vehicle_grid
    "v2-world2": ("v2", lambda: _grid(2, 2)),  # another horizon and neighbour count in the index arithmetic
}


@pytest.mark.parametrize("part", list(PARTITIONS))
def test_sharded_ranks_match_the_device_loop_and_the_oracle(cases, part):
    """Every rank of a partition, after every iteration, on the rows it owns: status, iterations, state and prediction equal to
    `cfz_loop_step`'s bit for bit; the carry flag it leaves is status == 0; status and iterations equal to the host replay's with
    the C port, states and predictions within 1e-6.  The samples (SAMPLES) have a shift fallback and a clamped reference window,
    asserted on the replay."""
    import torch

    name, parts = PARTITIONS[part]
    case = cases(name)
    case.check_sample()
    parts = parts()
    assert sorted((v, sh) for own, sh, n in parts for v in own) == sorted((v, sh) for v in range(case.V) for sh in range(parts[0][2]))
    board = _Board()
    engines = _ranks(case, parts, board)
    try:
        for t in range(K):
            board.post()
            for _, vl in board.ranks:
                vl.step()
            torch.cuda.synchronize()
            dev, (o_state, o_pred, o_status, o_iters) = case.device[t], case.replay[t]
            for r, (ex, vl) in enumerate(board.ranks):
                sl, own, n = ex.scenarios(S), ex.owned, len(ex.owned)
                sh = (sl.stop - sl.start, n)
                status, iters = vl.status.cpu().numpy().reshape(sh), vl.iters.cpu().numpy().reshape(sh)
                state, pred = vl.state.cpu().numpy(), vl.pred.cpu().numpy()
                assert state.shape == sh + (5,) and pred.shape == sh + (7, case.N)
                assert np.array_equal(status, dev["status"][sl][:, own]), (t, r)
                assert np.array_equal(iters, dev["iters"][sl][:, own]), (t, r)
                assert np.array_equal(state, dev["state"][sl][:, own]), (t, r)
                assert np.array_equal(pred, dev["pred"][sl][:, own]), (t, r)
                assert np.array_equal(vl.carry.cpu().numpy().reshape(sh), (status == 0).astype(np.int32)), (t, r)
                assert np.array_equal(status, o_status[sl][:, own]), (t, r)
                assert np.array_equal(iters, o_iters[sl][:, own]), (t, r)
                assert np.abs(state - o_state[sl][:, own]).max() < 1e-6, (t, r)
                assert np.abs(pred - o_pred[sl][:, own]).max() < 1e-6, (t, r)
    finally:
        for e in engines:
            e.close()


def test_a_board_that_is_not_a_snapshot_gives_another_result(cases):
    """The emulation itself: when rank 1 reads rank 0's prediction of the SAME iteration (the board is not copied before the
    iteration), its vehicles end elsewhere than in the device loop, on the sample of the test above.  So the vehicles of that
    sample interact, and the equalities above could not hold under a wrong exchange."""
    import torch

    case = cases("v4")
    board = _Board(snapshot=False)
    engines = _ranks(case, _grid(4, 2), board)
    try:
        for t in range(K):
            for _, vl in board.ranks:
                vl.step()
        torch.cuda.synchronize()
        dev = case.device[K - 1]
        (ex0, vl0), (ex1, vl1) = board.ranks
        assert not np.array_equal(vl1.pred.cpu().numpy(), dev["pred"][:, ex1.owned])
        assert not np.array_equal(vl1.state.cpu().numpy(), dev["state"][:, ex1.owned])
    finally:
        for e in engines:
            e.close()


# ---- cfz_mpc_solve_device, cfz_mpc_set_carry_device ---------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def twins():
    """Two engines of the same spec: `host` takes the host-buffer path, `dev` the device pointers."""
    from conflict_rez_amd import engine, scenarios

    spec = scenarios.parking_lot_spec()
    host, dev = engine.Engine(spec, max_batch=20), engine.Engine(spec, max_batch=20)
    yield host, dev
    host.close(); dev.close()


class _DeviceBatch:
    """The arguments of `solve_device` as torch tensors, uploaded and complete before any stream reads them."""

    def __init__(self, x0, ref, nbr, zu):
        import torch

        up = lambda a: None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")
        self.B = len(x0)
        self.x0, self.ref, self.nbr, self.zu = up(x0), up(ref), up(nbr), up(zu)
        self.status = torch.full((self.B,), -1, dtype=torch.int32, device="cuda")
        self.iters = torch.full((self.B,), -1, dtype=torch.int32, device="cuda")
        self.stats = torch.full((self.B, 3), -1.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()

    def solve(self, eng, stream=None):
        eng.solve_device(self.B, self.x0, self.ref, self.nbr, self.zu, self.status, self.iters, self.stats,
                         stream=None if stream is None else stream.cuda_stream)

    def equals(self, out):
        """Bit for bit the result of `Engine.solve` (the statistics of a solve that never iterated may be NaN on both sides)."""
        stats = self.stats.cpu().numpy()
        assert np.array_equal(self.status.cpu().numpy(), out["status"])
        assert np.array_equal(self.iters.cpu().numpy(), out["iters"])
        assert np.array_equal(self.zu.cpu().numpy(), out["zu"])
        for c, key in enumerate(("cost", "kkt_err", "min_sep")):
            assert np.array_equal(stats[:, c], out[key], equal_nan=True), key


def test_golden_batch_on_a_torch_stream(twins, golden):
    """`solve_device` on a stream of the caller's: zu, status, iterations and the three statistics of the host-buffer path, the
    infeasible measurement among them detected without an iteration."""
    import torch

    host, dev = twins
    out = host.solve(golden["x0"], golden["ref"], golden["nbr"], golden["zu"], want_duals=False)
    d = _DeviceBatch(golden["x0"], golden["ref"], golden["nbr"], golden["zu"])
    st = torch.cuda.Stream()
    d.solve(dev, st)
    st.synchronize()
    d.equals(out)
    status, iters = d.status.cpu().numpy(), d.iters.cpu().numpy()
    assert (status == 4).sum() >= 1 and (iters[status == 4] == 0).all()
    assert status.tolist() == golden["meta"][:, 0].astype(int).tolist()


def test_handle_stream_and_the_deferred_solve_time(twins, golden):
    """stream=None is the handle's own stream, which torch knows nothing of: `last_solve_ms()` is the wait (it synchronises on the
    event behind the kernel and reads the time then), returns a positive time, and the same one when asked again."""
    host, dev = twins
    out = host.solve(golden["x0"], golden["ref"], golden["nbr"], golden["zu"], want_duals=False)
    d = _DeviceBatch(golden["x0"], golden["ref"], golden["nbr"], golden["zu"])
    d.solve(dev)
    ms = dev.last_solve_ms()
    d.equals(out)
    assert ms > 0.0
    assert dev.last_solve_ms() == ms


def test_no_neighbours_takes_a_null_d_nbr():
    """The configs[1] shape of `test_other_shapes_and_error_paths` (no neighbours, four obstacles) with d_nbr = NULL."""
    import torch

    from conflict_rez_amd import engine, scenarios

    table, _ = scenarios.load_reference_table()
    B = 5
    sp = scenarios.parking_lot_spec(n_nbr=0, n_obs=4)
    k0, noise = scenarios.sample_scenarios(B, table, seed=4)
    x0, ref, nbr, zu = scenarios.mpc_batch_from_table(sp, table[:1], k0, noise[:, :1])
    host, dev = engine.Engine(sp, max_batch=B), engine.Engine(sp, max_batch=B)
    try:
        out = host.solve(x0, ref, nbr, zu, want_duals=False)
        assert (out["status"] == 0).any()
        d = _DeviceBatch(x0, ref, None, zu)
        st = torch.cuda.Stream()
        d.solve(dev, st)
        st.synchronize()
        d.equals(out)
    finally:
        host.close(); dev.close()


def _carry_steps():
    """The first two MPC iterations of the three sequences of tests/golden/carry_inputs.npz (slot s = sequence s)."""
    ci = np.load(os.path.join(GOLDEN, "carry_inputs.npz"))
    return [tuple(ci[k][[t, 3 + t, 6 + t]] for k in ("x0", "ref", "nbr", "zu")) for t in range(2)]


FLAGS = [1, 0, 1]  # [1, 0, 1, 0, ...] over the three slots


@pytest.mark.parametrize("how", ["device", "staged"])
def test_carry_flags_reach_the_device_solve(twins, how):
    """The second MPC iteration with the flags [1, 0, 1]: `set_carry` + `solve` on one engine; on the other `solve_device` on a
    stream of the caller's, the flags either a device array (`set_carry_device`: the kernel reads the caller's memory) or host flags
    (`set_carry`: staged on the handle's stream, which the caller's stream has to wait for).  Equal bit for bit, a flagged instance
    takes fewer iterations than unflagged, and a third solve with nothing set is cold: the flags hold for one solve."""
    import torch

    host, dev = twins
    one, two = _carry_steps()
    st = torch.cuda.Stream()
    a1 = host.solve(*one, want_duals=False)
    d1 = _DeviceBatch(*one)
    d1.solve(dev, st)
    st.synchronize()
    d1.equals(a1)
    assert (a1["status"] == 0).all()  # (every slot leaves a record to carry)
    a2 = host.solve(*two, want_duals=False, carry=FLAGS)
    d2 = _DeviceBatch(*two)
    flags = torch.tensor(FLAGS, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    if how == "device":
        dev.set_carry_device(3, flags)
    else:
        dev.set_carry(FLAGS)
    d2.solve(dev, st)
    st.synchronize()
    d2.equals(a2)
    cold = host.solve(*two, want_duals=False)
    flagged = np.array(FLAGS, bool)
    assert (a2["iters"][flagged] < cold["iters"][flagged]).any()
    assert np.array_equal(a2["iters"][~flagged], cold["iters"][~flagged])
    d3 = _DeviceBatch(*two)
    d3.solve(dev, st)
    st.synchronize()
    d3.equals(cold)
    del flags


def test_refused_calls_leave_the_handle_usable(twins, golden, cases):
    """-1 with the library's text for a batch beyond max_batch, a null d_zu, a `cfz_vsl_step` whose V is not n_nbr + 1 and one whose
    S * n_own is beyond max_batch; a correct solve right after each pair."""
    import torch

    from conflict_rez_amd import engine

    host, dev = twins
    out = host.solve(golden["x0"], golden["ref"], golden["nbr"], golden["zu"], want_duals=False)
    d = _DeviceBatch(golden["x0"], golden["ref"], golden["nbr"], golden["zu"])
    st = torch.cuda.Stream()

    def solves_correctly():
        d.zu.copy_(torch.tensor(golden["zu"], dtype=torch.float64))  # (the warm start again: d_zu is in/out)
        torch.cuda.synchronize()
        d.solve(dev, st)
        st.synchronize()
        d.equals(out)

    with pytest.raises(RuntimeError, match="batch size out of range"):
        dev.solve_device(dev.max_batch + 1, d.x0, d.ref, d.nbr, d.zu, d.status, d.iters, d.stats, stream=st.cuda_stream)
    solves_correctly()
    with pytest.raises(RuntimeError, match="null device pointer"):
        dev.solve_device(d.B, d.x0, d.ref, d.nbr, None, d.status, d.iters, d.stats, stream=st.cuda_stream)
    solves_correctly()
    # cfz_vsl_step: the rank that owns vehicles 0 and 2 of all scenarios; `small` is one instance short of its S * n_own
    case = cases("v4")
    board = _Board()
    engines = _ranks(case, _grid(4, 2), board)
    e = engines[0]
    small = engine.Engine(case.spec, max_batch=S * 2 - 1)
    try:
        vl = board.ranks[0][1]
        board.post()
        args = (vl.T, vl.table, vl.k0, 0, board.allpred, vl.pred, vl.state, vl.status, vl.iters, vl.stats, vl.carry)
        cur = torch.cuda.current_stream().cuda_stream
        with pytest.raises(RuntimeError, match=r"S \* n_own outside the handle's batch"):
            small.vsl_step(S, case.V, vl.d_own, *args, stream=cur)
        again = small.solve(golden["x0"], golden["ref"], golden["nbr"], golden["zu"], want_duals=False)
        assert all(np.array_equal(again[k], out[k], equal_nan=True) for k in ("zu", "status", "iters", "cost", "kkt_err", "min_sep"))
        with pytest.raises(RuntimeError, match=r"V must be n_nbr \+ 1"):
            e.vsl_step(S, case.V - 1, vl.d_own, *args, stream=cur)
        vl.step()
        torch.cuda.synchronize()
        dev0 = case.device[0]
        assert np.array_equal(vl.status.cpu().numpy().reshape(S, 2), dev0["status"][:, [0, 2]])
        assert np.array_equal(vl.pred.cpu().numpy(), dev0["pred"][:, [0, 2]])
        assert np.array_equal(vl.state.cpu().numpy(), dev0["state"][:, [0, 2]])
    finally:
        small.close()
        for e in engines:
            e.close()
