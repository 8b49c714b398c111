"""The merge of a workgroup's wavefronts (`block_merge` of conflict_rez_amd/csrc/cfz_wave.inl) alone, as delay_kernel and schedule_kernel
call it, run on an MI355X by tests/hip/block_merge.hip -- a stand-alone program that includes nothing of the product but that header --
for four wavefronts and for two, over 33 rounds of alternating parity with one barrier each, a wavefront held back in the odd rounds;
against the header's host form in a g++ build (tests/hip/wave_merge_host.cpp), which the CPU builds of the two kernels call.  The host
form itself is checked without a GPU against Python's min and sum.  Comparisons are of fields, never of padding."""
import numpy as np
import pytest

from emu_build import build_hip_program, ptr, run_program
from wave_case import CASE, host_lib, key as _key, same as _same

SUM = np.dtype([("sum", "<i4"), ("n", "<i4")])
ROUNDS = 33
WAVES = (4, 2)


def _inputs(waves):
    """The accumulator of wavefront w in round r, [ROUNDS, waves].  The round's smallest x is 5 r, held by a wavefront that changes with
    the round; the sums lie 10000 apart: no two rounds share their minimum or their sum (asserted below), so a slot of another round
    cannot produce a right answer."""
    r, w = np.meshgrid(np.arange(ROUNDS), np.arange(waves), indexing="ij")
    c = np.zeros((ROUNDS, waves), CASE)
    c["x"] = 5.0 * r + (w + r) % 4
    c["a"] = (r * 11 + w) % 5 - 2
    c["b"] = np.stack([w, r, 63 - w], -1)
    s = np.zeros((ROUNDS, waves), SUM)
    s["sum"] = 10000 * r + (w + 1) * (r + 3)
    s["n"] = 1
    return c, s


@pytest.fixture(scope="module")
def host():
    """The header's host form per round: acc [ROUNDS, waves] -> [ROUNDS]."""
    lib = host_lib()

    def run(acc):
        acc = np.ascontiguousarray(acc)
        out = np.zeros(acc.shape[0], acc.dtype)
        fn = lib.block_host_min if acc.dtype == CASE else lib.block_host_sum
        assert fn(ptr(acc), acc.shape[0], acc.shape[1], ptr(out)) == 0
        return out

    return run


@pytest.mark.parametrize("waves", WAVES)
def test_host_form_against_min_and_sum(host, waves):
    """Without a GPU: the fold of every round is the lexicographic minimum / the sum and the count of its wavefronts, and the rounds differ."""
    c, s = _inputs(waves)
    m, t = host(c), host(s)
    for r in range(ROUNDS):
        assert _key(m[r]) == min(_key(c[r, w]) for w in range(waves)), r
        assert int(t["sum"][r]) == sum(int(v) for v in s["sum"][r]) and int(t["n"][r]) == waves, r
    assert len({_key(v) for v in m}) == ROUNDS and len(set(t["sum"].tolist())) == ROUNDS  # the condition on the inputs
    assert len({int(np.argmin(c["x"][r])) for r in range(ROUNDS)}) == waves  # every wavefront holds the minimum in some round


@pytest.fixture(scope="module")
def device(tmp_path_factory):
    """tests/hip/block_merge.hip built for gfx950 and run once -> {waves: (min [ROUNDS, 64 waves] CASE, sum [ROUNDS, 64 waves] SUM)}."""
    d = tmp_path_factory.mktemp("block_merge")
    exe, fin, fout = build_hip_program("tests/hip/block_merge.hip", d / "block_merge"), str(d / "in.bin"), str(d / "out.bin")
    with open(fin, "wb") as f:
        for waves in WAVES:
            c, s = _inputs(waves)
            f.write(c.tobytes() + s.tobytes())
    run_program(exe, [fin, fout])
    raw = open(fout, "rb").read()
    assert len(raw) == sum(ROUNDS * 64 * w * (CASE.itemsize + SUM.itemsize) for w in WAVES)
    out, at = {}, 0
    for w in WAVES:
        n = ROUNDS * 64 * w
        out[w] = (np.frombuffer(raw, CASE, n, at).reshape(ROUNDS, 64 * w), np.frombuffer(raw, SUM, n, at + n * CASE.itemsize).reshape(ROUNDS, 64 * w))
        at += n * (CASE.itemsize + SUM.itemsize)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("waves", WAVES)
def test_every_lane_of_every_round_equals_the_host_fold(device, host, waves):
    """Every lane of every round holds the host form's fold of that round's accumulators, so all lanes of a round are equal too."""
    c, s = _inputs(waves)
    for got, want in zip(device[waves], (host(c), host(s))):
        assert got.shape == (ROUNDS, 64 * waves)
        for r in range(ROUNDS):
            assert _same(got[r], np.repeat(got[r, :1], 64 * waves)), r
            assert _same(got[r], np.repeat(want[r:r + 1], 64 * waves)), r
