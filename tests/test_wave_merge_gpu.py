"""The merge of a wavefront's accumulators (conflict_rez_amd/csrc/cfz_wave.inl) alone: `wave_xor` and the two butterflies that audit_kernel,
score_kernel, conflict_kernel and delay_kernel call, run on an MI355X by tests/hip/wave_merge.hip -- a stand-alone program that includes
nothing of the product but that header -- over two test structs with padding words (tests/hip/wave_merge_case.h), against the header's
host forms in a g++ build (tests/hip/wave_merge_host.cpp), which the CPU builds of the four kernels call.  The host forms themselves are
checked without a GPU against plain folds over the lanes.  Comparisons are of fields, never of padding."""
import numpy as np
import pytest

from emu_build import build_hip_program, ptr, run_program
from wave_case import CASE, host_lib, key as _key, same as _same

SPAN = np.dtype([("first", "<i4"), ("last", "<i4"), ("count", "<i4"), ("sum", "<f8")], align=True)
assert SPAN.itemsize == 24  # as the static_asserts of wave_merge_case.h
LANES = 64
OFFS = (1, 2, 4, 8, 16, 32)
WIDTHS = (1, 2, 4, 8, 16, 32, 64)


def _inputs():
    """Lane l's values.  x ties in fours (lanes 7, 23, 39, 55 share the smallest), a decides among them for lane 55, b[2] makes every lane
    distinct; the sums mix +-1e16 with tenths, so that their value depends on the order in which they are added."""
    l = np.arange(LANES)
    c = np.zeros(LANES, CASE)
    c["x"] = ((l * 29 + 5) % 16) * 0.25
    c["a"] = (l * 11) % 5 - 2
    c["b"] = np.stack([(l * 7) % 3, (l * 13) % 4, 63 - l], 1)
    s = np.zeros(LANES, SPAN)
    s["first"] = s["last"] = l
    s["count"] = 1
    s["sum"] = ((l % 3) - 1) * 1e16 + (l + 1) * 0.1
    return c, s


@pytest.fixture(scope="module")
def host():
    """The header's host forms: (acc, width) -> the lanes after the butterfly, a new array."""
    lib = host_lib()

    def run(fn, acc, width):
        out = np.ascontiguousarray(acc).copy()
        assert fn(ptr(out), len(out), width) == 0
        return out

    return (lambda acc, width: run(lib.wave_host_min, acc, width)), (lambda acc, width: run(lib.wave_host_concat, acc, width))


def test_host_forms_against_plain_folds(host):
    """Without a GPU.  Commutative: every lane of a group ends with the group's lexicographic minimum (a minimum is idempotent, so not only
    lane 0).  Ordered: every lane of a group holds first = the group's first lane, last = its last, count = width -- a swapped operand
    anywhere would exchange first and last -- and the same sum, bit for bit."""
    host_min, host_concat = host
    c, s = _inputs()
    fwd, rev = 0.0, 0.0
    for v in s["sum"]:
        fwd = fwd + float(v)
    for v in s["sum"][::-1]:
        rev = rev + float(v)
    assert fwd != rev  # a condition on the inputs: the sum does depend on the order
    assert min(range(LANES), key=lambda l: _key(c[l])) == 55
    for w in WIDTHS:
        m, o = host_min(c, w), host_concat(s, w)
        for g in range(0, LANES, w):
            want = min((c[l] for l in range(g, g + w)), key=_key)
            assert all(_key(m[l]) == _key(want) for l in range(g, g + w)), (w, g)
            assert (o["first"][g:g + w] == g).all() and (o["last"][g:g + w] == g + w - 1).all() and (o["count"][g:g + w] == w).all(), (w, g)
            assert len(set(o["sum"][g:g + w].view(np.int64).tolist())) == 1, (w, g)


@pytest.fixture(scope="module")
def device(tmp_path_factory):
    """tests/hip/wave_merge.hip built for gfx950 and run once -> (xor [6, 64] CASE, min [64] CASE, concat [7, 64] SPAN)."""
    d = tmp_path_factory.mktemp("wave_merge")
    exe, fin, fout = build_hip_program("tests/hip/wave_merge.hip", d / "wave_merge"), str(d / "in.bin"), str(d / "out.bin")
    c, s = _inputs()
    with open(fin, "wb") as f:
        f.write(c.tobytes() + s.tobytes())
    run_program(exe, [fin, fout])
    raw = open(fout, "rb").read()
    n_case = (len(OFFS) + 1) * LANES
    assert len(raw) == n_case * CASE.itemsize + len(WIDTHS) * LANES * SPAN.itemsize
    cases = np.frombuffer(raw, CASE, n_case)
    spans = np.frombuffer(raw, SPAN, len(WIDTHS) * LANES, n_case * CASE.itemsize)
    return cases[: len(OFFS) * LANES].reshape(len(OFFS), LANES), cases[len(OFFS) * LANES :], spans.reshape(len(WIDTHS), LANES)


@pytest.mark.gpu
def test_wave_xor_moves_every_field(device):
    """Lane l receives lane l ^ off's struct: every field, on both sides of the padding words."""
    c, _ = _inputs()
    lanes = np.arange(LANES)
    for k, off in enumerate(OFFS):
        assert _same(device[0][k], c[lanes ^ off]), off


@pytest.mark.gpu
def test_butterflies_equal_the_host_forms(device, host):
    """Both butterflies, every lane, against the host forms on the same inputs: the commutative one at width 64, the ordered one at every
    group width, where every lane of a group also holds the same total with the same bits."""
    host_min, host_concat = host
    c, s = _inputs()
    assert _same(device[1], host_min(c, LANES))
    assert _key(device[1][0]) == _key(c[55])
    for k, w in enumerate(WIDTHS):
        got = device[2][k]
        assert _same(got, host_concat(s, w)), w
        for g in range(0, LANES, w):
            assert _same(got[g:g + w], np.repeat(got[g:g + 1], w)), (w, g)
