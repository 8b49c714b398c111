"""The delay search over a conflict map, twice: a ctypes binding of the test-only CPU build of the kernel source
(tests/emu/cfz_delay_emu.cpp over conflict_rez_amd/csrc/cfz_delay.inl, the lane count an argument), and an independent numpy statement
of the definitions of include/confrez_hip.h ("start delays that resolve a plan set's conflicts"): a plain itertools.product over the caps
that takes the minimum of (max(d), sum(d), d) over the feasible vectors -- no shells, no bits, no merges -- that both the CPU build and
the GPU kernel are checked against.  Also the synthetic maps and the cases both test modules use."""
import ctypes as C
import functools
import itertools

import numpy as np

from conflict_binding import pairs
from emu_build import load, ptr

OUT = ("delays", "found", "span", "total")
_i, _vp = C.c_int, C.c_void_p
PROTOTYPES = {"cfz_emu_delay_search": (_i, [_i, _i, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp])}  # of tests/emu/cfz_delay_emu.cpp


def lib():
    return load("cfz_delay_emu", ("tests/emu/cfz_delay_emu.cpp", "conflict_rez_amd/csrc/cfz_delay.inl", "conflict_rez_amd/csrc/cfz_wave.inl"), PROTOTYPES)


def vehicles(npair):
    V = int(round((1 + (1 + 8 * npair) ** 0.5) / 2))
    assert V * (V - 1) // 2 == npair
    return V


def _caps(cap, P, V, D):
    return np.full((P, V), D, np.int32) if cap is None else np.ascontiguousarray(np.broadcast_to(np.asarray(cap, np.int32), (P, V)))


def emu_delays(count, clear=None, slack=0, cap=None, lanes=64):
    """The CPU build with `lanes` lanes per set -> dict(delays [P, V], found, span, total, clear [P] (NaN where it is not written))."""
    count = np.ascontiguousarray(count, np.int32)
    P, npair, L = count.shape
    V, D = vehicles(npair), L // 2
    clear = None if clear is None else np.ascontiguousarray(clear, float)
    cap = None if cap is None else _caps(cap, P, V, D)
    delays, info, rclear = np.full((P, V), -7, np.int32), np.full((P, 3), -7, np.int32), np.full(P, np.nan)
    assert lib().cfz_emu_delay_search(P, V, D, ptr(count), ptr(clear), slack, ptr(cap), lanes, ptr(delays), ptr(info), ptr(rclear)) == 0
    return dict(delays=delays, found=info[:, 0] == 1, span=info[:, 1], total=info[:, 2], clear=rclear)


# ---- numpy statement ---------------------------------------------------------------------------------------------------------
def search(count, clear=None, slack=0, cap=None):
    """delays, found, span, total, clear from their definitions: per set the minimum of (max(d), sum(d), d) over every d in the box of
    the caps for which every pair's lag, and every lag within `slack` of it, lies inside the window and is free."""
    count = np.asarray(count)
    P, npair, L = count.shape
    V, D = vehicles(npair), L // 2
    cap = _caps(cap, P, V, D)
    free = count == 0
    if clear is not None:
        free = free & np.isfinite(np.asarray(clear))
    pr = pairs(V)
    out = dict(delays=np.full((P, V), -1, np.int32), found=np.zeros(P, bool), span=np.full(P, -1, np.int32), total=np.full(P, -1, np.int32),
               clear=np.full(P, np.nan if clear is None else -np.inf))
    for p in range(P):
        ok = [[all(0 <= t <= 2 * D and free[p, q, t] for t in range(j - slack, j + slack + 1)) for j in range(L)] for q in range(npair)]
        feasible = (d for d in itertools.product(*(range(int(c) + 1) for c in cap[p])) if all(ok[q][d[w] - d[u] + D] for q, (u, w) in enumerate(pr)))
        best = min(((max(d), sum(d), d) for d in feasible), default=None)
        if best is None:
            continue
        out["delays"][p], out["found"][p], out["span"][p], out["total"][p] = best[2], True, best[0], best[1]
        if clear is not None:
            out["clear"][p] = min((clear[p, q, best[2][w] - best[2][u] + D] for q, (u, w) in enumerate(pr)), default=np.inf)
    return out


def same(a, b, what=OUT):
    """Every integer of two results equal; -> True so that it can stand in an assert."""
    for k in what:
        assert np.array_equal(a[k], b[k]), (k, a[k].tolist(), b[k].tolist())
    return True


# ---- synthetic maps ----------------------------------------------------------------------------------------------------------
def iid_map(P, V, D, rho, seed=0):
    rng = np.random.default_rng([seed, P, V, D]); npair = V * (V - 1) // 2
    hit = rng.random((P, npair, 2 * D + 1)) < rho
    return (hit * rng.integers(1, 9, hit.shape)).astype(np.int32)


def band_map(P, V, D, seed=0):   # one blocked interval of lags per pair, near lag 0: what real maps look like
    rng = np.random.default_rng([seed, P, V, D, 1]); npair = V * (V - 1) // 2; lag = np.arange(-D, D + 1)
    c = rng.integers(-2, 3, (P, npair, 1)); h = rng.integers(0, D // 2 + 1, (P, npair, 1)); on = rng.random((P, npair, 1)) < 0.7
    hit = on & (np.abs(lag - c) <= h)
    return (hit * rng.integers(1, 9, hit.shape)).astype(np.int32)


def clear_map(count, seed=0):
    """Clearances that go with a count map: above the margin where the count is 0, below it elsewhere, all distinct."""
    rng = np.random.default_rng([seed, 7] + list(count.shape))
    return np.where(count == 0, rng.uniform(0.05, 3.0, count.shape), rng.uniform(-1.5, 0.05, count.shape))


# name: (generator, its arguments, slack, cap, some set is not found, some set is found at span >= 2): the cases of both test modules.
# D = 0; 2D+1 no multiple of 32; shells smaller than one round of 256 lanes (V = 2) and of many rounds (V = 4, D = 10); a cap of 0; 28 pairs.
CASES = {
    "iid_2_0": (iid_map, (16, 2, 0, 0.5), 0, None, True, False),
    "iid_2_1": (iid_map, (16, 2, 1, 0.5), 0, None, True, False),
    "iid_4_5_cap": (iid_map, (16, 4, 5, 0.45), 0, (5, 0, 5, 5), True, True),
    "iid_4_9": (iid_map, (16, 4, 9, 0.55), 0, None, False, True),
    "band_3_6_r1": (band_map, (16, 3, 6), 1, None, True, True),
    "band_4_10": (band_map, (16, 4, 10), 0, None, False, True),
    "band_4_10_r2": (band_map, (16, 4, 10), 2, None, True, True),
    "iid_5_3": (iid_map, (8, 5, 3, 0.4), 0, None, True, True),
    "iid_8_1": (iid_map, (4, 8, 1, 0.15), 0, None, True, False),
    "iid_1_3": (iid_map, (16, 1, 3, 0.5), 0, None, False, False),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(count, clear, slack, cap, reference) of a case: the numpy statement computed once, shared by the tests of both modules, not to
    be written to.  Asserts that the reference contains what the table says, so that a generator change cannot quietly empty a case."""
    gen, args, slack, cap, some_not, some_far = CASES[name]
    count = gen(*args)
    clear = clear_map(count)
    ref = search(count, clear, slack, cap)
    assert (~ref["found"]).any() == some_not and (ref["span"] >= 2).any() == some_far, (name, ref["span"].tolist())
    for a in (count, clear) + tuple(ref.values()):
        a.setflags(write=False)
    return count, clear, slack, cap, ref


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def check_refusals(lib, h):
    """Every refusal of the three C entry points that needs no handle: -1, the text names the cause, the outputs stay unwritten.  Calls
    that pass those checks are refused for the null handle where h is None (the loop form: for the missing loop_init) and served
    otherwise.  -> the number of calls that were served."""
    import conflict_binding as cb

    count, tab = np.zeros((2, 6, 9), np.int32), np.ascontiguousarray(cb.synthetic(2, 4, 64))
    delays, info, rclear = np.full((2, 4), 7, np.int32), np.full((2, 3), 7, np.int32), np.full(2, 7.0)
    cap_bad, cap_neg = np.array([[4, 4, 4, 4], [4, 5, 4, 4]], np.int32), np.array([[0, -1, 0, 0]] * 2, np.int32)
    o = (ptr(delays), ptr(info), ptr(rclear))
    search = lambda P=2, V=4, D=4, c=ptr(count), r=0, cap=None, out=o: lib.cfz_delay_search(h, P, V, D, c, None, r, cap, *out)  # noqa: E731
    plan = lambda P=2, V=4, T=64, t=ptr(tab), D=4, m=0.05, r=0, cap=None, out=o: lib.cfz_plan_delays(h, P, V, T, t, D, m, r, cap, *out)  # noqa: E731
    loop = lambda D=4, m=0.05, r=0: lib.cfz_loop_plan_delays(h, D, m, r, None, *o)  # noqa: E731
    # (D+1)^V against 2^31: 215^4 and 46340^2 are below it, 216^4, 15^8 and 46341^2 above
    for call, text in ((lambda: search(P=0), "P, V must be positive"), (lambda: search(V=0), "P, V must be positive"),
                       (lambda: search(V=9), "V must be in 1..CFZ_MAX_NBR"), (lambda: search(D=-1), "D must not be negative"),
                       (lambda: search(r=-1), "slack must not be negative"), (lambda: search(c=None), "null count"),
                       (lambda: search(out=(None, ptr(info), ptr(rclear))), "null delays"), (lambda: search(cap=ptr(cap_bad)), "a cap lies outside"),
                       (lambda: search(cap=ptr(cap_neg)), "a cap lies outside"), (lambda: search(D=215), "search space too large"),
                       (lambda: search(V=8, D=14), "search space too large"), (lambda: search(V=2, D=46340), "search space too large"),
                       (lambda: plan(P=0), "P, T must be positive"), (lambda: plan(T=0), "P, T must be positive"),
                       (lambda: plan(V=9), "V must be in 1..CFZ_MAX_NBR"), (lambda: plan(D=-1), "D must not be negative"),
                       (lambda: plan(m=-1.0), "margin must be finite"), (lambda: plan(t=None), "null tables"),
                       (lambda: plan(r=-1), "slack must not be negative"), (lambda: plan(out=(None, None, None)), "null delays"),
                       (lambda: plan(cap=ptr(cap_bad)), "a cap lies outside"), (lambda: plan(D=215), "search space too large"),
                       (lambda: loop(D=-1), "D must not be negative"), (lambda: loop(m=float("nan")), "margin must be finite"),
                       (lambda: loop(r=-1), "slack must not be negative")):
        assert call() == -1 and text in lib.cfz_last_error().decode(), (text, lib.cfz_last_error().decode())
    assert (delays == 7).all() and (info == 7).all() and (rclear == 7.0).all()
    served = 0
    for call in (search, plan):
        rc = call()
        assert rc == (-1 if h is None else 0) and (h is not None or "null handle" in lib.cfz_last_error().decode())
        served += rc == 0
    return served
