"""The conflict map of a plan pool, twice: a ctypes binding of the test-only CPU build of the kernel source
(tests/emu/cfz_conflict_emu.cpp over conflict_rez_amd/csrc/cfz_conflict.inl, the lanes per lag as an argument), and an independent numpy
statement of the definitions of include/confrez_hip.h ("conflict map of a set of plans") over audit_binding.body / signed_distance -- one
(set, pair, lag) at a time, no columns, no keys, no merges -- that both the CPU build and the GPU kernel are checked against.  Also the
synthetic plans and the comparison rule both test modules use."""
import ctypes as C
import functools

import numpy as np

import audit_binding as ab
from emu_build import load, ptr

_i, _d, _vp = C.c_int, C.c_double, C.c_void_p
PROTOTYPES = {  # of tests/emu/cfz_conflict_emu.cpp
    "cfz_emu_conflict_lds_t": (_i, []),
    "cfz_emu_plan_conflicts": (_i, [_i, _i, _i, _vp, _vp, _i, _d, _i, _vp, _vp]),
}

G = (3.3, 0.9, 0.6, 0.9)  # the default body (front, left, rear, right)
MARGIN = 0.05             # the default dmin
TIE = 1e-12
# (V, T, D): no lag at all; a window wider than the plan (every index clamped); steps no multiple of 64 and lags no multiple of 4;
# exactly one round of the lanes; one step more than a round with the widest window
SHAPES = ((2, 5, 0), (2, 5, 7), (3, 70, 7), (4, 64, 3), (4, 65, 40))
PS = (1, 3)
INTS = ("when", "first", "count")


def lib():
    return load("cfz_conflict_emu", ["tests/emu/cfz_conflict_emu.cpp", "tests/emu/emu_columns.h"] + ["conflict_rez_amd/csrc/" + f for f in ("cfz_conflict.inl", "cfz_audit.inl", "cfz_wave.inl")],
                PROTOTYPES)


def lds_t():
    """The longest plan that conflict_kernel stages in LDS."""
    return int(lib().cfz_emu_conflict_lds_t())


def pairs(V):
    return [(u, w) for u in range(V) for w in range(u + 1, V)]


def emu_conflicts(tables, D, margin=MARGIN, g=G, lanes=64):
    """The CPU build with `lanes` lanes per lag -> dict(clear, when, first, count [P, npair, 2D+1])."""
    tables = np.ascontiguousarray(tables, float)
    if tables.ndim == 3:
        tables = tables[None]
    P, V, T = tables.shape[:3]
    g = np.ascontiguousarray(g, float)
    npair = V * (V - 1) // 2
    clear, info = np.empty((P, npair, 2 * D + 1)), np.empty((P, npair, 2 * D + 1, 3), np.int32)
    assert lib().cfz_emu_plan_conflicts(P, V, T, ptr(tables), ptr(g), D, margin, lanes, ptr(clear), ptr(info)) == 0
    return dict(clear=clear, when=info[..., 0], first=info[..., 1], count=info[..., 2])


# ---- numpy statement ---------------------------------------------------------------------------------------------------------
def lag_indices(T, tau):
    """(iu, iw) [T + |tau|]: the sample of either vehicle of a pair at every step of lag tau."""
    i = np.arange(T + abs(tau))
    return np.clip(i - max(-tau, 0), 0, T - 1), np.clip(i - max(tau, 0), 0, T - 1)


def conflicts(tables, D, margin=MARGIN, g=G):
    """clear, when, first, count from their definitions, and where the comparison rule has to exempt an integer:
    tie_when: a second step, at other poses, comes within TIE of the minimum (steps at the very same poses -- both vehicles waiting or
    parked -- have the very same distance in every implementation, and the lowest of them is `when` in all);
    tie_margin: some d_i lies within TIE of the margin."""
    tables = np.asarray(tables, float)
    if tables.ndim == 3:
        tables = tables[None]
    P, V, T = tables.shape[:3]
    W = ab.body(g, tables[..., 0], tables[..., 1], tables[..., 2])  # [P, V, T, 4, 2]
    pr = pairs(V)
    sh = (P, len(pr), 2 * D + 1)
    out = dict(clear=np.empty(sh), when=np.empty(sh, np.int32), first=np.empty(sh, np.int32), count=np.empty(sh, np.int32),
               tie_when=np.zeros(sh, bool), tie_margin=np.zeros(sh, bool))
    idx = [lag_indices(T, tau) for tau in range(-D, D + 1)]
    IU, IW = np.concatenate([i[0] for i in idx]), np.concatenate([i[1] for i in idx])
    cut = np.cumsum([0] + [len(i[0]) for i in idx])
    for p in range(P):
        for q, (u, w) in enumerate(pr):
            dd = ab.signed_distance(W[p, u, IU], W[p, w, IW])  # every step of every lag of the pair in one call
            for j, (iu, iw) in enumerate(idx):
                d = dd[cut[j] : cut[j + 1]]
                pose = np.concatenate([tables[p, u, iu, :3], tables[p, w, iw, :3]], 1)
                k = int(np.argmin(d))
                k = int(np.flatnonzero((pose == pose[k]).all(1))[0])  # the lowest step at those poses, whatever numpy's last bits say
                below = np.flatnonzero(d < margin)
                o = (p, q, j)
                out["clear"][o], out["when"][o] = d[k], k
                out["first"][o], out["count"][o] = (below[0] if len(below) else -1), len(below)
                out["tie_when"][o] = ((d - d[k] <= TIE) & (pose != pose[k]).any(1)).any()
                out["tie_margin"][o] = (np.abs(d - margin) <= TIE).any()
    return out


def check_against_statement(out, ref):
    """The project's rule: distances within 1e-12 of the numpy statement (a distance is a few products and sums of coordinates below
    100 m and one root: its rounding error is of the order 1e-14), integers equal; `when` is exempt where the statement has a near tie
    of the minimum, `first` and `count` where it has a distance within 1e-12 of the margin.  -> the number of entries exempted, which
    every test asserts to be 0: the plans are chosen so that the statement has no near tie."""
    assert out["clear"].shape == ref["clear"].shape
    assert (np.abs(out["clear"] - ref["clear"]) <= 1e-12).all(), np.abs(out["clear"] - ref["clear"]).max()
    assert np.array_equal(out["when"][~ref["tie_when"]], ref["when"][~ref["tie_when"]]), np.argwhere((out["when"] != ref["when"]) & ~ref["tie_when"])[:5]
    for n in ("first", "count"):
        assert np.array_equal(out[n][~ref["tie_margin"]], ref[n][~ref["tie_margin"]]), (n, np.argwhere((out[n] != ref[n]) & ~ref["tie_margin"])[:5])
    return int(ref["tie_when"].sum() + ref["tie_margin"].sum())


# ---- synthetic plans ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def synthetic(P, V, T, seed=0):
    """P sets of V smooth random plans of T samples in a 9 m x 9 m yard: every vehicle starts at a random pose and drives 0.05 to 0.3 m
    per sample along a heading that turns by a slowly varying rate, so that bodies (3.9 m x 1.8 m) meet, part and pass at a distance
    at different lags.  Columns 3: are filled with numbers the conflict map must not read.  Shared, not to be written to."""
    rng = np.random.default_rng([seed, P, V, T])
    tab = np.empty((P, V, T, 7))
    step = rng.uniform(0.05, 0.3, (P, V, 1)) * (1 + 0.3 * np.sin(np.arange(T) * rng.uniform(0.05, 0.3, (P, V, 1)) + rng.uniform(0, 6, (P, V, 1))))
    rate = rng.uniform(-0.06, 0.06, (P, V, 1)) + 0.03 * np.sin(np.arange(T) * rng.uniform(0.02, 0.2, (P, V, 1)) + rng.uniform(0, 6, (P, V, 1)))
    psi = rng.uniform(-np.pi, np.pi, (P, V, 1)) + np.cumsum(rate, -1)
    tab[..., 2] = psi
    tab[..., 0] = rng.uniform(10.0, 19.0, (P, V, 1)) + np.cumsum(step * np.cos(psi), -1)
    tab[..., 1] = rng.uniform(10.0, 19.0, (P, V, 1)) + np.cumsum(step * np.sin(psi), -1)
    tab[..., 3:] = rng.uniform(-50.0, 50.0, (P, V, T, 4))
    tab.setflags(write=False)
    return tab


@functools.lru_cache(maxsize=None)
def packaged_pool():
    """The pool of three packaged plan sets of tests/test_scenario_loop_gpu.py (_three_tables): the warm-start table, the planned table
    and the planned table from its sample 20 on, each held at its last sample to the common length.  Shared, not to be written to."""
    from conflict_rez_amd import scenarios

    ws, _ = scenarios.load_reference_table(kind="state_ws")
    pl, _ = scenarios.load_reference_table(kind="planned")
    tabs = [ws, pl, pl[:, 20:]]
    T = max(t.shape[1] for t in tabs)
    pool = np.stack([np.concatenate([t, np.repeat(t[:, -1:], T - t.shape[1], axis=1)], 1) for t in tabs])
    pool.setflags(write=False)
    return pool


@functools.lru_cache(maxsize=None)
def packaged_reference(D):
    """The numpy statement on packaged_pool(): computed once."""
    out = conflicts(packaged_pool(), D)
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def synthetic_reference(P, V, T, D):
    """The numpy statement on synthetic(P, V, T): computed once, shared by the tests of both modules."""
    out = conflicts(synthetic(P, V, T), D)
    for a in out.values():
        a.setflags(write=False)
    return out
