"""The coordination diagrams and the hold-point schedules of a plan pool, twice: a ctypes binding of the test-only CPU build of the kernel
sources (tests/emu/cfz_schedule_emu.cpp over conflict_rez_amd/csrc/cfz_coord.inl and cfz_schedule.inl, the wavefronts that take the orders
an argument), and independent Python statements of the definitions of include/confrez_hip.h ("coordination diagrams and hold-point
schedules"): the diagram from audit_binding.signed_distance < margin, every entry on its own, and the schedule from sets of (sample, time)
nodes -- what can be reached from (0, 0), what can reach (goal, H-1), the largest sample in both at every step: no bits, no shifted words,
no walk back -- that both the CPU build and the GPU kernels are checked against.  Also the plans and the cases both test modules use."""
import ctypes as C
import functools
import itertools

import numpy as np

import audit_binding as ab
import conflict_binding as cb
from conflict_binding import pairs
from emu_build import load, ptr

G, MARGIN, TIE = cb.G, cb.MARGIN, 1e-12
OUT = ("schedule", "arrival", "waits", "found", "order", "makespan", "total", "feasible_orders")


_i, _vp = C.c_int, C.c_void_p
PROTOTYPES = {  # of tests/emu/cfz_schedule_emu.cpp
    "cfz_emu_schedule_lds_bytes": (_i, []),
    "cfz_emu_schedule_wave_words": (_i, [_i, _i, _i]),
    "cfz_emu_plan_coordination": (_i, [_i, _i, _i, _vp, _vp, _vp, C.c_double, _vp]),
    "cfz_emu_plan_schedule": (_i, [_i, _i, _i, _vp, _vp, _vp, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp]),
}


def lib():
    return load("cfz_schedule_emu", ["tests/emu/cfz_schedule_emu.cpp", "tests/emu/emu_columns.h"]
                + ["conflict_rez_amd/csrc/" + f for f in ("cfz_schedule.inl", "cfz_coord.inl", "cfz_conflict.inl", "cfz_audit.inl", "cfz_wave.inl")], PROTOTYPES)


def all_orders(V):
    return np.array(list(itertools.permutations(range(V))), np.int32)


def history_in_lds(V, T, H):
    """Whether schedule_kernel keeps the four wavefronts' rows and schedules of this shape in LDS (else: in global memory)."""
    return 4 * 4 * int(lib().cfz_emu_schedule_wave_words(V, T, H)) <= int(lib().cfz_emu_schedule_lds_bytes())


def lds_edge():
    """The longest horizon whose rows and schedules schedule_kernel keeps in LDS at V = 2, T = 65: 4 H words per wavefront, 64 H bytes."""
    H = int(lib().cfz_emu_schedule_lds_bytes()) // 64
    assert history_in_lds(2, 65, H) and not history_in_lds(2, 65, H + 1)
    return H


def _lengths(length, P, V, T):
    return np.full((P, V), T, np.int32) if length is None else np.ascontiguousarray(np.broadcast_to(np.asarray(length, np.int32), (P, V)))


def unpack(words, T):
    """Rows of 32-bit words [..., nw] -> bool [..., T]."""
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=-1, bitorder="little")[..., :T].astype(bool)


def pack(bits):
    """bool [..., T] -> rows of 32-bit words [..., (T + 31) // 32]."""
    T = bits.shape[-1]
    pad = np.zeros(bits.shape[:-1] + (32 * ((T + 31) // 32),), np.uint8)
    pad[..., :T] = bits
    return np.ascontiguousarray(np.packbits(pad, axis=-1, bitorder="little")).view(np.uint32)


def emu_diagram(tables, margin=MARGIN, length=None, g=G):
    """The CPU build -> both sides as the kernel writes them, bool [P, npair, 2, T, T]: [:, :, 0, i, j] and [:, :, 1, j, i] are B[i][j]."""
    tables = np.ascontiguousarray(tables, float)
    if tables.ndim == 3:
        tables = tables[None]
    P, V, T = tables.shape[:3]
    length = None if length is None else _lengths(length, P, V, T)
    words = np.full((P, V * (V - 1) // 2, 2, T, (T + 31) // 32), 0xDEADBEEF, np.uint32)
    assert lib().cfz_emu_plan_coordination(P, V, T, ptr(tables), ptr(length), ptr(np.ascontiguousarray(g, float)), margin, ptr(words)) == 0
    return unpack(words, T)


def emu_schedule_diagram(sides, hold, H, slack=0, orders=None, length=None, waves=4):
    """The CPU build of the search over given diagrams sides [P, npair, 2, T, T] (emu_diagram's, or any) -> the dict of Engine.plan_schedule."""
    P, npair, _, T, _ = sides.shape
    V = int(round((1 + (1 + 8 * npair) ** 0.5) / 2))
    words = pack(sides)
    hold = np.ascontiguousarray(np.broadcast_to(np.asarray(hold) != 0, (P, V, T)), dtype=np.uint8)
    orders = all_orders(V) if orders is None else np.ascontiguousarray(np.atleast_2d(orders), dtype=np.int32)
    length = None if length is None else _lengths(length, P, V, T)
    sch, arr, wts, info = np.full((P, V, H), -7, np.int32), np.full((P, V), -7, np.int32), np.full((P, V), -7, np.int32), np.full((P, 5), -7, np.int32)
    rc = lib().cfz_emu_plan_schedule(P, V, T, ptr(words), ptr(length), ptr(hold), H, slack, len(orders), ptr(orders), waves, ptr(sch), ptr(arr), ptr(wts), ptr(info))
    assert rc == 0, rc
    return dict(schedule=sch, arrival=arr, waits=wts, found=info[:, 0] == 1, order=info[:, 1], makespan=info[:, 2], total=info[:, 3], feasible_orders=info[:, 4])


def emu_schedule(tables, hold, H, margin=MARGIN, slack=0, orders=None, length=None, waves=4):
    return emu_schedule_diagram(emu_diagram(tables, margin, length), hold, H, slack, orders, length, waves)


# ---- statements --------------------------------------------------------------------------------------------------------------
def diagram(tables, margin=MARGIN, length=None, g=G):
    """B[P, npair, T, T] from its definition, and near[P, npair, T, T]: where the distance lies within TIE of the margin."""
    tables = np.asarray(tables, float)
    if tables.ndim == 3:
        tables = tables[None]
    P, V, T = tables.shape[:3]
    n = _lengths(length, P, V, T)
    W = ab.body(g, tables[..., 0], tables[..., 1], tables[..., 2])  # [P, V, T, 4, 2]
    B, near = np.zeros((P, V * (V - 1) // 2, T, T), bool), np.zeros((P, V * (V - 1) // 2, T, T), bool)
    for p in range(P):
        for q, (u, w) in enumerate(pairs(V)):
            lu, lw = n[p, u], n[p, w]
            d = ab.signed_distance(W[p, u, :lu, None], W[p, w, None, :lw])
            B[p, q, :lu, :lw], near[p, q, :lu, :lw] = d < margin, np.abs(d - margin) <= TIE
    return B, near


def _vehicle(g, holdable, blocked_at, H):
    """The smallest arrival and the pointwise largest schedule of one vehicle with goal sample g, from sets of nodes.  holdable: set of
    samples; blocked_at[t]: set of samples it must not be at at step t.  -> (arrival, [s(0) .. s(H-1)]) or None."""
    reach = [set() for _ in range(H)]
    if 0 not in blocked_at[0]:
        reach[0].add(0)
    for t in range(1, H):
        bad = blocked_at[t]
        reach[t] = {i for i in reach[t - 1] if i in holdable and i not in bad} | {i + 1 for i in reach[t - 1] if i < g and i + 1 not in bad}
    live = [set() for _ in range(H)]
    live[H - 1] = reach[H - 1] & {g}
    for t in range(H - 2, -1, -1):
        nxt = live[t + 1]
        live[t] = {i for i in reach[t] if (i in nxt and i in holdable) or i + 1 in nxt}
    if not live[0]:
        return None
    s = [max(n) for n in live]
    return s.index(g), s


def schedule_set(B, length, hold, H, slack, orders):
    """One plan set from the definitions: B [npair, T, T] bool, length [V], hold [V, T] -> (schedule [V, H], arrival, waits, info[5])."""
    V, T = hold.shape
    pr = pairs(V)
    best, feasible, cache = None, 0, {}
    for oi, pi in enumerate(orders):
        pi = tuple(int(v) for v in pi)
        res = {}
        for k, v in enumerate(pi):
            key = pi[: k + 1]  # a vehicle's schedule depends on the vehicles before it and on nothing else
            if key not in cache:
                g = int(length[v]) - 1
                bad = np.zeros((T, H), bool)  # [sample of v, step]
                for e in pi[:k]:
                    se = np.asarray(res[e][1])
                    for d in range(-slack, slack + 1):
                        at = se[np.clip(np.arange(H) + d, 0, H - 1)]
                        bad |= B[pr.index((v, e))][:, at] if v < e else B[pr.index((e, v))][at, :].T
                holdable = set(np.flatnonzero(hold[v, : g + 1]).tolist()) | {g}
                cache[key] = _vehicle(g, holdable, [set(np.flatnonzero(bad[:, t]).tolist()) for t in range(H)], H)
            if cache[key] is None:
                res = None
                break
            res[v] = cache[key]
        if res is None:
            continue
        feasible += 1
        cand = (max(res[v][0] for v in range(V)), sum(res[v][0] for v in range(V)), oi)
        if best is None or cand < best[0]:
            best = (cand, res)
    if best is None:
        return np.full((V, H), -1, np.int32), np.full(V, -1, np.int32), np.full(V, -1, np.int32), np.array([0, -1, -1, -1, 0], np.int32)
    (mk, tot, oi), res = best
    arr = np.array([res[v][0] for v in range(V)], np.int32)
    sch = np.array([res[v][1] for v in range(V)], np.int32)
    waits = np.array([sum(1 for t in range(arr[v]) if sch[v, t + 1] == sch[v, t]) for v in range(V)], np.int32)
    return sch, arr, waits, np.array([1, oi, mk, tot, feasible], np.int32)


def schedule(B, hold, H, slack=0, orders=None, length=None):
    """The statement on P sets: B [P, npair, T, T] -> the dict of Engine.plan_schedule."""
    P, npair, T, _ = B.shape
    V = int(round((1 + (1 + 8 * npair) ** 0.5) / 2))
    hold = np.broadcast_to(np.asarray(hold) != 0, (P, V, T))
    n = _lengths(length, P, V, T)
    orders = all_orders(V) if orders is None else np.atleast_2d(orders)
    rows = [schedule_set(B[p], n[p], hold[p], H, slack, orders) for p in range(P)]
    sch, arr, wts, info = (np.stack([r[i] for r in rows]) for i in range(4))
    return dict(schedule=sch, arrival=arr, waits=wts, found=info[:, 0] == 1, order=info[:, 1], makespan=info[:, 2], total=info[:, 3], feasible_orders=info[:, 4])


def same(a, b, what=OUT):
    """Every integer of two results equal; -> True so that it can stand in an assert."""
    for k in what:
        assert np.array_equal(a[k], b[k]), (k, np.asarray(a[k]).tolist(), np.asarray(b[k]).tolist())
    return True


def check_schedules(out, B, hold, H, slack, length=None):
    """What a result promises, checked directly: every found schedule starts at 0, moves by 0 or 1, rests only where it may, ends at
    its goal, and the set is conflict-free with the slack; arrival, waits, makespan and total are what the schedule says."""
    P, npair, T, _ = B.shape
    V = out["schedule"].shape[1]
    hold = np.broadcast_to(np.asarray(hold) != 0, (P, V, T))
    n = _lengths(length, P, V, T)
    for p in np.flatnonzero(out["found"]):
        s = out["schedule"][p]
        for v in range(V):
            g = n[p, v] - 1
            step = np.diff(s[v])
            assert s[v, 0] == 0 and s[v, -1] == g and set(step.tolist()) <= {0, 1}
            rest = s[v, :-1][step == 0]
            assert (hold[p, v, rest] | (rest == g)).all()
            assert out["arrival"][p, v] == int(np.argmax(s[v] == g)) and out["waits"][p, v] == out["arrival"][p, v] - g
        assert out["makespan"][p] == out["arrival"][p].max() and out["total"][p] == out["arrival"][p].sum()
        for q, (u, w) in enumerate(pairs(V)):
            for d in range(-slack, slack + 1):
                tt = np.clip(np.arange(H) + d, 0, H - 1)
                assert not B[p, q][s[u], s[w, tt]].any() and not B[p, q][s[u, tt], s[w]].any()
    return True


# ---- plans, masks and cases --------------------------------------------------------------------------------------------------
SEED = 2  # of the crossing plans: chosen so that no distance of any case lies within TIE of the margin (the host tests assert it)


@functools.lru_cache(maxsize=None)
def crossing(P, V, T, seed=0):
    """P sets of V plans of T samples that cross one yard: every vehicle starts 6 to 10 m from the centre, heads for it along a gently
    curved line, passes it near the middle of its plan and ends as far out on the other side, so that the bodies (3.9 m x 1.8 m) meet
    near the centre and a vehicle that waits lets another one through.  Columns 3: are filled with numbers nothing may read.  Shared, not
    to be written to."""
    rng = np.random.default_rng([seed, P, V, T, 17])
    th = rng.uniform(-np.pi, np.pi, (P, V, 1))
    R = rng.uniform(6.0, 10.0, (P, V, 1))
    step = 2.0 * R / max(T - 1, 1) * rng.uniform(0.9, 1.2, (P, V, 1))
    k = np.arange(T)[None, None, :]
    psi = th + rng.uniform(-0.3, 0.3, (P, V, 1)) * (k / max(T - 1, 1) - 0.5)
    tab = np.empty((P, V, T, 7))
    tab[..., 2] = psi
    tab[..., 0] = 15.0 - R[..., 0:1] * np.cos(th) + np.cumsum(step * np.cos(psi), -1) - step * np.cos(psi[..., :1])
    tab[..., 1] = 15.0 - R[..., 0:1] * np.sin(th) + np.cumsum(step * np.sin(psi), -1) - step * np.sin(psi[..., :1])
    tab[..., 3:] = rng.uniform(-50.0, 50.0, (P, V, T, 4))
    tab.setflags(write=False)
    return tab


def random_hold(P, V, T, seed=0, rho=0.2, first=0.7):
    """Random hold masks: a sample with probability rho, sample 0 with probability `first`."""
    rng = np.random.default_rng([seed, P, V, T, 11])
    hold = rng.random((P, V, T)) < rho
    hold[:, :, 0] = rng.random((P, V)) < first
    return hold.astype(np.uint8)


def random_lengths(P, V, T, seed=0):
    rng = np.random.default_rng([seed, P, V, T, 13])
    return rng.integers(max(1, T // 2), T + 1, (P, V)).astype(np.int32)


def crafted():
    """Three hand-made sets of two vehicles, T = 44, margin MARGIN -> (tables [3, 2, 44, 7], length [3, 2], hold [3, 2, 44]).
    Set 0: vehicle 0 drives north along x = 16 through the spot where vehicle 1, coming from the west along y = 10 in 13 samples, parks.
      Vehicle 1 first: it parks in vehicle 0's way for good, the order is infeasible.  Vehicle 0 first: vehicle 1 could be at its goal
      early (steps 12 .. 23 are free there), is shut out of it while vehicle 0 passes, and may come back afterwards: its arrival is the
      start of the LAST run of free steps at the goal, and it waits at its first sample, the only one it may hold.
    Set 1: both start on the same spot: blocked at step 0, nothing is feasible.
    Set 2: far apart: every order is feasible without a wait."""
    T = 44
    tab = np.zeros((3, 2, T, 7))
    tab[..., 3:] = 1.0
    k = np.arange(T)
    tab[0, 0, :, 0], tab[0, 0, :, 1], tab[0, 0, :, 2] = 16.0, -6.0 + 0.5 * k, np.pi / 2
    kb = np.minimum(k, 12)
    tab[0, 1, :, 0], tab[0, 1, :, 1], tab[0, 1, :, 2] = 10.0 + 0.5 * kb, 10.0, 0.0
    tab[1, 0, :, 0], tab[1, 0, :, 1] = 12.0 + 0.3 * k, 12.0
    tab[1, 1, :, 0], tab[1, 1, :, 1], tab[1, 1, :, 2] = 12.5, 12.0 + 0.3 * k, np.pi / 2
    tab[2, 0, :, 0], tab[2, 0, :, 1] = 5.0 + 0.2 * k, 5.0
    tab[2, 1, :, 0], tab[2, 1, :, 1] = 5.0 + 0.2 * k, 25.0
    length = np.array([[T, 13], [T, T], [T, 30]], np.int32)
    hold = np.zeros((3, 2, T), np.uint8)
    hold[:, :, 0] = 1
    return tab, length, hold


# name: (P, V, T, H, slack, orders (None: all), unequal lengths).  T = 1: parked vehicles, H = T; 31 / 32 / 33 and 64 / 65: the carry across
# a word and a lane, a row of one ballot and of one more; H no multiple of anything; V = 8 with 5 orders (no multiple of the four
# wavefronts); O = 1; slack 0 and 2; the rows of one order just inside LDS and just outside ("edge": lds_edge(), the
# longest horizon that fits at V = 2, T = 65).
_O8 = np.array([np.roll(np.arange(8), i) for i in range(4)] + [np.arange(8)[::-1]], np.int32)
CASES = {
    "t1": (5, 2, 1, 1, 0, None, False),
    "t31_v3": (3, 3, 31, 53, 0, None, False),
    "t32_v2_r2": (4, 2, 32, 47, 2, None, True),
    "t33_v4": (2, 4, 33, 71, 0, None, True),
    "t64_v3_r2": (2, 3, 64, 101, 2, None, False),
    "t65_v4": (2, 4, 65, 97, 0, None, True),
    "t65_v2_o1": (4, 2, 65, 65, 0, np.array([[1, 0]], np.int32), False),
    "t40_v8_o5": (2, 8, 40, 79, 0, _O8, True),
    "t65_lds_edge": (1, 2, 65, "edge", 0, None, True),
    "t65_global": (1, 2, 65, "edge+1", 2, None, True),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(tables, hold, length, H, slack, orders, B, near, reference) of a case: the statements computed once, shared by the tests of both
    modules, not to be written to."""
    P, V, T, H, slack, orders, unequal = CASES[name]
    H = lds_edge() + (H == "edge+1") if isinstance(H, str) else H
    tables = crossing(P, V, T, SEED)
    hold = random_hold(P, V, T, SEED)
    length = random_lengths(P, V, T, SEED) if unequal else None
    B, near = diagram(tables, MARGIN, length)
    ref = schedule(B, hold, H, slack, orders, length)
    for a in (tables, hold, B, near) + tuple(ref.values()) + (() if length is None else (length,)):
        a.setflags(write=False)
    return tables, hold, length, H, slack, orders, B, near, ref


@functools.lru_cache(maxsize=None)
def crafted_reference(H=77, slack=0):
    tab, length, hold = crafted()
    B, near = diagram(tab, MARGIN, length)
    return B, near, schedule(B, hold, H, slack, None, length)


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def check_refusals(lib, h):
    """Every refusal of the three C entry points that needs no handle: -1, the text names the cause, the outputs stay unwritten.  Calls
    that pass those checks are refused for the null handle where h is None (the loop form: for the missing loop_init) and served
    otherwise.  -> the number of calls that were served."""
    P, V, T, H = 2, 3, 40, 50
    tab = np.ascontiguousarray(cb.synthetic(P, V, T, SEED))
    hold, orders = random_hold(P, V, T), all_orders(V)
    sch, arr, wts, info = np.full((P, V, H), 7, np.int32), np.full((P, V), 7, np.int32), np.full((P, V), 7, np.int32), np.full((P, 5), 7, np.int32)
    blk = np.full((P, 3, T, 2), 7, np.uint32)
    bad_len, bad_len0 = np.array([[40, 41, 40]] * 2, np.int32), np.array([[40, 0, 40]] * 2, np.int32)
    bad_ord, bad_ord2 = np.array([[0, 1, 1]], np.int32), np.array([[0, 1, 3]], np.int32)

    def plan(P=P, V=V, T=T, t=ptr(tab), n=None, hd=ptr(hold), H=H, m=0.05, r=0, O=6, o=ptr(orders), s=ptr(sch)):
        return lib.cfz_plan_schedule(h, P, V, T, t, n, hd, H, m, r, O, o, s, ptr(arr), ptr(wts), ptr(info))

    def coord(P=P, V=V, T=T, t=ptr(tab), n=None, m=0.05, b=ptr(blk)):
        return lib.cfz_plan_coordination(h, P, V, T, t, n, m, b)

    def loop(m=0.05, r=0):
        return lib.cfz_loop_plan_schedule(h, None, ptr(hold), H, m, r, 6, ptr(orders), ptr(sch), ptr(arr), ptr(wts), ptr(info))

    for call, text in ((lambda: plan(P=0), "P, T must be positive"), (lambda: plan(T=0), "P, T must be positive"),
                       (lambda: plan(V=0), "V must be in 1..CFZ_MAX_NBR"), (lambda: plan(V=9), "V must be in 1..CFZ_MAX_NBR"),
                       (lambda: plan(m=-1.0), "margin must be finite"), (lambda: plan(m=float("nan")), "margin must be finite"),
                       (lambda: plan(t=None), "null tables"), (lambda: plan(n=ptr(bad_len)), "a length lies outside"),
                       (lambda: plan(n=ptr(bad_len0)), "a length lies outside"), (lambda: plan(H=0), "H, O must be positive"),
                       (lambda: plan(O=0), "H, O must be positive"), (lambda: plan(H=39), "H must not be below T"),
                       (lambda: plan(T=2049, H=2049), "T must not exceed CFZ_SCHEDULE_MAX_T"),
                       (lambda: plan(H=32769), "H must not exceed CFZ_SCHEDULE_MAX_H"), (lambda: plan(r=-1), "slack must not be negative"),
                       (lambda: plan(hd=None), "null hold"), (lambda: plan(o=None), "null orders"), (lambda: plan(s=None), "null schedule"),
                       (lambda: plan(O=1, o=ptr(bad_ord)), "an order is not a permutation"),
                       (lambda: plan(O=1, o=ptr(bad_ord2)), "an order is not a permutation"),
                       (lambda: plan(P=30000, H=32768), "schedule too large"),
                       (lambda: coord(P=0), "P, T must be positive"), (lambda: coord(V=9), "V must be in 1..CFZ_MAX_NBR"),
                       (lambda: coord(m=float("inf")), "margin must be finite"), (lambda: coord(t=None), "null tables"),
                       (lambda: coord(b=None), "null blocked"), (lambda: coord(n=ptr(bad_len)), "a length lies outside"),
                       (lambda: loop(m=-0.1), "margin must be finite"), (lambda: loop(r=-1), "slack must not be negative")):
        assert call() == -1 and text in lib.cfz_last_error().decode(), (text, lib.cfz_last_error().decode())
    assert (sch == 7).all() and (arr == 7).all() and (wts == 7).all() and (info == 7).all() and (blk == 7).all()
    served = 0
    for call in (plan, coord):
        rc = call()
        assert rc == (-1 if h is None else 0) and (h is not None or "null handle" in lib.cfz_last_error().decode())
        served += rc == 0
    return served
