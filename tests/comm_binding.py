"""The closed loop's lossy prediction exchange (`cfz_loop_set_comm`; conflict_rez_amd/csrc/cfz_comm.inl), stated a second time for the
tests: a ctypes binding of the test-only CPU build of the kernel source (tests/emu/cfz_comm_emu.cpp), an independent numpy statement
of the delivery bits on top of `disturbance_binding.philox4x32_10`, and the age rule in plain Python as a `Setting` that the host
replay (`oracle.closed_loop.replay(comm=...)`, which keeps the message history) asks which message and which rows a vehicle reads."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from disturbance_binding import philox4x32_10  # noqa: E402
from emu_build import load, ptr  # noqa: E402

MAX_AGE = 6  # CFZ_MAX_AGE
_i, _vp = C.c_int, C.c_void_p
PROTOTYPES = {  # of tests/emu/cfz_comm_emu.cpp
    "cfz_emu_max_age": (_i, []),
    "cfz_emu_delivered": (None, [C.c_long] + [_vp] * 8),
    "cfz_emu_comm": (None, [C.c_uint64, _vp, _vp, _i, _i, _i, _i, _vp]),
    "cfz_emu_age": (_i, [_vp, _i, _i, _i, _i]),
    "cfz_emu_age_drawn": (_i, [C.c_uint64, _vp, _vp] + [_i] * 6),
    "cfz_emu_want": (_i, [_i, _i]),
    "cfz_emu_slot": (_i, [_i, _i]),
    "cfz_emu_row": (_i, [_i] * 5),
}


def lib():
    return load("cfz_comm_emu", ("tests/emu/cfz_comm_emu.cpp", "conflict_rez_amd/csrc/cfz_comm.inl", "conflict_rez_amd/csrc/cfz_disturb.inl"), PROTOTYPES)


def emu_delivered(seed, stream, v, u, tau, p):
    """Arrays [n] -> (bit [n] bool, ctr [n,4] uint32: the Philox counter of each draw)."""
    seed = np.ascontiguousarray(seed, np.uint64); n = len(seed)
    stream = np.ascontiguousarray(np.broadcast_to(stream, n), np.uint32)
    v, u, tau = (np.ascontiguousarray(np.broadcast_to(a, n), np.int32) for a in (v, u, tau))
    p = np.ascontiguousarray(np.broadcast_to(p, n), float)
    bit, ctr = np.empty(n, np.int32), np.empty((n, 4), np.uint32)
    lib().cfz_emu_delivered(n, ptr(seed), ptr(stream), ptr(v), ptr(u), ptr(tau), ptr(p), ptr(bit), ptr(ctr))
    return bit.astype(bool), ctr


def emu_comm(seed, p_drop, stream, V, tau0, K):
    p_drop = np.ascontiguousarray(p_drop, float); stream = np.ascontiguousarray(stream, np.uint32)
    out = np.empty((K, len(p_drop), V, V), np.int32)
    lib().cfz_emu_comm(C.c_uint64(int(seed)), ptr(p_drop), ptr(stream), len(p_drop), V, int(tau0), int(K), ptr(out))
    return out.astype(bool)


def emu_age(bits, base, tau_star, max_age, tau_on):
    bits = np.ascontiguousarray(bits, np.int32)
    return lib().cfz_emu_age(ptr(bits), int(base), int(tau_star), int(max_age), int(tau_on))


def emu_age_drawn(seed, p_drop, stream, max_age, tau_on, s, v, u, tau_star):
    p_drop = np.ascontiguousarray(p_drop, float); stream = np.ascontiguousarray(stream, np.uint32)
    return lib().cfz_emu_age_drawn(C.c_uint64(int(seed)), ptr(p_drop), ptr(stream), int(max_age), int(tau_on), int(s), int(v), int(u), int(tau_star))


# ---- numpy statement of the delivery bits ------------------------------------------------------------------------------------------
def counters(stream, v, u, tau):
    """The Philox counter (stream, receiver, tau + 1, 8 + sender) of broadcastable integer arrays -> [..., 4] uint64."""
    a = np.broadcast_arrays(*(np.asarray(x).astype(np.int64) for x in (stream, v, np.asarray(tau).astype(np.int64) + 1, np.asarray(u).astype(np.int64) + 8)))
    return np.stack(a, -1).astype(np.uint64)


def u1_of(seed, stream, v, u, tau):
    """The first uniform of the draw, in (0, 1]: an exact 53-bit value."""
    ctr = counters(stream, v, u, tau)
    seed = np.broadcast_to(np.asarray(seed, np.uint64), ctr.shape[:-1])
    key = np.stack([seed & np.uint64(0xFFFFFFFF), seed >> np.uint64(32)], -1)
    w = philox4x32_10(ctr, key).astype(np.uint64)
    return (((w[..., 0] >> np.uint64(5)) << np.uint64(26)) + (w[..., 1] >> np.uint64(6)) + np.uint64(1)).astype(float) * 2.0 ** -53


def delivered_bits(seed, stream, v, u, tau, p):
    return u1_of(seed, stream, v, u, tau) > np.asarray(p, float)


def delivered(seed, p_drop, stream, V, tau0, K):
    """bool [K, S, V, V] of messages [tau0, tau0 + K): [k, s, v, u] is the bit of receiver v, sender u; the diagonal is True."""
    p_drop = np.asarray(p_drop, float); stream = np.asarray(stream)
    tau = (tau0 + np.arange(K))[:, None, None, None]
    b = delivered_bits(np.uint64(int(seed)), stream[None, :, None, None], np.arange(V)[None, None, :, None], np.arange(V)[None, None, None, :], tau,
                       p_drop[None, :, None, None])
    b = np.array(b)
    b[:, :, np.arange(V), np.arange(V)] = True
    return b


# ---- the age rule and the read row, in plain Python --------------------------------------------------------------------------------
def want(t, earlier):
    """The message a vehicle wants of a neighbour in iteration t: t - 1, or t of a neighbour ranked before it (sequential exchange)."""
    return t if earlier else t - 1


def age_rule(bit, tau_star, max_age, tau_on):
    """Smallest a >= 0 with bit(tau_star - a), or min(max_age, tau_star - tau_on): the message tau_on counts as delivered, and so does
    one of age max_age."""
    a_eff = min(max_age, tau_star - tau_on)
    for a in range(a_eff):
        if bit(tau_star - a):
            return a
    return a_eff


def rows(N, fresh, compensate, a):
    return np.minimum(np.arange(N) + fresh + (a if compensate else 0), N - 1)


class Setting:
    """A comm setting of the replay.  bits [T, S, V, V] (bool, indexed by the message number tau from 0; `Engine.loop_comm(0, T)`) or
    age: a function (t, s, v, u, earlier) -> the age outright; tau_on: the message history starts at."""

    def __init__(self, max_age, compensate, tau_on, bits=None, age=None):
        self.max_age, self.compensate, self.tau_on, self.bits, self.age = int(max_age), bool(compensate), int(tau_on), bits, age

    def age_of(self, t, s, v, u, earlier):
        if self.age is not None:
            return self.age(t, s, v, u, earlier)
        return age_rule(lambda tau: bool(self.bits[tau, s, v, u]), want(t, earlier), self.max_age, self.tau_on)

    def read(self, t, s, v, u, earlier, N):
        """What the replay asks: (the message tau vehicle v takes of neighbour u in iteration t, the rows [N] it reads of it)."""
        a = self.age_of(t, s, v, u, earlier)
        return want(t, earlier) - a, rows(N, 0 if earlier else 1, self.compensate, a)
