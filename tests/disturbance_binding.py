"""The closed loop's disturbance streams, twice: a ctypes binding of the test-only CPU build of the kernel source
(tests/emu/cfz_disturb_emu.cpp over conflict_rez_amd/csrc/cfz_disturb.inl), and an independent numpy statement of the same definition
(Philox4x32-10, 53-bit uniforms, Box-Muller) that both the CPU build and the GPU kernels are checked against."""
import ctypes as C

import numpy as np

from emu_build import load, ptr

# the base sigma set of the tests: measurement (x, y, psi, v, delta), actuator (a, w), process (x, y, psi, v, delta)
SIGMA = dict(meas=(0.02, 0.02, 0.005, 0.02, 0.0), act=(0.05, 0.02), proc=(0.005, 0.005, 0.002, 0.01, 0.0))


def sigma12(meas=None, act=None, proc=None):
    return np.concatenate([np.zeros(5) if meas is None else np.asarray(meas, float), np.zeros(2) if act is None else np.asarray(act, float),
                           np.zeros(5) if proc is None else np.asarray(proc, float)])


_i, _d, _vp = C.c_int, C.c_double, C.c_void_p
PROTOTYPES = {  # of tests/emu/cfz_disturb_emu.cpp
    "cfz_emu_philox": (None, [_vp, _vp, _vp]),
    "cfz_emu_box_muller": (None, [_vp, _vp]),
    "cfz_emu_normals": (None, [C.c_long] + [_vp] * 6),
    "cfz_emu_disturbance": (None, [C.c_uint64, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "cfz_emu_disturb_add": (_d, [_d, _d]),
}


def lib():
    return load("cfz_disturb_emu", ("tests/emu/cfz_disturb_emu.cpp", "conflict_rez_amd/csrc/cfz_disturb.inl"), PROTOTYPES)


def emu_philox(ctr, key):
    ctr = np.ascontiguousarray(ctr, np.uint32); key = np.ascontiguousarray(key, np.uint32)
    out = np.empty(4, np.uint32)
    lib().cfz_emu_philox(ptr(ctr), ptr(key), ptr(out))
    return out


def emu_box_muller(words):
    w = np.ascontiguousarray(words, np.uint32)
    z = np.empty(2)
    lib().cfz_emu_box_muller(ptr(w), ptr(z))
    return z


def emu_normals(seed, stream, v, step):
    """Arrays [n] -> (words [n,6,4] uint32, z [n,12])."""
    seed = np.ascontiguousarray(seed, np.uint64); n = len(seed)
    stream, v, step = (np.ascontiguousarray(np.broadcast_to(a, n), np.uint32) for a in (stream, v, step))
    words, z = np.empty((n, 6, 4), np.uint32), np.empty((n, 12))
    lib().cfz_emu_normals(n, ptr(seed), ptr(stream), ptr(v), ptr(step), ptr(words), ptr(z))
    return words, z


def emu_disturbance(seed, sigma, level, stream, V, t0, K):
    sigma = np.ascontiguousarray(sigma, float); level = np.ascontiguousarray(level, float); stream = np.ascontiguousarray(stream, np.uint32)
    S = len(level)
    d = np.empty((K, S, V, 12))
    lib().cfz_emu_disturbance(C.c_uint64(int(seed)), ptr(sigma), ptr(level), ptr(stream), S, V, int(t0), int(K), ptr(d))
    return d


# ---- numpy statement -------------------------------------------------------------------------------------------------------------
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr [..., 4], key [..., 2] (any integer type, values below 2^32) -> [..., 4] uint32, in 64-bit arithmetic."""
    c = [np.asarray(ctr)[..., i].astype(np.uint64) for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) for i in range(2)]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & _MASK]
        k = [(k[0] + np.uint64(W0)) & _MASK, (k[1] + np.uint64(W1)) & _MASK]
    return np.stack(c, -1).astype(np.uint32)


def box_muller(words):
    """words [..., 4] uint32 -> z [..., 2]."""
    w = np.asarray(words).astype(np.uint64)
    u1 = (((w[..., 0] >> np.uint64(5)) << np.uint64(26)) + (w[..., 1] >> np.uint64(6)) + np.uint64(1)).astype(float) * 2.0 ** -53
    u2 = (((w[..., 2] >> np.uint64(5)) << np.uint64(26)) + (w[..., 3] >> np.uint64(6))).astype(float) * 2.0 ** -53
    r = np.sqrt(-2.0 * np.log(u1))
    return np.stack([r * np.cos(2 * np.pi * u2), r * np.sin(2 * np.pi * u2)], -1)


def words(seed, stream, v, step):
    """Broadcastable integer arrays -> words [..., 6, 4] of the six calls j = 0..5."""
    seed = np.asarray(seed, np.uint64)
    stream, v, step = (np.asarray(a).astype(np.uint64) for a in (stream, v, step))
    shp = np.broadcast_shapes(seed.shape, stream.shape, v.shape, step.shape)
    j = np.arange(6, dtype=np.uint64)
    ctr = np.stack(np.broadcast_arrays(*(np.broadcast_to(a, shp)[..., None] for a in (stream, v, step)), j), -1)  # [..., 6, 4]
    key = np.broadcast_to(np.stack([seed & _MASK, seed >> np.uint64(32)], -1)[..., None, :], ctr.shape[:-1] + (2,))
    return philox4x32_10(ctr, key)


def normals(seed, stream, v, step):
    """The twelve standard normals z [..., 12] of (seed, stream, v, step)."""
    w = words(seed, stream, v, step)
    return box_muller(w).reshape(w.shape[:-2] + (12,))


def disturbance(seed, sigma, level, stream, V, t0, K):
    """d [K, S, V, 12] of steps [t0, t0 + K): level_s * sigma_i * z_i, rounded after each product."""
    level = np.asarray(level, float); stream = np.asarray(stream)
    z = normals(np.uint64(int(seed)), stream[None, :, None], np.arange(V)[None, None, :], (t0 + np.arange(K))[:, None, None])
    return (level[None, :, None, None] * np.asarray(sigma, float)) * z
