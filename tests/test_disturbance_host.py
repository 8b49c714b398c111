"""The disturbance streams of the closed loop (conflict_rez_amd/csrc/cfz_disturb.inl) on the host: the CPU build of the kernel source
(tests/emu/cfz_disturb_emu.cpp) against Random123's published vectors of Philox4x32-10, against the numpy statement of the
definition in tests/disturbance_binding.py, and the moments of what it draws."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import disturbance_binding as db  # noqa: E402


def _hex(s):
    return np.array([int(w, 16) for w in s.split()], np.uint32)


KAT = [  # Random123 kat_vectors, philox4x32 10: counter, key, output
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


def test_philox_known_answers():
    """(1) The three published vectors through the CPU build of the kernel source, and through the numpy statement."""
    for ctr, key, out in KAT:
        assert np.array_equal(db.emu_philox(_hex(ctr), _hex(key)), _hex(out)), ctr
        assert np.array_equal(db.philox4x32_10(_hex(ctr), _hex(key)), _hex(out)), ctr


def test_variates_against_the_numpy_statement():
    """(2) The twelve variates of 10^4 random (seed, stream, v, step): words equal, z within 1e-13 (libm against numpy: a few ulp at
    |z| < 9)."""
    rng = np.random.default_rng(7)
    n = 10_000
    seed = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    stream = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    v = rng.integers(0, 8, n).astype(np.uint32)
    step = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    seed[0], stream[0], v[0], step[0] = 0, 0, 0, 0
    seed[1], stream[1], step[1] = 2 ** 64 - 1, 2 ** 32 - 1, 2 ** 32 - 1
    words, z = db.emu_normals(seed, stream, v, step)
    assert np.array_equal(words, db.words(seed, stream, v, step))
    ref = db.normals(seed, stream, v, step)
    assert np.isfinite(z).all()
    dev = float(np.abs(z - ref).max())
    print(f"max |z(CPU build) - z(numpy)| over {n} x 12 variates: {dev:.2e}")
    assert dev <= 1e-13
    # the disturbance is level * sigma * z, rounded after each product: equal to the numpy statement of the same two products where z is
    sigma = db.sigma12(**db.SIGMA)
    level = np.array([0.0, 0.5, 1.0, 2.0])
    d = db.emu_disturbance(2024, sigma, level, np.array([3, 3, 3, 9]), 4, 5, 3)
    dref = db.disturbance(2024, sigma, level, np.array([3, 3, 3, 9]), 4, 5, 3)
    assert np.abs(d - dref).max() <= 1e-13 * sigma.max() * level.max()
    assert not d[:, 0].any()
    assert np.array_equal(d[:, 1], 0.5 * d[:, 2])  # common random numbers: equal streams, the level scales exactly (powers of two)
    assert not np.array_equal(d[:, 3], 2.0 * d[:, 2])  # another stream id, other noise


def _moments(z):
    m, s = z.mean(0), z.std(0)
    return m, s, (((z - m) / s) ** 4).mean(0)


def test_moments():
    """(3) 10^6 draws per variate index (seed 2024, streams 0..999, vehicle 0, steps 0..999): |mean| < 5e-3, |std - 1| < 5e-3, kurtosis
    3 +- 0.05, |correlation| < 5e-3 between any two indices, between consecutive steps and between neighbouring streams of one index.
    Standard errors at this n: 1e-3 (mean, std, correlation), 4.9e-3 (kurtosis)."""
    ns, nt = 1000, 1000
    stream = np.repeat(np.arange(ns, dtype=np.uint32), nt)
    step = np.tile(np.arange(nt, dtype=np.uint32), ns)
    _, z = db.emu_normals(np.full(ns * nt, 2024, np.uint64), stream, 0, step)
    m, s, k = _moments(z)
    print("mean", np.round(m, 4), "\nstd ", np.round(s, 4), "\nkurt", np.round(k, 4))
    assert np.abs(m).max() < 5e-3 and np.abs(s - 1).max() < 5e-3 and np.abs(k - 3).max() < 0.05
    c = np.corrcoef(z.T)
    off = np.abs(c - np.eye(12)).max()
    zz = z.reshape(ns, nt, 12)
    c_step = max(abs(np.corrcoef(zz[:, :-1, i].ravel(), zz[:, 1:, i].ravel())[0, 1]) for i in range(12))
    c_stream = max(abs(np.corrcoef(zz[:-1, :, i].ravel(), zz[1:, :, i].ravel())[0, 1]) for i in range(12))
    print(f"largest |correlation|: between indices {off:.2e}, consecutive steps {c_step:.2e}, neighbouring streams {c_stream:.2e}")
    assert off < 5e-3 and c_step < 5e-3 and c_stream < 5e-3


def test_u1_is_never_zero():
    """(4) The all-zero words give u1 = 2^-53, the all-one words u1 = 1: both z finite, in the CPU build and in the numpy statement."""
    for w in (np.zeros(4, np.uint32), np.full(4, 0xFFFFFFFF, np.uint32)):
        z = db.emu_box_muller(w)
        assert np.isfinite(z).all(), (w, z)
        assert np.abs(z - db.box_muller(w)).max() <= 1e-13
    z0 = db.emu_box_muller(np.zeros(4, np.uint32))
    assert abs(z0[0] - np.sqrt(2 * 53 * np.log(2))) < 1e-13 and z0[1] == 0.0  # u1 = 2^-53, u2 = 0
    assert np.abs(db.emu_box_muller(np.full(4, 0xFFFFFFFF, np.uint32))).max() == 0.0  # u1 = 1: r = 0


def test_addition_is_not_contracted():
    """The disturbance enters by one rounded addition of a rounded product: (x + d) of the CPU build is numpy's x + d."""
    rng = np.random.default_rng(1)
    for x, d in rng.normal(size=(100, 2)):
        assert db.lib().cfz_emu_disturb_add(x, d * 1e-3) == x + d * 1e-3
