"""ctypes tables of the two CPU builds of the solver sources (tests/emu/cfz_emu.cpp, tests/emu/cfz_plan_emu.cpp), and the Newton step's
sweeps and scans of those builds on the systems of oracle/sweeps.py.  Not a test module."""
import ctypes as C
import functools

import numpy as np

import emu_binding
import plan_emu_binding
from emu_build import load, ptr
from oracle import sweeps as sw

_i, _d, _vp = C.c_int, C.c_double, C.c_void_p
SOURCE, PLAN_SOURCE = "tests/emu/cfz_emu.cpp", "tests/emu/cfz_plan_emu.cpp"
STRUCTS = {"cfz::KSpec": emu_binding.KSpec, "cfzp::PSpec": plan_emu_binding.PSpec}
PROTOTYPES = {  # of tests/emu/cfz_emu.cpp
    "cfz_emu_sizeof_kspec": (_i, []),
    "cfz_emu_carry_doubles": (_i, [_i, _i]),
    "cfz_emu_solve": (_i, [_vp] * 5 + [_vp] * 8 + [_i]),
    "cfz_emu_layout": (None, [_i, _i, _i, _vp]),
    "cfz_emu_riccati": (None, [_vp, _i, _i, _i, _d]),
    "cfz_emu_forward_scan": (None, [_vp, _i, _i, _i, _d]),
    "cfz_emu_costate_scan": (None, [_vp, _i, _i, _i]),
}
PLAN_PROTOTYPES = {  # of tests/emu/cfz_plan_emu.cpp
    "cfzp_emu_sizeof_spec": (_i, []),
    "cfzp_emu_n": (_i, [_vp]),
    "cfzp_emu_state_ws": (_i, [_vp] * 5),
    "cfzp_emu_riccati_dense": (_i, [_i, _d, _i, _vp, _vp, _vp]),
    "cfzp_emu_riccati": (_i, [_i, _i, _i, _d, _i, _vp, _vp, _vp, _vp]),
}
LAYOUT_WORDS = "total ab d hc gk kk rP p dp x0 pi0 dpi0 dpi pi cs".split()


def _bind(lib, table):
    for name, (restype, argtypes) in table.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


@functools.lru_cache(maxsize=None)
def lib():
    """The CPU build of cfz_solver.inl as tests/emu_binding.py builds it: hardware fma where the host has one."""
    return _bind(C.CDLL(emu_binding.build()), PROTOTYPES)


def host_has_fma():
    return " fma " in open("/proc/cpuinfo").read()


@functools.lru_cache(maxsize=None)
def plan_lib(dense_transposed):
    """The CPU build of cfz_plan.inl: the default one, or the one whose plain loops take the accumulator as the matrix-core sweep does."""
    if not dense_transposed:
        return _bind(C.CDLL(plan_emu_binding.build()), PLAN_PROTOTYPES)
    return load("cfz_plan_emu_dense", (PLAN_SOURCE, "conflict_rez_amd/csrc/cfz_plan.inl"), PLAN_PROTOTYPES,
                flags=("-O2", "-Wno-unknown-pragmas", "-DCFZP_DENSE_SWEEP", "-DCFZP_DENSE_TRANSPOSED"))


@functools.lru_cache(maxsize=None)
def layout(N, nb, n_nbr):
    out = np.zeros(len(LAYOUT_WORDS), np.int32)
    lib().cfz_emu_layout(N, nb, n_nbr, ptr(out))
    return dict(zip(LAYOUT_WORDS, (int(v) for v in out)))


def mpc_workspace(s, nb, n_nbr, fill=0.0, gains=None):
    """A workspace in the product's layout: `fill` everywhere, then the inputs of the sweep and the scans; the sensitivities and the defect of
    stage N - 1 and the word s20 of every stage are no input and keep the fill.  gains = (kk, vf): the sweep's outputs as inputs of the scans."""
    L, N = layout(s.N, nb, n_nbr), s.N
    m = np.full(L["total"], fill)
    ab = np.array(s.ab)
    ab[:, 10] = fill
    m[L["ab"] : L["ab"] + 15 * (N - 1)] = ab[: N - 1].ravel()
    m[L["d"] : L["d"] + 5 * (N - 1)] = s.d[: N - 1].ravel()
    m[L["hc"] : L["hc"] + 11 * N] = s.hc.ravel()
    m[L["gk"] : L["gk"] + 7 * N] = s.gk.ravel()
    m[L["x0"] : L["x0"] + 5], m[L["p"] : L["p"] + 5], m[L["pi0"] : L["pi0"] + 5] = s.x0, s.p0, s.pi0
    m[L["pi"] : L["pi"] + 5 * (N - 1)] = s.pi[: N - 1].ravel()
    if gains is not None:
        m[L["kk"] : L["kk"] + 12 * N], m[L["rP"] : L["rP"] + 30] = np.asarray(gains[0], float).ravel(), np.asarray(gains[1], float)
    return m


def cpu_mpc(s, nb=9, n_nbr=3, fill=0.0, gains=None):
    """The CPU build's sweep (unless `gains` are given), forward scan and costate scan on ONE workspace -> dict over oracle.sweeps.MPC_GROUPS."""
    L, N = layout(s.N, nb, n_nbr), s.N
    m = mpc_workspace(s, nb, n_nbr, fill, gains)
    out = {}
    if gains is None:
        lib().cfz_emu_riccati(ptr(m), N, nb, n_nbr, s.dt)
    out["kk"], out["vf"] = m[L["kk"] : L["kk"] + 12 * N].reshape(N, 12).copy(), m[L["rP"] : L["rP"] + 30].copy()
    lib().cfz_emu_forward_scan(ptr(m), N, nb, n_nbr, s.dt)
    lib().cfz_emu_costate_scan(ptr(m), N, nb, n_nbr)
    out["dp"], out["dpi0"] = m[L["dp"] : L["dp"] + 7 * N].reshape(N, 7).copy(), m[L["dpi0"] : L["dpi0"] + 5].copy()
    out["dpi"] = m[L["dpi"] : L["dpi"] + 5 * (N - 1)].reshape(N - 1, 5).copy()
    return out


def cpu_plan(s, one_lane=False, dense_transposed=True, fill=0.0):
    """cfzp::riccati_backward_dense of the chosen build, or the default one-lane riccati_backward with a cell end at every stage
    -> dict(fb, vf, flag); the rows no sweep writes are zero."""
    T = s.T
    st, fb, vf = np.array(s.st).ravel(), np.full((T + 1) * sw.KFB, fill), np.full((T + 1) * sw.KVF, fill)
    if one_lane:
        ce = s.ce() if T else np.zeros((1, 6))
        flag = plan_lib(False).cfzp_emu_riccati(T, 1, T, s.dt, s.has_final, ptr(st), ptr(ce), ptr(fb), ptr(vf))
    else:
        flag = plan_lib(dense_transposed).cfzp_emu_riccati_dense(T, s.dt, s.has_final, ptr(st), ptr(fb), ptr(vf))
    return plan_rows(fb, vf, flag, T)


def plan_rows(fb, vf, flag, T):
    """The rows a sweep writes (fb 1 .. T - 1, vf 1 .. T) of its raw outputs, the others zero."""
    fb, vf = np.array(fb, float).reshape(T + 1, sw.KFB), np.array(vf, float).reshape(T + 1, sw.KVF)
    fb[[0, T]] = 0.0
    vf[0] = 0.0
    return dict(fb=fb, vf=vf, flag=int(flag))
