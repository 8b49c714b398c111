"""The device functions that compute every Newton step of the interior-point solvers -- the MPC step's backward sweep on the matrix cores
(cfz_solver.inl riccati_backward_mfma), its forward and costate scans over the lanes (forward_scan, costate_scan) and the `state_ws` sweep
(cfz_plan.inl riccati_backward_mfma, from LDS and from global memory) -- run ALONE on an MI355X by tests/hip/sweep_blocks.hip, a stand-alone
program over the product's own sources, on the systems of oracle/sweeps.py, against the textbook recursion in longdouble and the dense KKT
system solved by LAPACK and refined.

These functions exist in the device pass only (the CPU build runs plain loops), and the end-to-end tests forgive a slightly wrong Newton
step: the interior-point iteration still converges.  Here a wrong operand entry, a prefetch one stage off or a scan step that combines the
wrong partner moves an output by 1e-3 and more, against bounds of 1e-14 .. 1e-10.

The bound of an output group on a system: 32 x max(error of the CPU build of the product source, error of the numpy float64 recursion,
2^-52) on THAT system (oracle/sweeps.py `yardstick`); no bound may exceed 1e-9 and no yardstick 3e-11 (tests/test_sweeps_host.py).

Measured on an MI355X (error = max |x - ref| / max |ref| over an output group; ratio = error / max(CPU build, numpy, 2^-52); over every
horizon, layout, mode and seed; in brackets the group with the largest ratio):
  MPC step, benign:        largest kernel error 1.87e-15, largest ratio 1.44  (dpi, N 31: kernel 9.28e-16, CPU build 6.42e-16, numpy 4.62e-16, bound 2.06e-14)
  MPC step, barrier:       largest kernel error 1.42e-12, largest ratio 2.00  (dpi, N 7: kernel 4.45e-16, CPU build 1.59e-16, numpy 9.74e-17, bound 7.11e-15)
  MPC step, flat:          largest kernel error 1.94e-13, largest ratio 1.53  (dpi0, N 4: kernel 3.66e-16, CPU build 1.64e-16, numpy 2.39e-16, bound 7.65e-15)
  state_ws LDS, benign:    largest kernel error 1.16e-15, largest ratio 1.46  (fb: kernel 3.39e-16, CPU build 1.27e-16, numpy 2.33e-16, bound 7.46e-15)
  state_ws LDS, barrier:   largest kernel error 2.82e-12, largest ratio 1.86  (vf: kernel 1.85e-14, CPU build 7.77e-15, numpy 9.96e-15, bound 3.19e-13)
  state_ws LDS, flat:      largest kernel error 2.15e-15, largest ratio 2.52  (fb: kernel 5.61e-16, CPU build 2.01e-16, numpy 2.01e-16, bound 7.11e-15)
  state_ws LDS, long:      largest kernel error 6.51e-16, largest ratio 1.35  (fb: kernel 5.83e-16, CPU build 4.32e-16, numpy 3.65e-16, bound 1.38e-14)
  state_ws global:         benign 9.55e-16 / 1.46, barrier 1.76e-12 / 1.00, flat 1.96e-15 / 2.52, long 6.51e-16 / 1.35
  MPC sweep against the CPU build of riccati_backward_dense (hardware fma): 0 of 23,184 gain and value-function words differ (0 ulp) -- the
  statement above riccati_backward_dense holds, for the sweep as it stands today (ric_fetch, the value function in the step's slots).
NaN in every word that is no input, several systems in a launch against one, LDS against global pointers: the same bits.  The first run found
nothing wrong in the four functions.  Three wrong versions of the sources, each a change of arithmetic alone, fail this module: two terms of
forward_scan's vector half swapped (dp off by 2.5e-2 at N = 3), the `state_ws` sweep without its symmetrisation (fb off by 1.9e-3 at T = 299,
the third digit the history speaks of), the (3, 6) cross term of ric_H at (4, 6) (both builds wrong alike: the yardstick leaves its cap).  What the generator found on the CPU (oracle/sweeps.py generate_mpc): the MPC sweep, like the `state_ws`
sweep before its symmetrisation, takes its accumulator transposed and does not symmetrise it; within 32 stages that stays harmless (the value
function 1e-10 from symmetric on the untamed `flat` family, 1e-16 on `benign`), which is why the families are tamed rather than the sweep changed.
"""
import numpy as np
import pytest

import sweeps_binding as sb
import test_sweeps_host as host
from emu_build import build_hip_program, run_program
from oracle import sweeps as sw

pytestmark = pytest.mark.gpu

MPC_NS = host.MPC_NS      # 2, 3: the prefetch guards k > 0 / k > 1;  5 / 6: the value function changes its home;  32: the kernel's limit
LAYOUTS = host.LAYOUTS
SEEDS = host.SEEDS
# the longest plan cfz_state_ws keeps in LDS: (kSt + kFb) (T + 1) doubles beside state_ws_kernel<true>'s 128 static bytes in gfx950's 160 KiB
T_LDS_MAX = (160 * 1024 - 128) // (8 * (sw.KST + sw.KFB)) - 1
PLAN_TS_LDS = (1, 2, 3, 30, 299, 300, T_LDS_MAX)
PLAN_TS_GLOBAL = (3, 510)
assert T_LDS_MAX == 434 and set(PLAN_TS_LDS + PLAN_TS_GLOBAL) <= set(host.PLAN_TS)
MODE_GROUPS = {1: ("kk", "vf"), 2: ("dp", "dpi0", "dpi"), 3: ("kk", "dp", "dpi0", "dpi")}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """tests/hip/sweep_blocks.hip built once for gfx950; `run(header, *arrays)` = one invocation, its output as float64."""
    d = tmp_path_factory.mktemp("sweep_blocks")
    exe = build_hip_program("tests/hip/sweep_blocks.hip", d / "sweep_blocks")
    count = [0]

    def run(header, *arrays):
        count[0] += 1
        fin, fout = str(d / f"in{count[0]}.bin"), str(d / f"out{count[0]}.bin")
        with open(fin, "wb") as f:
            f.write(np.array(list(header) + [0] * (8 - len(header)), np.int64).tobytes())
            for a in arrays:
                f.write(np.ascontiguousarray(a).tobytes())
        run_program(exe, [fin, fout])
        return np.fromfile(fout, np.float64)

    return run


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.int64), np.ascontiguousarray(b, np.float64).view(np.int64))


def _ulps(a, b):
    """Largest distance of two finite float64 arrays in units of the last place."""
    key = lambda x: np.where(x.view(np.int64) < 0, np.int64(-2 ** 63) - x.view(np.int64), x.view(np.int64)).astype(np.float64)
    return float(np.abs(key(np.ascontiguousarray(a, np.float64)) - key(np.ascontiguousarray(b, np.float64))).max())


def _mpc_cases(N):
    return [host.mpc_case(f, N, seed) for f in sw.MPC_FAMILIES for seed in SEEDS]


_mpc_runs = {}


def _mpc(run, mode, cases, layout, fill=2):
    """One invocation on systems of one N -> list over the fills of lists over the systems of dict(kk, vf, dp, dpi0, dpi); kept per
    (mode, systems, layout, fill), so that the tests share the runs."""
    key = (mode, tuple((s.family, s.N, s.seed) for s, _ in cases), layout, fill)
    if key not in _mpc_runs:
        N = cases[0][0].N
        recs = []
        for s, y in cases:
            kk, vf = (np.asarray(y["ref"]["kk"], float), np.asarray(y["ref"]["vf"], float)) if mode == 2 else (np.zeros((N, 12)), np.zeros(30))
            recs.append(np.concatenate([s.ab.ravel(), s.d.ravel(), s.hc.ravel(), s.gk.ravel(), kk.ravel(), vf, s.x0, s.p0, s.pi0, s.pi.ravel()]))
            assert recs[-1].size == 55 * N + 45
        out = run([mode, len(cases), fill, N, *layout], np.array([cases[0][0].dt]), np.concatenate(recs))
        per = 24 * N + 35
        assert out.size == (2 if fill == 2 else 1) * len(cases) * per
        runs = []
        for o in out.reshape(-1, len(cases), per):
            at = np.cumsum([0, 12 * N, 30, 7 * N, 5, 5 * N])
            runs.append([dict(kk=r[at[0] : at[1]].reshape(N, 12), vf=r[at[1] : at[2]], dp=r[at[2] : at[3]].reshape(N, 7), dpi0=r[at[3] : at[4]],
                              dpi=r[at[4] : at[5]].reshape(N, 5)[: N - 1]) for r in o])
        _mpc_runs[key] = runs
    return _mpc_runs[key]


def _report(tag, rows):
    """rows: (family, group, kernel error, y) -> per family the figures the module docstring carries."""
    for fam in dict.fromkeys(r[0] for r in rows):
        mine = [r for r in rows if r[0] == fam]
        w = max(mine, key=lambda r: r[2] / r[3]["yard"][r[1]])
        print(f"{tag}, {fam}: largest kernel error {max(r[2] for r in mine):.2e}; largest ratio {w[2] / w[3]['yard'][w[1]]:.2f} ({w[1]}: kernel {w[2]:.2e}, "
              f"CPU build {w[3]['err_cpu'][w[1]]:.2e}, numpy {w[3]['err_model'][w[1]]:.2e}, bound {w[3]['bound'][w[1]]:.2e})")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("N", MPC_NS)
def test_mpc_sweep_scans_and_newton_step(harness, N, layout):
    """Six systems (three families, two seeds) of one horizon in one launch, per mode: the sweep alone (gains, value function), the scans alone
    from the reference's gains (dp, dpi0, dpi against the KKT solution), and the Newton step's three calls on one workspace.  Every group
    within its system's bound; with NaN in every word that is no input the outputs are finite and the same bits."""
    cases = _mpc_cases(N)
    rows = []
    for mode, groups in MODE_GROUPS.items():
        zeros, nans = _mpc(harness, mode, cases, layout)
        for (s, y), a, b in zip(cases, zeros, nans):
            assert host.caps_hold(y)
            for g in groups:
                err = sw.rel_err(a[g], y["ref"][g])
                rows.append((s.family, g, err, y))
                assert err <= y["bound"][g], (mode, s.family, s.seed, g, err, y["bound"][g])
                assert np.isfinite(b[g]).all() and _same_bits(a[g], b[g]), (mode, s.family, s.seed, g)
    _report(f"MPC N {N} layout {layout}", rows)


def test_mpc_sweep_against_the_cpu_build_bits(harness):
    """The claim above riccati_backward_dense (cfz_solver.inl): the CPU build's plain loops form every sum in the order of
    v_mfma_f64_16x16x4_f64, so that every gain and every value-function word has the matrix-core sweep's bits.  Mode 1 against the CPU build
    compiled with hardware fma (tests/emu_binding.py), all horizons, both layouts."""
    if not sb.host_has_fma():
        pytest.skip("the host has no hardware fma to build the CPU side of the comparison with")
    worst, differ, words = 0.0, 0, 0
    for N in MPC_NS:
        cases = _mpc_cases(N)
        for layout in LAYOUTS:
            for (s, y), a in zip(cases, _mpc(harness, 1, cases, layout)[0]):
                cpu = sb.cpu_mpc(s, *layout)
                for g in ("kk", "vf"):
                    words += a[g].size
                    if not _same_bits(a[g], cpu[g]):
                        differ += int((np.ascontiguousarray(a[g]).view(np.int64) != np.ascontiguousarray(cpu[g]).view(np.int64)).sum())
                        worst = max(worst, _ulps(a[g], cpu[g]))
    print(f"MPC sweep against the CPU build: {differ} of {words} words differ, by at most {worst:g} ulp")
    assert differ == 0, (differ, words, worst)


def test_mpc_systems_alone_and_together(harness):
    """A system computes the same bits alone in a launch as among five others: nothing of one workgroup reaches another."""
    for N in (6, 32):
        cases = _mpc_cases(N)
        for mode in (1, 3):
            together = _mpc(harness, mode, cases, LAYOUTS[0])[0]
            for i in (1, 4):
                alone, = _mpc(harness, mode, [cases[i]], LAYOUTS[0], fill=0)[0]
                for g in MODE_GROUPS[mode]:
                    assert _same_bits(alone[g], together[i][g]), (N, mode, i, g)


def _plan(run, systems, lds, fill=2):
    """One invocation of the `state_ws` sweep -> list over the fills of lists over the systems of dict(fb, vf, flag) (oracle/sweeps.py's rows)."""
    tot = sum(s.T + 1 for s in systems)
    out = run([4, len(systems), fill, int(lds)], np.array([systems[0].dt]), np.array([s.T for s in systems], np.int64),
              np.array([s.has_final for s in systems], np.int64), np.concatenate([s.st.ravel() for s in systems]))
    per = tot * (sw.KFB + sw.KVF) + len(systems)
    assert out.size == (2 if fill == 2 else 1) * per
    runs = []
    for o in out.reshape(-1, per):
        fb, vf, flags = o[: tot * sw.KFB].reshape(tot, sw.KFB), o[tot * sw.KFB : tot * (sw.KFB + sw.KVF)].reshape(tot, sw.KVF), o[tot * (sw.KFB + sw.KVF) :]
        at, res = 0, []
        for s, fl in zip(systems, flags):
            res.append(sb.plan_rows(fb[at : at + s.T + 1], vf[at : at + s.T + 1], fl, s.T))
            at += s.T + 1
        runs.append(res)
    return runs


def _plan_cases(family, Ts):
    return [host.plan_case(family, T, seed, hf) for T in ((sw.LONG_T,) if family == "long" else Ts) for seed in SEEDS for hf in (0, 1)]


@pytest.mark.parametrize("lds", (True, False), ids=("lds", "global"))
@pytest.mark.parametrize("family", sw.PLAN_FAMILIES)
def test_state_ws_sweep(harness, family, lds):
    """The sweep as newton_step<true> passes its data (LDS pointers; every length up to the longest plan that fits) and as newton_step<false>
    does (global pointers), both values of has_final, two seeds, one launch: flag 0, fb and vf within the system's bound, finite and the
    same bits from NaN-filled fb and vf."""
    cases = _plan_cases(family, PLAN_TS_LDS if lds else PLAN_TS_GLOBAL)
    zeros, nans = _plan(harness, [c[0] for c in cases], lds)
    rows = []
    for (s, y), a, b in zip(cases, zeros, nans):
        assert host.caps_hold(y) and a["flag"] == 0 and b["flag"] == 0
        for g in sw.PLAN_GROUPS:
            err = sw.rel_err(a[g], y["ref"][g])
            rows.append((family, g, err, y))
            assert err <= y["bound"][g], (s.T, s.seed, s.has_final, g, err, y["bound"][g])
            assert np.isfinite(b[g]).all() and _same_bits(a[g], b[g]), (s.T, s.seed, s.has_final, g)
    _report(f"state_ws {'LDS' if lds else 'global'}", rows)


@pytest.mark.parametrize("lds", (True, False), ids=("lds", "global"))
def test_state_ws_alone_together_and_a_singular_stage(harness, lds):
    """M_ee exactly singular at stage T - 1 (no input curvature there, a terminal value function without v and delta): flag 1, a status, and
    the system in the next workgroup is solved within its bound, with the bits it has alone in a launch.  The LDS and the global
    instantiation compute the same bits."""
    s, y = host.plan_case("benign", 30, 0, 1)
    (broken, beside), = _plan(harness, [sw.singular_plan(30, 0), s], lds, fill=1)
    assert broken["flag"] == 1 and beside["flag"] == 0
    (alone,), = _plan(harness, [s], lds, fill=0)
    (other,), = _plan(harness, [s], not lds, fill=0)
    for g in sw.PLAN_GROUPS:
        assert sw.rel_err(beside[g], y["ref"][g]) <= y["bound"][g]
        assert _same_bits(alone[g], beside[g]) and _same_bits(alone[g], other[g]), g
