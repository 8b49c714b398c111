"""The C-ABI library: loads without a GPU, exports every entry point the header declares, agrees with the
ctypes struct mirrors, and refuses to work without a HIP device (no CPU path)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from conflict_rez_amd import engine

    return engine.load_library()


def test_every_declared_symbol_is_exported(lib):
    from conflict_rez_amd import engine

    hdr = open(os.path.join(ROOT, "include", "confrez_hip.h")).read()
    declared = set(re.findall(r"\b(cfz_[a-z_0-9]+)\s*\(", hdr))
    assert declared, "no declarations found"
    for name in sorted(declared):
        assert hasattr(lib, name), name
    assert declared == set(engine.EXPORTS)


def test_struct_mirrors_and_defaults(lib):
    from conflict_rez_amd import engine

    s, o = engine._CSpec(), engine._COptions()
    lib.cfz_default_spec(C.byref(s)); lib.cfz_default_options(C.byref(o))
    assert (s.N, s.rk_substeps, s.dt, s.wb, s.dmin) == (30, 4, 0.1, 2.5, 0.05)
    assert list(s.g) == [3.3, 0.9, 0.6, 0.9] and list(s.weights) == [100, 100, 100, 1, 1, 1]
    assert list(s.bounds) == [2.5, 32.5, 7.5, 27.5, -2.5, 2.5, -0.85, 0.85, -1.5, 1.5, -1.0, 1.0]
    assert (o.max_iter, o.tol, o.constr_viol_tol, o.compl_inf_tol, o.mu_init) == (600, 1e-2, 1e-2, 1e-4, 1e-3)
    assert C.sizeof(engine._CSpec) == 4 * 4 + 8 * 3 + 8 * (4 + 12 + 6) + 8 * 8 * 8 + 8 * 8 * 4
    # the python-side spec of the parking lot round-trips
    from conflict_rez_amd import scenarios

    cs = scenarios.parking_lot_spec().to_c()
    assert (cs.N, cs.n_obs, cs.n_nbr) == (30, 6, 3) and list(cs.b_obs[:4]) == [-2.85, 13.75, -7.5, 14.65]


def test_no_cpu_fallback(lib):
    """Without a GPU the product path fails loudly; with one, creation succeeds (then this only checks errors)."""
    import torch

    from conflict_rez_amd import engine, scenarios

    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by the gpu tests")
    with pytest.raises(RuntimeError, match="cfz_create"):
        engine.Engine(scenarios.parking_lot_spec(), max_batch=4)
    assert b"no CPU path" in lib.cfz_last_error() or b"hipGetDeviceCount" in lib.cfz_last_error()


def test_ctypes_mirrors_have_the_headers_layout(tmp_path):
    """Every field of the four structs that cross the boundary sits at the offset the C header gives it (a C program compiled from
    include/confrez_hip.h prints sizeof and offsetof; the ctypes mirrors of conflict_rez_amd/engine.py must agree, name by name):
    the structs grew in every round, and a mirror that drifts reads options from the wrong words without any error."""
    import subprocess

    from conflict_rez_amd import engine

    pairs = {"cfz_spec": engine._CSpec, "cfz_options": engine._COptions, "cfz_plan_options": engine._CPlanOptions,
             "cfz_colloc_options": engine._CCollocOptions}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "confrez_hip.h"', "int main(void) {"]
    for cname, mirror in pairs.items():
        lines.append(f'  printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for fname, _ in mirror._fields_:
            lines.append(f'  printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    seen = 0
    for ln in out:
        if not ln:
            continue
        cname, fname, val = ln.split()
        mirror = pairs[cname]
        assert int(val) == (C.sizeof(mirror) if fname == "sizeof" else getattr(mirror, fname).offset), ln
        seen += 1
    assert seen == sum(len(m._fields_) + 1 for m in pairs.values())


# ---- the tables of prototypes against the C text --------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "confrez_hip.h")).read()


def _header_structs():
    """The struct types of the header: the four that are mirrored, the two that cross as opaque pointers only."""
    from conflict_rez_amd import engine

    return {"cfz_spec": engine._CSpec, "cfz_options": engine._COptions, "cfz_plan_options": engine._CPlanOptions,
            "cfz_colloc_options": engine._CCollocOptions, "cfz_handle": None, "cfz_plan_ws": None}


def test_prototypes_agree_with_the_header():
    """engine.PROTOTYPES row by row against include/confrez_hip.h: the same functions in the same order, every return type, every
    parameter count, every parameter's type (an argtypes list that is one entry short, or has an int where the header has a double,
    loads and runs and reads its arguments from the wrong registers).  Not seen: two parameters of one type in swapped order."""
    import c_decls
    from conflict_rez_amd import engine

    decls = c_decls.declarations(_header())
    assert len(decls) == 68  # a condition on the parser: what the header declares today
    assert decls["cfz_state_ws_default_guess"][1][2] == "const double init_pose[3]" and decls["cfz_abi_version"] == ("int", [])
    assert decls["cfz_score"][1][9] == "const double *tables" and decls["cfz_last_error"][0] == "const char *"
    bad = c_decls.mismatches(engine.PROTOTYPES, decls, _header_structs())
    assert not bad, "\n".join(bad)
    assert list(engine.PROTOTYPES) == list(decls), "the rows are not in the header's order"
    assert engine.EXPORTS == tuple(engine.PROTOTYPES)
    assert engine.ABI_VERSION == int(re.search(r"#define\s+CFZ_ABI_VERSION\s+(\d+)", _header()).group(1))


def test_the_prototype_check_can_fail():
    """The same check on four damaged copies of the table names cfz_score, and the parameter where there is one to name."""
    import c_decls
    from conflict_rez_amd import engine

    decls, structs = c_decls.declarations(_header()), _header_structs()
    restype, args = engine.PROTOTYPES["cfz_score"]
    k = args.index(C.c_double)
    damaged = {"one argument short": (restype, args[:-1]), "one argument twice more": (restype, args + [args[-1]] * 2),
               "a double as an int": (restype, args[:k] + [C.c_int] + args[k + 1:])}
    for what, row in damaged.items():
        bad = c_decls.mismatches({**engine.PROTOTYPES, "cfz_score": row}, decls, structs)
        assert len(bad) == 1 and bad[0].startswith("cfz_score:"), (what, bad)
    assert f"parameter {k} `double pos_tol`" in bad[0], bad
    bad = c_decls.mismatches({n: r for n, r in engine.PROTOTYPES.items() if n != "cfz_score"}, decls, structs)
    assert len(bad) == 1 and bad[0].startswith("cfz_score:"), bad
    # and the helper does not pass what it does not know
    with pytest.raises(ValueError, match="unknown base type"):
        c_decls.expected_ctypes("const cfz_thing *t", structs)
    with pytest.raises(ValueError, match="unknown base type"):
        c_decls.expected_ctypes("unsigned int n", structs)


def test_declared_parameter_counts_are_what_ctypes_bound(lib):
    """The parser against what ctypes knows of the loaded library: the parameter count of a declaration is the length of the bound argtypes."""
    import c_decls

    decls = c_decls.declarations(_header())
    for name in ("cfz_abi_version", "cfz_destroy", "cfz_create", "cfz_state_ws_default_guess", "cfz_loop_set_disturbance", "cfz_vsl_step",
                 "cfz_score", "cfz_plan_schedule", "cfz_last_error"):
        assert len(getattr(lib, name).argtypes) == len(decls[name][1]), name


def test_test_bindings_agree_with_their_sources():
    """The tables of the seven analysis bindings and of the wave-merge host library against the `extern "C"` definitions of their
    sources: every function has a row (the zero-argument ones too), no table has another, return type, count and types agree."""
    import audit_binding, c_decls, comm_binding, conflict_binding, delay_binding, disturbance_binding, schedule_binding, score_binding, wave_case  # noqa: E401

    tables = {"emu/cfz_audit_emu.cpp": audit_binding, "emu/cfz_score_emu.cpp": score_binding, "emu/cfz_conflict_emu.cpp": conflict_binding,
              "emu/cfz_delay_emu.cpp": delay_binding, "emu/cfz_schedule_emu.cpp": schedule_binding, "emu/cfz_disturb_emu.cpp": disturbance_binding,
              "emu/cfz_comm_emu.cpp": comm_binding, "hip/wave_merge_host.cpp": wave_case}
    structs = {"WaveCase": None, "WaveSpan": None, "WaveSum": None}  # of tests/hip/wave_merge_case.h: passed as numpy arrays
    seen = 0
    for source, module in tables.items():
        decls = c_decls.declarations(open(os.path.join(ROOT, "tests", source)).read())
        bad = c_decls.mismatches(module.PROTOTYPES, decls, structs)
        assert decls and not bad, (source, bad)
        seen += len(decls)
    assert seen == 24 + 4  # a condition on the parser: the static helpers and the functions of the namespaces are not among them


def test_a_named_library_may_lack_functions_the_packaged_one_may_not(tmp_path, monkeypatch):
    """A stub that exports the layout version and one more function: named through `path` or CFZ_LIBRARY (a diagnostic build, another
    commit's build) it loads with that function bound and the others left out; standing in the package's place it is refused, and the
    text names every missing function.  A stub of another layout version is refused either way, before anything is bound."""
    import subprocess

    from conflict_rez_amd import engine

    def stub(name, version):
        src = tmp_path / f"{name}.c"
        src.write_text(f"int cfz_abi_version(void) {{ return {version}; }}\nint cfz_max_batch(const void *h) {{ return 7; }}\n")
        subprocess.check_call(["gcc", "-shared", "-fPIC", "-o", str(tmp_path / f"{name}.so"), str(src)])
        return str(tmp_path / f"{name}.so")

    monkeypatch.setattr(engine, "_lib", None)  # (the loads below replace the cached library: put back afterwards)
    monkeypatch.delenv("CFZ_LIBRARY", raising=False)
    good, old = stub("stub6", engine.ABI_VERSION), stub("stub5", engine.ABI_VERSION - 1)
    lib = engine.load_library(good)
    assert lib.cfz_max_batch.argtypes == [C.c_void_p] and lib.cfz_max_batch(None) == 7
    monkeypatch.setenv("CFZ_LIBRARY", good)
    monkeypatch.setattr(engine, "_lib", None)
    assert engine.load_library().cfz_max_batch(None) == 7
    monkeypatch.delenv("CFZ_LIBRARY")
    monkeypatch.setattr(engine, "_lib", None)
    monkeypatch.setattr(engine, "LIB_PATH", good)
    with pytest.raises(RuntimeError, match="lacks symbols") as e:
        engine.load_library()
    assert all(n in str(e.value) for n in engine.EXPORTS if n not in ("cfz_abi_version", "cfz_max_batch")) and "'cfz_max_batch'" not in str(e.value)
    for kw in (dict(path=old), dict()):
        monkeypatch.setattr(engine, "LIB_PATH", old)
        with pytest.raises(RuntimeError, match=f"struct layout version {engine.ABI_VERSION - 1}, this binding is written against {engine.ABI_VERSION}"):
            engine.load_library(**kw)
