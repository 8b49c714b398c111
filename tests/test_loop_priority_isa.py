"""The issue priority of the persistent closed-loop kernels, in the machine code of the built library (no GPU needed).

`s_setprio` is a scalar instruction: it ignores EXEC and runs once in every wavefront that reaches it.  A raise that sits under a
condition the compiler takes for lane-dependent is compiled into an EXEC-masked region and runs in every wavefront, directly followed
by the lowering of the other arm: a no-op (the library built from the revision before this test was exactly that; docs/notebook.md,
"Issue priority on the critical path").  So for each of the ten persistent kernels the gfx950 code object of libconfrez_hip.so is
disassembled with the LLVM tools of the ROCm tree, and every `s_setprio` in it must

* be reached only as the fall-through of a scalar conditional branch (`s_cbranch_scc0/1`, `s_cbranch_vccz/nz`): walking back from it,
  that branch comes before any label (another way in), any write of EXEC and any other `s_setprio`;
* not be followed by another `s_setprio` before the next label or branch (raise and lower back to back on one path);

and at least one of them raises (a non-zero operand).
"""
import os
import re
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "conflict_rez_amd", "libconfrez_hip.so")
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
KERNELS = ("loop_kernel", "loop_kernel_seq", "loop_kernel_dist", "loop_kernel_seq_dist", "loop_kernel_comm", "loop_kernel_seq_comm",
           "loop_kernel_pool", "loop_kernel_seq_pool", "loop_kernel_pool_comm", "loop_kernel_seq_pool_comm")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
UNIFORM_BRANCH = ("s_cbranch_scc0", "s_cbranch_scc1", "s_cbranch_vccz", "s_cbranch_vccnz")


def code_objects(lib, workdir):
    """The gfx950 code objects of a library: its .hip_fatbin section holds one (uncompressed) clang offload bundle per translation
    unit -- magic, entry count, then (offset, size, id length, id) per entry."""
    fat = os.path.join(workdir, "fatbin")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", lib, os.path.join(workdir, "copy")])
    blob = open(fat, "rb").read()
    out = []
    for m in re.finditer(re.escape(MAGIC), blob):
        base = m.start()
        (n,) = struct.unpack_from("<Q", blob, base + len(MAGIC))
        p = base + len(MAGIC) + 8
        for _ in range(n):
            off, size, idlen = struct.unpack_from("<QQQ", blob, p)
            ident = blob[p + 24:p + 24 + idlen].decode()
            p += 24 + idlen
            if ident.endswith("gfx950") and size:
                out.append(os.path.join(workdir, f"co{len(out)}.elf"))
                open(out[-1], "wb").write(blob[base + off:base + off + size])
    assert out, "no gfx950 code object in .hip_fatbin (a compressed bundle?)"
    return out


def kernel_listings(lib, workdir):
    """{kernel name: [("label", name) | ("inst", mnemonic, operands)]} for the ten persistent kernels."""
    found = {}
    for co in code_objects(lib, workdir):
        text = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--symbolize-operands", co], text=True)
        cur = None
        for line in text.splitlines():
            m = re.match(r"[0-9a-f]+ <(\S+)>:$", line)
            if m:
                sym = m.group(1)
                if re.fullmatch(r"L\d+", sym):
                    if cur is not None:
                        found[cur].append(("label", sym))
                    continue
                cur = next((k for k in KERNELS if f"{len(k)}{k}E" in sym or sym == k), None)
                if cur is not None:
                    found[cur] = []
                continue
            if cur is None or not line.startswith("\t"):
                continue
            body = line.split("//", 1)[0].strip()
            if body:
                mnemonic, _, operands = body.partition(" ")
                found[cur].append(("inst", mnemonic, operands.strip()))
    return found


def writes_exec(mnemonic, operands):
    if "saveexec" in mnemonic or mnemonic.startswith("v_cmpx"):
        return True
    return operands.split(",", 1)[0].strip() in ("exec", "exec_lo", "exec_hi")


def priority_faults(listing):
    """What is wrong with the `s_setprio`s of one kernel's listing (empty: nothing), and the operands met."""
    faults, levels = [], []
    for i, item in enumerate(listing):
        if item[0] != "inst" or item[1] != "s_setprio":
            continue
        levels.append(int(item[2], 0))
        where = f"s_setprio {item[2]} (instruction {i})"
        for j in range(i - 1, -1, -1):  # backwards: the scalar branch that decides it must come first
            prev = listing[j]
            if prev[0] == "label":
                faults.append(f"{where}: a label ({prev[1]}) before any scalar conditional branch")
                break
            if prev[1] in UNIFORM_BRANCH:
                break
            if prev[1] == "s_setprio":
                faults.append(f"{where}: follows s_setprio {prev[2]} on the same path")
                break
            if writes_exec(prev[1], prev[2]):
                faults.append(f"{where}: inside a region entered through `{prev[1]} {prev[2]}`")
                break
            if prev[1].startswith(("s_cbranch", "s_branch", "s_endpgm")):
                faults.append(f"{where}: decided by `{prev[1]}`, not by a scalar condition")
                break
        else:
            faults.append(f"{where}: unconditional from the kernel's entry")
        for nxt in listing[i + 1:]:  # forwards, to the end of the straight-line path
            if nxt[0] == "label" or nxt[1].startswith(("s_cbranch", "s_branch", "s_endpgm")):
                break
            if nxt[1] == "s_setprio":
                faults.append(f"{where}: s_setprio {nxt[2]} follows on the same path")
                break
    return faults, levels


@pytest.fixture(scope="module")
def listings(tmp_path_factory):
    assert os.path.exists(LIB), f"{LIB} is not built"
    return kernel_listings(LIB, str(tmp_path_factory.mktemp("isa")))


@pytest.mark.parametrize("kernel", KERNELS)
def test_priority_is_decided_by_a_scalar_branch(listings, kernel):
    assert kernel in listings, f"{kernel} not found in the library's gfx950 code ({sorted(listings)})"
    faults, levels = priority_faults(listings[kernel])
    assert any(levels), f"{kernel}: no s_setprio with a non-zero priority (found {levels})"
    assert 0 in levels, f"{kernel}: the raised priority is never lowered (found {levels})"
    assert not faults, f"{kernel}: " + "; ".join(faults)


def test_the_checker_sees_the_masked_form():
    """The sequence the compiler made of a raise under a lane-dependent condition, and the scalar form, through the same checker."""
    masked = [("inst", "v_cmp_ge_i32_e32", "vcc, s0, v6"), ("inst", "s_and_saveexec_b64", "s[0:1], vcc"),
              ("inst", "s_xor_b64", "s[0:1], exec, s[0:1]"), ("inst", "s_setprio", "3"), ("inst", "s_andn2_saveexec_b64", "s[0:1], s[0:1]"),
              ("inst", "s_setprio", "0"), ("inst", "s_or_b64", "exec, exec, s[0:1]")]
    faults, levels = priority_faults(masked)
    assert levels == [3, 0] and len(faults) >= 2 and any("saveexec" in f for f in faults), faults
    scalar = [("inst", "s_cmp_gt_i32", "s4, s5"), ("inst", "s_cbranch_scc1", "L7"), ("inst", "s_setprio", "3"), ("label", "L7"),
              ("inst", "v_add_f64", "v[0:1], v[0:1], v[2:3]"), ("inst", "s_cbranch_vccnz", "L9"), ("inst", "s_setprio", "0"), ("label", "L9")]
    assert priority_faults(scalar) == ([], [3, 0])
