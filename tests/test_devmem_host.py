"""Who owns device memory (conflict_rez_amd/csrc/cfz_devmem.h), without a GPU: tests/hip/devmem_host.cpp, a stand-alone program over that
header alone, puts DevBuf and Arena on a counting allocator over malloc that can be told to fail its k-th call, built with
g++ -fsanitize=address,undefined and run once per case.  Exit status 0 means every check of the case held, nothing was live at its end
and neither sanitizer spoke."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("alloc_reset", "reserve", "move", "release_by_assignment", "commit", "arena")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("devmem") / "devmem_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror",
                           "-o", out, os.path.join(ROOT, "tests", "hip", "devmem_host.cpp")])
    return out


@pytest.mark.parametrize("case", CASES)
def test_case(exe, case):
    r = subprocess.run([exe, case], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == f"{case}: ok, live blocks 0" and not r.stderr, (r.returncode, r.stdout, r.stderr)


def test_header_needs_no_hip(tmp_path):
    """With a policy supplied the header compiles with plain g++ and no ROCm header (nothing on the include path but the compiler's own)."""
    src = tmp_path / "only.cpp"
    src.write_text('#include "cfz_devmem.h"\nstruct M { static int alloc(void **, size_t) { return -1; } static void free(void *) {} };\n'
                   "int main() { DevBuf<double, M> b; Arena<M> a; void *p; return (b.alloc(3) == -1 && arena_alloc(a, &p, 8) == -1 && !b) ? 0 : 1; }\n")
    exe = str(tmp_path / "only")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "conflict_rez_amd", "csrc"), "-o", exe, str(src)])
    assert subprocess.run([exe], timeout=60).returncode == 0
