"""What the test-only native code is built and reached with: the one build rule of the CPU builds of the kernel sources (tests/emu/*.cpp,
tests/hip/wave_merge_host.cpp), their loading and binding from a table of prototypes, and the driver of the stand-alone GPU programs
(tests/hip/*.hip).  The binding modules and the GPU test modules call it.  Not a test module."""
import ctypes as C
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ("-O2", "-ffp-contract=off")
_loaded = {}


def build_shared(lib, sources, flags, force=False):
    """g++ `flags` on sources[0] into the shared library `lib`, when it is missing or older than any of `sources` (or `force`).  Built
    aside and renamed: parallel test workers never see a half-written library.  -> lib"""
    if force or not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(s) for s in sources):
        os.makedirs(os.path.dirname(lib), exist_ok=True)
        tmp = lib + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", *flags, "-fPIC", "-shared", "-o", tmp, sources[0]])
        os.replace(tmp, lib)
    return lib


def load(stem, sources, prototypes, flags=FLAGS):
    """tests/_build/lib<stem>.so: built by `build_shared` from `sources` (paths from the repository's root, the translation unit first)
    when stale, loaded, and every row of `prototypes`, name -> (restype, argtypes), bound; once per process and library."""
    path = os.path.join(ROOT, "tests", "_build", f"lib{stem}.so")
    if path not in _loaded:
        lib = C.CDLL(build_shared(path, [os.path.join(ROOT, s) for s in sources], list(flags)))
        for name, (restype, argtypes) in prototypes.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
        _loaded[path] = lib
    return _loaded[path]


def ptr(a):
    """A numpy array as the void pointer of an argument; None stays None (NULL)."""
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def build_hip_program(source, exe):
    """hipcc --offload-arch=gfx950 -O3 on `source` (a path from the repository's root) into the program `exe`; raises with the
    compiler's stderr."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-o", str(exe), os.path.join(ROOT, source)], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed on {source} (status {r.returncode}):\n{r.stderr}")
    return str(exe)


def run_program(exe, args, timeout=120):
    """One run of a built program -> its stdout; a non-zero status raises with the status and stderr, so that a fixture which runs a GPU
    program ends there and starts nothing after it."""
    r = subprocess.run([str(exe), *(str(a) for a in args)], capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise RuntimeError(f"{exe} ended with status {r.returncode}:\n{r.stderr}")
    return r.stdout
