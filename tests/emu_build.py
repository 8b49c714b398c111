"""The one build rule of the test-only CPU builds of the kernel sources (tests/emu/*.cpp): the binding modules call it.  Not a test module."""
import os
import subprocess


def build_shared(lib, sources, flags, force=False):
    """g++ `flags` on sources[0] into the shared library `lib`, when it is missing or older than any of `sources` (or `force`).  Built
    aside and renamed: parallel test workers never see a half-written library.  -> lib"""
    if force or not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(s) for s in sources):
        os.makedirs(os.path.dirname(lib), exist_ok=True)
        tmp = lib + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", *flags, "-fPIC", "-shared", "-o", tmp, sources[0]])
        os.replace(tmp, lib)
    return lib
