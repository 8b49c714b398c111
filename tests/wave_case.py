"""What tests/test_wave_merge_gpu.py and tests/test_block_merge_gpu.py share: the padded test struct of tests/hip/wave_merge_case.h as a
numpy dtype, its sort key, the comparison of struct arrays by their fields, and the g++ build of the header's host forms
(tests/hip/wave_merge_host.cpp)."""
import ctypes as C

import numpy as np

from emu_build import load

_i, _vp = C.c_int, C.c_void_p
PROTOTYPES = {  # of tests/hip/wave_merge_host.cpp
    "wave_host_min": (_i, [_vp, _i, _i]),
    "wave_host_concat": (_i, [_vp, _i, _i]),
    "block_host_min": (_i, [_vp, _i, _i, _vp]),
    "block_host_sum": (_i, [_vp, _i, _i, _vp]),
}


def host_lib():
    return load("wave_merge_host", ("tests/hip/wave_merge_host.cpp", "tests/hip/wave_merge_case.h", "conflict_rez_amd/csrc/cfz_wave.inl"), PROTOTYPES)


CASE = np.dtype([("a", "<i4"), ("x", "<f8"), ("b", "<i4", (3,))], align=True)
assert CASE.itemsize == 32  # as the static_assert of wave_merge_case.h


def same(a, b):
    """Every field equal, doubles by their bits; padding is never compared."""
    return all(np.array_equal(np.ascontiguousarray(a[n]).view(np.int64 if a.dtype[n] == np.float64 else np.int32),
                              np.ascontiguousarray(b[n]).view(np.int64 if a.dtype[n] == np.float64 else np.int32)) for n in a.dtype.names)


def key(c):
    """The order of case_min: (x, a, b[0], b[1], b[2])."""
    return (float(c["x"]), int(c["a"]), *(int(v) for v in c["b"]))
