"""What tests/test_wave_merge_gpu.py and tests/test_block_merge_gpu.py share: the padded test struct of tests/hip/wave_merge_case.h as a
numpy dtype, its sort key, and the comparison of struct arrays by their fields."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = np.dtype([("a", "<i4"), ("x", "<f8"), ("b", "<i4", (3,))], align=True)
assert CASE.itemsize == 32  # as the static_assert of wave_merge_case.h


def same(a, b):
    """Every field equal, doubles by their bits; padding is never compared."""
    return all(np.array_equal(np.ascontiguousarray(a[n]).view(np.int64 if a.dtype[n] == np.float64 else np.int32),
                              np.ascontiguousarray(b[n]).view(np.int64 if a.dtype[n] == np.float64 else np.int32)) for n in a.dtype.names)


def key(c):
    """The order of case_min: (x, a, b[0], b[1], b[2])."""
    return (float(c["x"]), int(c["a"]), *(int(v) for v in c["b"]))
