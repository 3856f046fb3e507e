"""Host side of the range-proven functions of pvt_math.h (pvt_log_unit, pvt_acos_unit) for the tests: the header compiled
by gcc with the referee's own flags (oracle/Makefile: -O3 -ffp-contract=off -fno-fast-math) behind four vector wrappers.
The referee itself is the route to every OTHER function of the header (oracle.math); these two it does not call, so they
get a small library of their own, built once per test session in a temporary directory.  Also the argument sets both
tests/test_log_acos_unit.py and tests/test_gpu_log_acos_unit.py run."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "pvtrace_amd", "csrc", "pvt_math.h")
FN = {"log": 0, "log_unit": 1, "acos": 2, "acos_unit": 3}
DEVICE_FN = {"log_unit": 20, "acos_unit": 21}   # math_kernel's codes (pvt_selftest_math)

SHIM = r"""
#include "%s"
void unit_math(int fn, const double* x, double* y, long n) {
    for (long i = 0; i < n; i++)
        y[i] = fn == 0 ? pvt_log(x[i]) : fn == 1 ? pvt_log_unit(x[i]) : fn == 2 ? pvt_acos(x[i]) : pvt_acos_unit(x[i]);
}
"""


@functools.lru_cache(maxsize=None)
def _lib():
    tmp = tempfile.mkdtemp(prefix="pvt_math_unit_")
    src, so = os.path.join(tmp, "shim.c"), os.path.join(tmp, "libshim.so")
    with open(src, "w") as fh:
        fh.write(SHIM % HEADER)
    subprocess.check_call(["gcc", "-O3", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-shared", src, "-o", so])
    lib = C.CDLL(so)
    lib.unit_math.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_long]
    lib.unit_math.restype = None
    return lib


def host(fn, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.empty_like(x)
    _lib().unit_math(FN[fn], x.ctypes.data, y.ctypes.data, x.size)
    return y


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _around(v):
    v = float(v)
    return [np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)]


def _from_high_word(hi):
    """The first double whose high word is `hi` and the last one before it."""
    first = np.array([np.uint64(hi) << np.uint64(32)], dtype=np.uint64).view(np.float64)[0]
    return [np.nextafter(first, -np.inf), first]


def log_edges():
    """2^-53, 1 - 2^-53, 1, every power of two of [2^-53, 1] and the two doubles either side of each boundary of the
    reduction (high word 0x3fe6a09e) in every binade of [2^-53, 1].  (In the lower binades the doubles next to a boundary
    are finer than 2^-53: more than the draws can produce, and the two functions agree there all the same.)"""
    out = [2.0 ** -53, 1.0 - 2.0 ** -53, 1.0]
    out += [2.0 ** -e for e in range(0, 54)]
    for e in range(0, 53):
        out += _from_high_word(0x3FE6A09E - (e << 20))
    return np.array(out)


def acos_edges():
    """0; 2^-57, 0.5, 0.975 (the first double of high word 0x3fef3333) and their neighbours; 1 - 2^-53; 1."""
    out = [0.0, 1.0 - 2.0 ** -53, 1.0]
    out += _around(2.0 ** -57) + _around(0.5)
    low, first = _from_high_word(0x3FEF3333)
    out += [low, first, np.nextafter(first, np.inf)]
    # (2^-57 is the last argument answered by pio2_hi only up to its high word: the whole of that word, and the next)
    out += _from_high_word(0x3C600000) + _from_high_word(0x3C600001)
    return np.array(out)


def log_draws(n, seed=12345):
    """n arguments 1 - rng_uniform() from the kernel's generator (the referee's wrapper "uniform2": the second draw of the
    stream seeded with each integer)."""
    from oracle import oracle as O

    u = O.math("uniform2", np.arange(seed, seed + n, dtype=np.float64))
    return 1.0 - u
