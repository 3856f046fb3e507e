"""pvt_log_unit and pvt_acos_unit (pvt_math.h) are pvt_log and pvt_acos with the special cases their call sites cannot
reach left out: on their domains -- k 2^-53 with 1 <= k <= 2^53, and [0, 1] -- they must return the SAME BITS, or a
photon's history in the lean kernels would leave the generic kernels' and the referee's.  Host side, no GPU; the device
side is tests/test_gpu_log_acos_unit.py."""
import numpy as np

from oracle import oracle as O
from tests import math_unit_host as M

N = 1_000_000


def same_bits(a, b):
    return np.array_equal(M.bits(a), M.bits(b))


def test_the_shim_is_the_referees_header():
    """pvt_log / pvt_acos through the shim are what the referee computes (same header, same flags)."""
    x = 1.0 - np.random.default_rng(1).random(10_000)
    assert same_bits(M.host("log", x), O.math("log", x, O.MATH_PORTABLE))
    assert same_bits(M.host("acos", x), O.math("acos", x, O.MATH_PORTABLE))


def test_log_unit_on_the_edges_of_its_domain():
    x = M.log_edges()
    assert x.min() == 2.0 ** -53 and x.max() == 1.0 and len(x) > 150
    got, want = M.host("log_unit", x), M.host("log", x)
    assert same_bits(got, want), x[M.bits(got) != M.bits(want)]
    assert M.bits(M.host("log_unit", [1.0]))[0] == 0            # +0.0, not -0.0
    assert M.host("log_unit", [2.0 ** -53])[0] == np.log(2.0 ** -53)


def test_log_unit_on_a_million_draws_of_the_kernels_generator():
    x = M.log_draws(N)
    assert x.min() > 0.0 and x.max() <= 1.0 and np.array_equal(x * 2.0 ** 53, np.floor(x * 2.0 ** 53))
    assert len(np.unique(x)) > 0.99 * N
    got, want = M.host("log_unit", x), M.host("log", x)
    assert same_bits(got, want), x[M.bits(got) != M.bits(want)][:5]


def test_acos_unit_on_the_edges_of_its_domain():
    x = M.acos_edges()
    assert x.min() == 0.0 and x.max() == 1.0
    got, want = M.host("acos_unit", x), M.host("acos", x)
    assert same_bits(got, want), x[M.bits(got) != M.bits(want)]
    pio2_hi = 1.57079632679489655800e+00
    assert M.bits(M.host("acos_unit", [1.0]))[0] == 0           # exactly +0.0
    assert M.host("acos_unit", [0.0, 2.0 ** -57, -0.0]).tolist() == [pio2_hi] * 3


def test_acos_unit_on_a_million_uniform_values():
    rng = np.random.default_rng(20261020)
    # uniform on [0, 1), and the same number again crowded towards 1 (grazing exits), towards 0 and around 0.5
    x = np.concatenate([rng.random(N), 1.0 - rng.random(N // 4) ** 4, rng.random(N // 4) ** 8,
                        0.5 + (rng.random(N // 4) - 0.5) * 1e-6, 0.975 + (rng.random(N // 4) - 0.5) * 1e-6])
    got, want = M.host("acos_unit", x), M.host("acos", x)
    assert same_bits(got, want), x[M.bits(got) != M.bits(want)][:5]
