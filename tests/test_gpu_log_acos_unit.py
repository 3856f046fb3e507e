"""pvt_log_unit and pvt_acos_unit on the device (math_kernel's codes 20 and 21: the short division and square-root
sequences) against the host (gcc, plain IEEE division and square root; tests/math_unit_host.py): the same bits on
4 x 10^5 arguments each, the edges of their domains included.  The host side equals pvt_log / pvt_acos there
(tests/test_log_acos_unit.py), so the lean kernels draw what the generic ones draw."""
import numpy as np
import pytest

from pvtrace_amd.engine import native
from tests import math_unit_host as M

N = 400_000


@pytest.mark.gpu
def test_log_unit_on_the_device_is_the_hosts_bit_for_bit():
    rng = np.random.default_rng(7)
    k = np.concatenate([rng.integers(1, 2 ** 53, N // 2, endpoint=True), rng.integers(1, 2 ** 20, N // 4),     # the whole domain, its low end,
                        2 ** 53 - rng.integers(0, 2 ** 20, N // 4)]).astype(np.float64)                          # and the arguments next to 1
    x = np.concatenate([M.log_draws(N // 4), k * 2.0 ** -53, M.log_edges()])
    assert x.min() >= 2.0 ** -53 and x.max() <= 1.0
    dev = native.selftest_math(M.DEVICE_FN["log_unit"], x)
    host = M.host("log_unit", x)
    assert np.array_equal(M.bits(dev), M.bits(host)), x[M.bits(dev) != M.bits(host)][:5]
    assert np.array_equal(M.bits(host), M.bits(M.host("log", x)))


@pytest.mark.gpu
def test_acos_unit_on_the_device_is_the_hosts_bit_for_bit():
    rng = np.random.default_rng(8)
    x = np.concatenate([rng.random(N // 2), 1.0 - rng.random(N // 4) ** 4, rng.random(N // 8) ** 8,
                        0.5 + (rng.random(N // 16) - 0.5) * 1e-6, 0.975 + (rng.random(N // 16) - 0.5) * 1e-6,
                        1.0 - rng.integers(1, 2 ** 12, N // 16) * 2.0 ** -53,                                    # the doubles next to 1
                        M.acos_edges()])
    assert x.min() >= 0.0 and x.max() <= 1.0
    dev = native.selftest_math(M.DEVICE_FN["acos_unit"], x)
    host = M.host("acos_unit", x)
    assert np.array_equal(M.bits(dev), M.bits(host)), x[M.bits(dev) != M.bits(host)][:5]
    assert np.array_equal(M.bits(host), M.bits(M.host("acos", x)))
