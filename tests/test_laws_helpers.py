"""Calibration of tests/laws.py: for every law, numpy samples drawn from the exact law pass its check and samples from
a stated small perturbation fail it; the closed forms agree with independent statements of the same physics.  CPU
only, fixed seeds, a few seconds."""
import math

import numpy as np
import pytest

from tests import laws as L

N = 200_000


def fails(check, *args):
    with pytest.raises(AssertionError):
        check(*args)


# -- closed forms ------------------------------------------------------------------------------------------------------
def test_fresnel_hecht_against_the_amplitude_form():
    """Hecht's sin / tan form equals the amplitude-coefficient form r_s = (n1 c_i - n2 c_t) / (n1 c_i + n2 c_t),
    r_p = (n2 c_i - n1 c_t) / (n2 c_i + n1 c_t); 4 % at normal incidence into glass; 0 for p at Brewster; 1 beyond the
    critical angle and at grazing incidence."""
    for n1, n2 in ((1.0, 1.5), (1.5, 1.0), (1.33, 1.7)):
        for deg in np.linspace(0.5, 89.5, 37):
            t = math.radians(deg)
            s = n1 / n2 * math.sin(t)
            if s >= 1.0:
                assert L.fresnel_r(t, n1, n2) == 1.0
                continue
            ci, ct = math.cos(t), math.sqrt(1 - s * s)
            rs = ((n1 * ci - n2 * ct) / (n1 * ci + n2 * ct)) ** 2
            rp = ((n2 * ci - n1 * ct) / (n2 * ci + n1 * ct)) ** 2
            assert abs(L.fresnel_r(t, n1, n2) - 0.5 * (rs + rp)) < 1e-12, (n1, n2, deg)
    assert abs(L.fresnel_r(0.0, 1.0, 1.5) - 0.04) < 1e-15
    tb = L.brewster(1.0, 1.5)
    tt = math.asin(math.sin(tb) / 1.5)
    assert abs(L.fresnel_r(tb, 1.0, 1.5) - 0.5 * (math.sin(tb - tt) / math.sin(tb + tt)) ** 2) < 1e-15
    assert abs(L.fresnel_r(math.radians(89.9999), 1.0, 1.5) - 1.0) < 1e-4
    assert L.fresnel_r(L.critical_angle(1.5, 1.0) + 1e-12, 1.5, 1.0) == 1.0
    assert L.fresnel_r(0.3, 1.5, 1.5) == 0.0


def test_exact_table_lookups():
    xs, ys = [400.0, 500.0, 600.0], [1.0, 3.0, 2.0]
    assert L.lerp_exact(450.0, xs, ys) == 2.0 and L.lerp_exact(300.0, xs, ys) == 1.0 and L.lerp_exact(700.0, xs, ys) == 2.0
    assert L.lerp_exact(500.0, xs, ys) == 3.0 and L.lerp_exact(575.0, xs, ys) == 2.25
    # the step rule: a value holds from just above the node before it up to its own node
    assert [L.step_exact(x, xs, ys) for x in (350.0, 400.0, 400.5, 500.0, 550.0, 600.0, 650.0)] == [1, 1, 3, 3, 2, 2, 2]
    v = [[0.0, 1.0], [1.0, 0.5]]
    assert L.bilinear_exact(500.0, 45.0, [400.0, 600.0], [0.0, 90.0], v) == 0.625
    assert L.bilinear_exact(900.0, 100.0, [400.0, 600.0], [0.0, 90.0], v) == 0.5


def test_beer_lambert_forms():
    p = L.absorption_outcomes([0.3, 0.9], 2.0)
    assert abs(sum(p) - 1.0) < 1e-15 and abs(p[0] - math.exp(-2.4)) < 1e-15 and abs(p[2] / p[1] - 3.0) < 1e-12
    assert L.absorption_outcomes([0.5e-8, 0.3e-8], 1e8)[0] == 1.0
    F = L.truncated_exponential_cdf(1.5, 2.0)
    assert F(0.0) == 0.0 and abs(F(2.0) - 1.0) < 1e-15 and abs(F(5.0) - 1.0) < 1e-15


def test_kt_start():
    assert abs(L.kt_start(560.0) - 1240.0 / (1240.0 / 560.0 + 1.5 * 8.617333262e-5 * 300.0)) < 1e-6
    assert 550.0 < L.kt_start(560.0) < 550.5


def test_hg_cdf_is_the_normalised_hg_density():
    """The HG mu-CDF integrates the HG density (1 - g^2) / (2 (1 + g^2 - 2 g mu)^1.5); mean g."""
    for g in (0.9, 0.3, -0.6):
        mu = np.linspace(-1.0, 1.0, 200_001)
        pdf = (1 - g * g) / (2 * (1 + g * g - 2 * g * mu) ** 1.5)
        cdf = np.concatenate(([0.0], np.cumsum((pdf[1:] + pdf[:-1]) / 2 * np.diff(mu))))
        assert np.max(np.abs(cdf - L.hg_mu_cdf(g)(mu))) < 1e-5, g
        mean = np.sum((mu * pdf)[1:] + (mu * pdf)[:-1]) / 2 * (mu[1] - mu[0])
        assert abs(mean - g) < 1e-5, g


def test_hist_emission_probabilities():
    x, cdf = np.array([500.0, 520.0, 540.0]), np.array([0.2, 0.7, 1.0])
    assert np.allclose(L.hist_emission_probabilities(x, cdf), [0.2, 0.5, 0.3])
    # from 510 nm: p1 = cdf[#{x < 510}] = 0.7, so only the last node remains
    assert np.allclose(L.hist_emission_probabilities(x, cdf, 510.0), [0.0, 0.0, 1.0])
    # from 500 nm: p1 = cdf[0] = 0.2
    assert np.allclose(L.hist_emission_probabilities(x, cdf, 500.0), [0.0, 0.5 / 0.8, 0.3 / 0.8])


def test_chi2_quantile_matches_known_values():
    """Wilson-Hilferty against the 1 - 1e-6 quantiles of chi-square (dof 10: 46.863, dof 100: 182.127): slightly
    conservative at few degrees of freedom, within 0.2 % at many."""
    assert 46.863 < L.chi2_quantile(10) < 46.863 * 1.03
    assert abs(L.chi2_quantile(100) - 182.127) / 182.127 < 0.002


# -- statistics: exact samples pass, perturbed samples fail ------------------------------------------------------------
def test_binomial_bound():
    rng = np.random.default_rng(1)
    L.assert_binomial(rng.binomial(N, 0.3), N, 0.3)
    fails(L.assert_binomial, rng.binomial(N, 0.3 * 1.03), N, 0.3)        # p off by 3 %
    L.assert_binomial(0, N, 0.0)
    fails(L.assert_binomial, 1, N, 0.0)
    L.assert_binomial(N, N, 1.0)
    fails(L.assert_binomial, N - 1, N, 1.0)
    L.assert_binomial(rng.binomial(N, 2e-5), N, 2e-5)                    # Poisson regime
    fails(L.assert_binomial, rng.binomial(N, 2e-4), N, 2e-5)
    L.assert_binomial(N, N, 1.0 - 1e-12)


def test_multinomial_bound():
    rng = np.random.default_rng(2)
    p = [0.3, 0.5, 0.2]
    L.assert_multinomial(rng.multinomial(N, p), p)
    fails(L.assert_multinomial, rng.multinomial(N, [0.31, 0.49, 0.2]), p)
    fails(L.assert_multinomial, [10, 0, N - 10], [0.0, 0.5, 0.5])


def test_chi2_bound():
    rng = np.random.default_rng(3)
    x = rng.normal(size=N)
    edges = np.linspace(-4.0, 4.0, 81)
    cdf = lambda v: 0.5 * (1 + np.vectorize(math.erf)(np.asarray(v) / math.sqrt(2)))
    probs = L.bin_probabilities(cdf, edges)
    counts = lambda s: np.bincount(np.searchsorted(edges, s, side="right"), minlength=edges.size + 1)
    L.assert_chi2(counts(x), probs)
    fails(L.assert_chi2, counts(x * 1.02), probs)                         # width off by 2 %
    fails(L.assert_chi2, counts(x + 0.03), probs)                         # shifted by 0.03 sigma


def test_ks_bounds():
    rng = np.random.default_rng(4)
    u = rng.random(N)
    L.assert_ks(u, L.uniform_cdf(0.0, 1.0))
    fails(L.assert_ks, u ** 1.02, L.uniform_cdf(0.0, 1.0))
    L.assert_ks2(u[: N // 2], rng.random(N))
    fails(L.assert_ks2, u[: N // 2] ** 1.03, rng.random(N))


def test_mean_bound():
    rng = np.random.default_rng(5)
    L.assert_mean(rng.exponential(2.0, N), 2.0)
    fails(L.assert_mean, rng.exponential(2.0 * 1.02, N), 2.0)


# -- the laws themselves, on numpy samples of the exact rule and of a stated perturbation ------------------------------
def _hg(g, u):
    s = 2 * u - 1
    return (1 + g * g - ((1 - g * g) / (1 + g * s)) ** 2) / (2 * g)


@pytest.mark.parametrize("g", [0.9, 0.3, -0.6])
def test_hg_law(g):
    """Exact HG samples pass; g scaled by 0.98 fails (KS or mean) at 1e6 samples, the GPU's n."""
    rng = np.random.default_rng(6)
    n = 1_000_000
    L.assert_ks(_hg(g, rng.random(n)), L.hg_mu_cdf(g))
    L.assert_mean(_hg(g, rng.random(n)), g)
    with pytest.raises(AssertionError):
        bad = _hg(0.98 * g, rng.random(n))
        L.assert_ks(bad, L.hg_mu_cdf(g))
        L.assert_mean(bad, g)


def test_isotropic_cone_lambertian_laws():
    rng = np.random.default_rng(7)
    L.assert_ks(2 * rng.random(N) - 1, L.isotropic_mu_cdf())
    fails(L.assert_ks, 2 * rng.random(N) ** 1.02 - 1, L.isotropic_mu_cdf())
    tm = 0.6
    L.assert_ks(np.sqrt(rng.random(N)) * math.sin(tm), L.cone_sin_cdf(tm))
    fails(L.assert_ks, np.sqrt(rng.random(N)) * math.sin(0.98 * tm), L.cone_sin_cdf(tm))
    mu = np.sqrt(1 - rng.random(N))                    # sin^2 theta uniform
    L.assert_ks(1 - mu * mu, L.lambertian_sin2_cdf())
    fails(L.assert_ks, 1 - rng.random(N) ** 2, L.lambertian_sin2_cdf())     # cos theta uniform instead
    L.assert_ks(np.arctan2(*rng.normal(size=(2, N))), L.uniform_cdf(-math.pi, math.pi))
    fails(L.assert_ks, np.arctan2(*rng.normal(size=(2, N)) * [[1.0], [1.1]]), L.uniform_cdf(-math.pi, math.pi))


def test_beer_lambert_depth_and_lifetime_laws():
    rng = np.random.default_rng(8)
    a, length = 1.2, 1.0
    d = rng.exponential(1 / a, 3 * N)
    d = d[d < length]
    L.assert_ks(d, L.truncated_exponential_cdf(a, length))
    fails(L.assert_ks, d[d < 0.97 * length] / 0.97, L.truncated_exponential_cdf(a, length))
    L.assert_ks(rng.exponential(4e-9, N), L.exponential_cdf(4e-9))
    fails(L.assert_ks, rng.exponential(4.1e-9, N), L.exponential_cdf(4e-9))


def test_emission_cdf_law():
    """Inverse-CDF samples of a piecewise-linear CDF pass, conditioned on lambda >= start too; a start off by 1 nm
    fails."""
    rng = np.random.default_rng(9)
    x = np.arange(400.0, 801.0, 5.0)
    y = np.exp(-0.5 * ((x - 600.0) / 40.0) ** 2)
    cdf = np.concatenate(([0.0], np.cumsum((y[1:] + y[:-1]) / 2)))
    cdf /= cdf[-1]
    edges = np.arange(402.5, 800.0, 5.0)
    counts = lambda s: np.bincount(np.searchsorted(edges, s, side="right"), minlength=edges.size + 1)
    for start in (None, 560.0, 550.2):
        p1 = 0.0 if start is None else np.interp(start, x, cdf)
        probs = L.bin_probabilities(L.emission_cdf(x, cdf, start), edges)
        L.assert_chi2(counts(np.interp(p1 + (1 - p1) * rng.random(N), cdf, x)), probs)
        if start is not None:
            q1 = np.interp(start - 1.0, x, cdf)
            fails(L.assert_chi2, counts(np.interp(q1 + (1 - q1) * rng.random(N), cdf, x)), probs)


def test_masks_and_pose():
    """Disc samples (r^2 uniform) posed by a rotation and a translation pass after `to_local`; r = R U fails; the
    pose undone without its rotation leaves the samples out of the light's plane."""
    rng = np.random.default_rng(10)
    R, t = L.rotation(2.1, (0.2, -1.0, 0.5)), np.array([-2.0, 0.5, 1.0])
    ang, rad = 2 * np.pi * rng.random(N), 2.0 * np.sqrt(rng.random(N))
    local = np.column_stack((rad * np.cos(ang), rad * np.sin(ang), np.zeros(N)))
    world = local @ R.T + t
    back = L.to_local(world, R, t)
    assert np.max(np.abs(back[:, 2])) < 1e-12
    L.assert_ks((back[:, 0] ** 2 + back[:, 1] ** 2) / 4.0, L.uniform_cdf(0.0, 1.0))
    fails(L.assert_ks, (2.0 * rng.random(N)) ** 2 / 4.0, L.uniform_cdf(0.0, 1.0))
    assert np.max(np.abs((local + t - t)[:, 2] - L.to_local(local + t, R, t)[:, 2])) > 0.1
    assert np.allclose(L.rotation(0.7, (1.0, 1.0, 0.0)) @ L.rotation(0.7, (1.0, 1.0, 0.0)).T, np.eye(3))
    assert np.allclose(L.rotation(math.pi / 2, (0, 0, 1)) @ [1.0, 0.0, 0.0], [0.0, 1.0, 0.0])
