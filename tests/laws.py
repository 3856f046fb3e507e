"""Closed-form laws the engine's sampling must obey, and the statistics that hold samples to them.  numpy only.

Written from the physics and from the contract's sampling rules, NOT from the referee's code: Fresnel in Hecht's
sin / tan form (the referee uses the n1 cos - n2 k form), table lookups in exact rational arithmetic
(`fractions.Fraction`), distributions as CDFs rather than as the inverse transforms the engine runs.

Every test that uses these runs under fixed seeds, so every verdict is deterministic.  The bounds are set so that a
correct engine fails with probability ~1e-6 per check: |z| < 5 (two-sided 5.7e-7), chi-square against its 1 - 1e-6
quantile, Kolmogorov-Smirnov D sqrt(n) < 2.7 (asymptotic tail 2 exp(-2 * 2.7^2) = 9e-7).
"""
import math
from fractions import Fraction

import numpy as np

Z_BOUND = 5.0
KS_BOUND = 2.7
CHI2_MIN_EXPECTED = 25.0
CHI2_TAIL = 1e-6
Z_TAIL_1E6 = 4.753424308822899      # upper 1e-6 quantile of the standard normal

KB_EV = 1.380649e-23 / 1.60217662e-19   # Boltzmann's constant in eV / K (the contract's value)
ALPHA_ZERO = 1e-8                       # the contract's clear-medium threshold: alpha <= this draws no depth


# -- optics ------------------------------------------------------------------------------------------------------------
def critical_angle(n1, n2):
    """asin(n2 / n1) for light going from n1 into n2 < n1; None when there is no total internal reflection."""
    return math.asin(n2 / n1) if n2 < n1 else None


def fresnel_r(theta, n1, n2):
    """Unpolarised Fresnel reflectance at angle of incidence `theta` (radians) from n1 into n2, Hecht's form:
    R_s = sin^2(ti - tt) / sin^2(ti + tt), R_p = tan^2(ti - tt) / tan^2(ti + tt), R = (R_s + R_p) / 2; 1 beyond the
    critical angle; ((n1 - n2) / (n1 + n2))^2 at normal incidence."""
    s = n1 / n2 * math.sin(theta)
    if s >= 1.0:
        return 1.0
    if theta == 0.0:
        return ((n1 - n2) / (n1 + n2)) ** 2
    tt = math.asin(s)
    if tt == theta:      # index-matched
        return 0.0
    rs = (math.sin(theta - tt) / math.sin(theta + tt)) ** 2
    rp = 0.0 if abs(theta + tt - math.pi / 2) < 1e-15 else (math.tan(theta - tt) / math.tan(theta + tt)) ** 2
    return 0.5 * (rs + rp)


def brewster(n1, n2):
    return math.atan(n2 / n1)


# -- tables, exactly ---------------------------------------------------------------------------------------------------
def _F(x):
    return Fraction(float(x))


def lerp_exact(x, xs, ys):
    """Piecewise-linear interpolation of (xs, ys) at x, clamped at both ends, in rational arithmetic -> float."""
    x, xs, ys = _F(x), [_F(v) for v in xs], [_F(v) for v in ys]
    if len(xs) == 1 or x <= xs[0]:
        return float(ys[0])
    if x >= xs[-1]:
        return float(ys[-1])
    k = max(i for i in range(len(xs)) if xs[i] <= x)
    t = (x - xs[k]) / (xs[k + 1] - xs[k])
    return float(ys[k] + t * (ys[k + 1] - ys[k]))


def step_exact(x, xs, ys):
    """The `hist=True` rule: ys[#{xs_i < x}], the index clamped to the table (a value holds from just above the node
    before it up to and including its own node)."""
    k = sum(1 for v in xs if v < x)
    return float(ys[min(k, len(ys) - 1)])


def bilinear_exact(wl, angle_deg, wavelengths, angles_deg, values):
    """R(wl, angle) of a reflectivity table: linear in wavelength on each angle row, then linear in angle; both axes
    clamped; rational arithmetic.  `values` is (n_angle, n_wavelength)."""
    values = np.asarray(values, dtype=float).reshape(len(angles_deg), len(wavelengths))
    rows = [lerp_exact(wl, wavelengths, row) for row in values]
    return lerp_exact(angle_deg, angles_deg, rows)


# -- Beer-Lambert ------------------------------------------------------------------------------------------------------
def escape_probability(alpha, length):
    """exp(-alpha L); exactly 1 for alpha <= ALPHA_ZERO (the contract draws no depth in a clear medium)."""
    return 1.0 if alpha <= ALPHA_ZERO else math.exp(-alpha * length)


def absorption_outcomes(alphas, length):
    """[P(escape), P(absorbed by component i)...]: component i takes alpha_i / alpha of the absorbed photons."""
    alpha = float(sum(alphas))
    esc = escape_probability(alpha, length)
    return [esc] + [(1.0 - esc) * a / alpha if alpha > 0 else 0.0 for a in alphas]


def truncated_exponential_cdf(alpha, length):
    """CDF of the absorption depth d in [0, L] given absorption before L."""
    norm = -math.expm1(-alpha * length)
    return lambda d: -np.expm1(-alpha * np.clip(d, 0.0, length)) / norm


def exponential_cdf(tau):
    return lambda t: -np.expm1(-np.maximum(t, 0.0) / tau)


# -- spectra -----------------------------------------------------------------------------------------------------------
def kt_start(wavelength, T=300.0):
    """The wavelength from which "kT" re-emission starts: 1240 / (1240 / wl + 3/2 k_B T)."""
    return 1240.0 / (1240.0 / wavelength + 1.5 * KB_EV * T)


def piecewise_cdf(x, cdf):
    """The CDF of inverse-CDF sampling of a compiled (x, cdf) table: piecewise linear, 0 below x[0], 1 above x[-1]."""
    x, cdf = np.asarray(x, float), np.asarray(cdf, float)
    return lambda v: np.interp(v, x, cdf, left=0.0, right=1.0)


def emission_cdf(x, cdf, start=None):
    """CDF of the re-emitted wavelength of a (non-hist) spectrum, conditioned on lambda >= `start` (None: the full
    spectrum): (F(v) - F(start)) / (1 - F(start))."""
    F = piecewise_cdf(x, cdf)
    p1 = 0.0 if start is None else float(F(start))
    return lambda v: np.clip((F(v) - p1) / (1.0 - p1), 0.0, 1.0)


def bin_probabilities(cdf, edges):
    """P(edges[k] <= X < edges[k+1]) from a CDF, plus the two outer tails -> (len(edges) + 1,)."""
    c = np.asarray(cdf(np.asarray(edges, float)), float)
    return np.diff(np.concatenate(([0.0], c, [1.0])))


def hist_emission_probabilities(x, cdf, start=None):
    """P(lambda = x_k) of a hist=True spectrum: the draw gamma is uniform on [p1, 1) and picks x_k for
    cdf_{k-1} < gamma <= cdf_k; p1 = cdf[#{x_i < start}] (the step rule), 0 for the full spectrum."""
    cdf = np.asarray(cdf, float)
    p1 = 0.0 if start is None else step_exact(start, list(x), list(cdf))
    lo = np.maximum(np.concatenate(([0.0], cdf[:-1])), p1)
    hi = np.maximum(cdf, p1)
    p = (hi - lo) / (1.0 - p1)
    p[-1] += max(0.0, 1.0 - max(cdf[-1], p1)) / (1.0 - p1)      # (a CDF that stops short of 1 runs off the table)
    return p


# -- directions (the contract's sampling rules, as CDFs of the polar cosine mu about the rule's axis) --------------------
def hg_mu_cdf(g):
    """Henyey-Greenstein: P(mu <= m) = (1 - g^2) / (2 g) [1 / sqrt(1 + g^2 - 2 g m) - 1 / (1 + g)]; mean g."""
    def F(m):
        m = np.clip(m, -1.0, 1.0)
        return (1 - g * g) / (2 * g) * (1 / np.sqrt(1 + g * g - 2 * g * m) - 1 / (1 + g))
    return F


def isotropic_mu_cdf():
    return lambda m: np.clip((np.asarray(m) + 1.0) / 2.0, 0.0, 1.0)


def cone_sin_cdf(theta_max):
    """The cone rule sin(theta) = sqrt(U) sin(theta_max): P(sin theta <= s) = s^2 / sin^2 theta_max.  (Not uniform in
    solid angle: that would be uniform in cos theta.)"""
    s2 = math.sin(theta_max) ** 2
    return lambda s: np.clip(np.asarray(s) ** 2 / s2, 0.0, 1.0)


def lambertian_sin2_cdf():
    """Lambertian (cosine-weighted) hemisphere: sin^2 theta uniform on [0, 1]."""
    return lambda v: np.clip(v, 0.0, 1.0)


def uniform_cdf(lo, hi):
    return lambda v: np.clip((np.asarray(v) - lo) / (hi - lo), 0.0, 1.0)


def azimuth(d, axis=2):
    """Azimuth about `axis` of unit vectors d (n, 3), in (-pi, pi]."""
    a, b = [(1, 2), (2, 0), (0, 1)][axis]
    return np.arctan2(d[:, b], d[:, a])


def rotation(angle, axis):
    """Rodrigues: the right-handed rotation by `angle` about `axis` (3x3)."""
    k = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def to_local(points, R, location=None):
    """World rows -> the frame of a pose (R, location): R^T (p - location)."""
    p = np.asarray(points, float)
    if location is not None:
        p = p - np.asarray(location, float)
    return p @ R


# -- statistics --------------------------------------------------------------------------------------------------------
def binomial_z(k, n, p):
    """z of k successes in n trials at probability p."""
    return (k - n * p) / math.sqrt(n * p * (1 - p))


def poisson_tails(k, lam):
    """(P(X <= k), P(X >= k)) of a Poisson variable of mean lam."""
    terms, term = [], math.exp(-lam)
    for i in range(k + 1):
        terms.append(term)
        term *= lam / (i + 1)
    below = min(1.0, sum(terms))
    return below, min(1.0, 1.0 - below + terms[-1])


def assert_binomial(k, n, p, what=""):
    """k of n at probability p: exactly 0 / n where p is 0 / 1, else |z| < 5; where the rarer outcome is expected
    fewer than 25 times, its count is held to the Poisson law instead (both tails above 1e-7)."""
    k, n = int(k), int(n)
    if p <= 0.0:
        assert k == 0, (what, k, n, p)
    elif p >= 1.0:
        assert k == n, (what, k, n, p)
    elif n * min(p, 1.0 - p) < 25.0:
        rare, lam = (k, n * p) if p < 0.5 else (n - k, n * (1.0 - p))
        below, above = poisson_tails(rare, lam)
        assert below > 1e-7 and above > 1e-7, (what, f"rare outcome {rare} times, expected {lam:.3g}")
    else:
        z = binomial_z(k, n, p)
        assert abs(z) < Z_BOUND, (what, f"k={k} n={n} p={p:.6g} z={z:.2f}")


def assert_multinomial(counts, probs, what=""):
    """Every category's count against its binomial law (exact at p = 0 / 1), and the whole by chi-square."""
    counts = np.asarray(counts, dtype=np.int64)
    n = int(counts.sum())
    for i, (k, p) in enumerate(zip(counts, probs)):
        assert_binomial(k, n, p, (what, "category", i))
    if sum(1 for p in probs if 0 < p) > 1:
        assert_chi2(counts, probs, what)


def merge_bins(counts, probs, n, min_expected=CHI2_MIN_EXPECTED):
    """Merge adjacent bins, from the ends inwards and left to right, until every expected count is >= min_expected."""
    counts, expected = list(np.asarray(counts, float)), list(np.asarray(probs, float) * n)
    oc, oe, acc_c, acc_e = [], [], 0.0, 0.0
    for c, e in zip(counts, expected):
        acc_c += c
        acc_e += e
        if acc_e >= min_expected:
            oc.append(acc_c)
            oe.append(acc_e)
            acc_c = acc_e = 0.0
    if acc_e > 0 or acc_c > 0:
        if oe:
            oc[-1] += acc_c
            oe[-1] += acc_e
        else:
            oc.append(acc_c)
            oe.append(acc_e)
    return np.array(oc), np.array(oe)


def chi2_quantile(dof, tail=CHI2_TAIL):
    """Wilson-Hilferty: the upper `tail` quantile of chi-square with `dof` degrees of freedom (tail = 1e-6 only)."""
    assert tail == CHI2_TAIL
    h = 2.0 / (9.0 * dof)
    return dof * (1.0 - h + Z_TAIL_1E6 * math.sqrt(h)) ** 3


def chi2_stat(counts, probs):
    counts = np.asarray(counts, float)
    n = counts.sum()
    oc, oe = merge_bins(counts, probs, n)
    if np.any((oe == 0) & (oc > 0)):
        return math.inf, len(oc) - 1
    keep = oe > 0
    return float(np.sum((oc[keep] - oe[keep]) ** 2 / oe[keep])), int(keep.sum()) - 1


def assert_chi2(counts, probs, what=""):
    """Pearson chi-square of `counts` against `probs` (bins merged to an expected count >= 25) below its 1 - 1e-6
    quantile; a count in a bin of probability 0 fails outright."""
    probs = np.asarray(probs, float)
    assert abs(probs.sum() - 1.0) < 1e-9, (what, probs.sum())
    stat, dof = chi2_stat(counts, probs)
    assert dof >= 1, (what, "chi-square needs at least two bins", dof)
    q = chi2_quantile(dof)
    assert stat < q, (what, f"chi2={stat:.1f} > {q:.1f} (dof {dof})")


def ks_stat(x, cdf):
    """One-sample Kolmogorov-Smirnov D of samples x against a continuous CDF."""
    x = np.sort(np.asarray(x, float))
    n = x.size
    F = np.asarray(cdf(x), float)
    i = np.arange(1, n + 1)
    return float(max(np.max(i / n - F), np.max(F - (i - 1) / n))), n


def assert_ks(x, cdf, what=""):
    """D sqrt(n) < 2.7."""
    d, n = ks_stat(x, cdf)
    assert d * math.sqrt(n) < KS_BOUND, (what, f"D={d:.3g} n={n} D*sqrt(n)={d * math.sqrt(n):.2f}")


def ks2_stat(a, b):
    """Two-sample Kolmogorov-Smirnov D and n_eff = n m / (n + m)."""
    a, b = np.sort(np.asarray(a, float)), np.sort(np.asarray(b, float))
    allv = np.concatenate((a, b))
    fa = np.searchsorted(a, allv, side="right") / a.size
    fb = np.searchsorted(b, allv, side="right") / b.size
    return float(np.max(np.abs(fa - fb))), a.size * b.size / (a.size + b.size)


def assert_ks2(a, b, what=""):
    """D sqrt(n_eff) < 2.7."""
    d, neff = ks2_stat(a, b)
    assert d * math.sqrt(neff) < KS_BOUND, (what, f"D={d:.3g} n_eff={neff:.0f} D*sqrt(n_eff)={d * math.sqrt(neff):.2f}")


def welch_z(mean_a, var_a, n_a, mean_b, var_b=0.0, n_b=math.inf):
    """(mean_a - mean_b) / sqrt(var_a / n_a + var_b / n_b); with b left out, against a known mean."""
    se = math.sqrt(var_a / n_a + (0.0 if math.isinf(n_b) else var_b / n_b))
    return (mean_a - mean_b) / se


def assert_mean(x, mean, what=""):
    """Sample mean of x against a known mean: |Welch z| < 5 with the sample variance."""
    x = np.asarray(x, float)
    z = welch_z(float(x.mean()), float(x.var(ddof=1)), x.size, mean)
    assert abs(z) < Z_BOUND, (what, f"mean={x.mean():.6g} want {mean:.6g} z={z:.2f}")
