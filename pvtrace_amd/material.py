"""Materials: refractive index, surface delegates and volume components.

Constructor-level mirror of the reference's material package
(pvtrace/material/material.py:10-63, component.py:33-440, distribution.py:8-193,
surface.py:13-272, utils.py:8-186).  These objects only *describe* a material:
the flattener (`pvtrace_amd.engine.compiler`) lowers them to SoA tables and the
HIP kernel does all per-photon sampling.  The scalar helper functions
(`fresnel_reflectivity`, `cone`, ...) are kept because user scenes pass them as
delegates (e.g. ``functools.partial(cone, theta)``) and tests use them as known
answers.
"""
import abc
import math
from dataclasses import replace

import numpy as np

from pvtrace_amd.lattice import Lattice, cell_clamped, cell_inside, check_axis, fmax, slot, walk

Q_E = 1.60217662e-19  # C
KB_EV = 1.380649e-23 / Q_E  # eV / K   (reference component.py:25-26)


# ----------------------------------------------------------------------
# Optics helpers (reference material/utils.py:8-45)

def fresnel_reflectivity(angle, n1, n2):
    """Unpolarised Fresnel reflectivity; 1.0 beyond the critical angle."""
    if n2 < n1 and angle > math.asin(n2 / n1):
        return 1.0
    c, s = math.cos(angle), math.sin(angle)
    k = math.sqrt(1.0 - (n1 / n2 * s) ** 2)
    rs = ((n1 * c - n2 * k) / (n1 * c + n2 * k)) ** 2
    rp = ((n1 * k - n2 * c) / (n1 * k + n2 * c)) ** 2
    return 0.5 * (rs + rp)


def specular_reflection(direction, normal):
    d = np.asarray(direction, dtype=np.float64)
    n = np.asarray(normal, dtype=np.float64)
    if np.dot(n, d) < 0.0:
        n = -n
    return d - 2.0 * np.dot(n, d) * n


def fresnel_refraction(direction, normal, n1, n2):
    """Snell refraction, vector form; `normal` must point along the ray."""
    d = np.asarray(direction, dtype=np.float64)
    nrm = np.asarray(normal, dtype=np.float64)
    n = n1 / n2
    dd = float(np.dot(d, nrm))
    c = math.sqrt(1.0 - n * n * (1.0 - dd * dd))
    sign = -1.0 if dd < 0.0 else 1.0
    return n * d + sign * (c - sign * n * dd) * nrm


def gaussian(x, c1, c2, c3):
    return c1 * np.exp(-(((c2 - x) / c3) ** 2))


def bandgap(x, cutoff, alpha):
    return (1 - np.heaviside(x - cutoff, 0.5)) * alpha


def simple_convert_spectum(spec):
    """(n, 2) spectrum with its x column turned from nanometres into electron-volts or back (E [eV] = hc/q 10^9 / nm is
    its own inverse); the y column untouched.  (The reference's helper of this -- misspelt -- name, material/utils.py:59-69.)"""
    out = np.array(spec)
    out[:, 0] = (6.62607015e-34 * 299792458.0 / 1.60217662e-19 * 1e9) / out[:, 0]
    return out


def thermodynamic_emission(abs_spec, T=300, mu=0.5):
    """Emission line shape in detailed balance with an absorption spectrum (generalised Planck
    law): `abs_spec` is an (n, 2) array of (nm, absorptance); returns (nm, emission) normalised to
    a peak of 1.  `T` in kelvin, `mu` the chemical potential in eV.  (Counterpart of the
    reference's pvtrace/material/utils.py:72-85, used to build test spectra.)"""
    planck, light, charge, boltzmann = 6.62607015e-34, 299792458.0, 1.60217662e-19, 1.38064852e-23
    spec = np.asarray(abs_spec, dtype=np.float64)
    ev = planck * light / charge * 1e9 / spec[:, 0]                  # photon energy of each row
    occupation = np.expm1((ev - mu) / (boltzmann / charge * T))
    emission = spec[:, 1] * ev * ev / occupation
    return np.column_stack((spec[:, 0], emission / np.max(emission)))


def spherical_to_cart(theta, phi, r=1):
    cart = np.column_stack((r * np.sin(theta) * np.cos(phi), r * np.sin(theta) * np.sin(phi), r * np.cos(theta)))
    return cart[0, :] if cart.size == 3 else cart


# ----------------------------------------------------------------------
# Phase functions / angular distributions (reference material/utils.py:104-186).
# The engine recognises these by identity / type and samples them on the
# device; calling them directly draws from numpy's global generator -- with numpy's
# own arccos / arcsin / sin / cos, as the reference's do: under one numpy seed the
# two packages return the same directions to the last bit (tests/golden/object_methods.npz).

def isotropic():
    g1, g2 = np.random.uniform(0, 1, 2)
    return spherical_to_cart(np.arccos(2 * g2 - 1), 2 * np.pi * g1)


def henyey_greenstein(g=0.0):
    p = np.random.uniform(0, 1)
    if abs(g) < 2.220446049250313e-13:
        return isotropic()
    s = 2 * p - 1
    mu = 1 / (2 * g) * (1 + g ** 2 - ((1 - g ** 2) / (1 + g * s)) ** 2)
    mu = min(max(mu, -1.0), 1.0)   # the quotient may leave [-1, 1] by a few ulp (small |g|, p = 0): arccos would be NaN
    phi = 2 * np.pi * np.random.uniform()
    return spherical_to_cart(np.arccos(mu), phi)


def cone(theta_max):
    if np.isclose(theta_max, 0.0) or theta_max > np.pi / 2:
        raise ValueError("Expected 0 < theta_max <= pi/2")
    p1, p2 = np.random.uniform(0, 1, 2)
    return spherical_to_cart(np.arcsin(np.sqrt(p1) * np.sin(theta_max)), 2 * np.pi * p2)


def lambertian():
    p1, p2 = np.random.uniform(0, 1, 2)
    return spherical_to_cart(np.arcsin(np.sqrt(p1)), 2 * np.pi * p2)


class HenyeyGreenstein(object):
    def __init__(self, g):
        self.g = float(g)

    def __call__(self):
        return henyey_greenstein(self.g)


class Cone(object):
    def __init__(self, theta_max):
        self.theta_max = float(theta_max)

    def __call__(self):
        return cone(self.theta_max)


# ----------------------------------------------------------------------
# Spectral distribution (reference material/distribution.py:8-193)

class Distribution(object):
    """A sampled spectrum y(x) with its cumulative distribution.

    With ``hist=False`` the CDF is the trapezoid integral normalised to 1 with a
    leading 0 (`_cdf` has the same length as `_x`); this is what the device
    kernel inverts for emission-wavelength sampling.  A constant is represented
    by ``x=None`` and a float `y`.
    """

    def __init__(self, x, y, hist=False):
        self.hist = hist
        if x is None and isinstance(y, float):
            self._x, self._y = None, y
            return
        x = np.asarray(x)
        y = np.asarray(y)
        if not np.all(np.diff(x) > 0):
            raise ValueError("x must be sorted and ascending.")
        if not np.isfinite(y).any():
            raise ValueError("All values of y must be finite.")
        if np.any(y < 0.0):
            raise ValueError(
                "Distributions are like histograms all counts must be positive."
            )
        self._x_range = (np.min(x), np.max(x))
        self._x, self._y = x, y
        if hist:
            cdf = np.cumsum(y, dtype=float)
            cdf *= 1.0 / cdf[-1]
            self._cdf = cdf
            self._edges = np.insert(x, x.size, 2 * x[-1] - x[-2])
        else:
            cdf = np.cumsum((y[:-1] + y[1:]) * 0.5)
            cdf = cdf / np.max(cdf)
            self._cdf = np.hstack([0.0, cdf])

    def _check(self, v, lo, hi, what):
        arr = np.asarray(v)
        if np.any(arr < lo) or np.any(arr > hi):
            raise ValueError(what, {"value": v, "range": (lo, hi)})

    def __call__(self, x):
        if self._x is None:
            if isinstance(x, (list, tuple, np.ndarray)):
                return np.zeros(len(x)) + self._y
            return self._y
        self._check(x, *self._x_range, "x is outside data range.")
        if self.hist:
            return self._y[np.searchsorted(self._edges[:-1], x)]
        return np.interp(x, self._x, self._y, left=np.nan, right=np.nan)

    def lookup(self, x):
        """CDF value at x."""
        self._check(x, *self._x_range, "x is outside data range.")
        if self.hist:
            return self._cdf[np.searchsorted(self._edges[:-1], x)]
        prob = np.interp(x, self._x, self._cdf, left=np.nan, right=np.nan)
        return prob.tolist() if np.size(prob) == 1 else prob

    def sample(self, p):
        """Inverse CDF."""
        self._check(p, 0.0, 1.0, "p is outside valid range.")
        if self.hist:
            idx = np.searchsorted(self._cdf, p)
            try:
                return self._x[idx]
            except IndexError:
                return self._x[-1]
        xval = np.interp(p, self._cdf, self._x, left=np.nan, right=np.nan)
        return xval.tolist() if np.size(xval) == 1 else xval

    @classmethod
    def from_functions(cls, x, callables, hist=False):
        x = np.array(x)
        if x.ndim != 1:
            raise ValueError("Requires a 1D array.")
        y = np.zeros(len(x))
        for f in callables:
            part = f(x)
            part[np.where(~np.isfinite(part))] = 0.0
            y += part
        return cls(x=x, y=y, hist=hist)


# ----------------------------------------------------------------------
# Surfaces (reference material/surface.py:13-272)

class SurfaceDelegate(abc.ABC):
    """Per-interaction surface behaviour.  Arbitrary Python delegates cannot
    run on the device; the flattener accepts the built-in delegates below and
    declarative `CoatedSurfaceDelegate` objects, and rejects everything else
    with `UnsupportedSceneError` (as the reference compiler does,
    pvtrace/engine/compiler.py:237-247)."""

    @abc.abstractmethod
    def reflectivity(self, surface, ray, geometry, container, adjacent):
        pass

    @abc.abstractmethod
    def reflected_direction(self, surface, ray, geometry, container, adjacent):
        pass

    @abc.abstractmethod
    def transmitted_direction(self, surface, ray, geometry, container, adjacent):
        pass


def _flipped_normal(geometry, ray):
    normal = np.asarray(geometry.normal(ray.position), dtype=np.float64)
    if np.dot(normal, ray.direction) < 0.0:
        normal = -normal
    return normal


def index_at(material, wavelength):
    """The refractive index of `material` at `wavelength` (nm): its `RefractiveIndexTable` evaluated there, or its
    scalar index AS IT IS.  The one place the host evaluates an index (`Material.refractive_index_at` is this, as a
    float).  The surface delegates call it directly: they are handed any object with a `refractive_index` (the
    reference's duck-typed nodes, rays without a wavelength), and a scalar index passed on unconverted keeps their
    arithmetic what it was, float for float."""
    n = material.refractive_index
    if isinstance(n, RefractiveIndexTable):
        return n.at(wavelength)
    return n


def _check_roughness(roughness):
    a = float(roughness)
    if not (math.isfinite(a) and 0.0 <= a <= 1.0):
        raise ValueError(f"roughness must be a finite GGX width alpha with 0 <= alpha <= 1, got {roughness!r}")
    return a


def ggx_visible_normal(normal, direction, alpha, ua, ub):
    """Step 2 of the rough-interface contract (`FresnelSurfaceDelegate`): the microfacet normal m drawn from the GGX
    distribution of visible normals (Heitz 2018, JCGT 7(4)) of width `alpha` for a photon travelling along `direction`
    towards a surface of geometric normal `normal` (either orientation; it is turned to face the photon).  Every
    argument may carry leading batch dimensions; (n, 3) directions with (n,) draws give (n, 3) normals."""
    d = np.asarray(direction, dtype=np.float64)
    nrm = np.asarray(normal, dtype=np.float64)
    a = np.asarray(alpha, dtype=np.float64)[..., None]
    ua = np.asarray(ua, dtype=np.float64)[..., None]
    ub = np.asarray(ub, dtype=np.float64)[..., None]
    facing = np.where(np.sum(d * nrm, axis=-1, keepdims=True) > 0.0, -nrm, nrm)   # d . N <= 0
    v = -d
    e1, e2 = ray_basis(facing)
    vx = np.sum(v * e1, axis=-1, keepdims=True)
    vy = np.sum(v * e2, axis=-1, keepdims=True)
    vz = np.sum(v * facing, axis=-1, keepdims=True)
    hx, hy, hz = a * vx, a * vy, vz
    inv = 1.0 / np.sqrt(hx * hx + hy * hy + hz * hz)
    hx, hy, hz = hx * inv, hy * inv, hz * inv
    lensq = hx * hx + hy * hy
    safe = np.where(lensq > 0.0, lensq, 1.0)
    il = 1.0 / np.sqrt(safe)
    t1x = np.where(lensq > 0.0, -hy * il, 1.0)
    t1y = np.where(lensq > 0.0, hx * il, 0.0)
    t2x, t2y, t2z = -hz * t1y, hz * t1x, hx * t1y - hy * t1x   # Vh x T1, T1.z = 0
    r = np.sqrt(ua)
    phi = 2.0 * np.pi * ub
    t1 = r * np.cos(phi)
    s = 0.5 * (1.0 + hz)
    t2 = (1.0 - s) * np.sqrt(1.0 - t1 * t1) + s * r * np.sin(phi)
    tz = np.sqrt(np.maximum(0.0, 1.0 - t1 * t1 - t2 * t2))
    nx = t1 * t1x + t2 * t2x + tz * hx
    ny = t1 * t1y + t2 * t2y + tz * hy
    nz = t2 * t2z + tz * hz
    mx, my, mz = a * nx, a * ny, np.maximum(0.0, nz)
    inv = 1.0 / np.sqrt(mx * mx + my * my + mz * mz)
    return (mx * inv) * e1 + (my * inv) * e2 + (mz * inv) * facing


def rough_fresnel_reflectivity(cos_m, n1, n2):
    """Step 3: the unpolarised Fresnel reflectivity about a microfacet, from cos(theta_m) = v . m (clamped to [0, 1]):
    the smooth branch's Hecht formula, 1.0 where q = n1 / n2 sin(theta_m) >= 1 (total internal reflection)."""
    c = min(max(float(cos_m), 0.0), 1.0)
    q = n1 / n2 * math.sqrt((1.0 - c) * (1.0 + c))
    if q >= 1.0:
        return 1.0
    k = math.sqrt(1.0 - q * q)
    rs = ((n1 * c - n2 * k) / (n1 * c + n2 * k)) ** 2
    rp = ((n1 * k - n2 * c) / (n1 * k + n2 * c)) ** 2
    return 0.5 * (rs + rp)


def rough_directions(direction, normal, m, n1, n2):
    """Steps 5 and 6: (reflected, transmitted) directions of a photon travelling along `direction` about the microfacet
    normal `m` (v . m > 0), each folded back across the tangent plane of the geometric `normal` when it lies on the
    wrong side of it.  The transmitted one is None under total internal reflection about m."""
    d = np.asarray(direction, dtype=np.float64)
    nrm = np.asarray(normal, dtype=np.float64)
    along = nrm if float(np.dot(nrm, d)) >= 0.0 else -nrm   # the geometric normal along the ray (-N)
    m = np.asarray(m, dtype=np.float64)
    dm = float(np.dot(d, m))
    reflected = d - 2.0 * dm * m
    if float(np.dot(reflected, along)) > 0.0:
        reflected = reflected - 2.0 * float(np.dot(reflected, along)) * along
    nf = -m                                  # the microfacet normal along the ray, as Snell's vector form takes it
    dd = min(max(-dm, 0.0), 1.0)
    n = n1 / n2
    c2 = 1.0 - n * n * (1.0 - dd * dd)
    if c2 < 0.0:
        return reflected, None
    transmitted = n * d + (math.sqrt(c2) - n * dd) * nf
    if float(np.dot(transmitted, along)) < 0.0:
        transmitted = transmitted - 2.0 * float(np.dot(transmitted, along)) * along
    return reflected, transmitted


class FresnelSurfaceDelegate(SurfaceDelegate):
    """Fresnel reflection / Snell refraction from the two refractive indices.

    roughness : the GGX (Trowbridge-Reitz) width alpha of the interface, finite, 0 <= alpha <= 1 (default 0: an
        optically perfect interface, exactly as before).  It is the roughness of the surface of the node that is HIT.

    A rough interface draws a microfacet normal per surface event and applies Fresnel and Snell about it.  The
    sampling contract, the same on the host and on the device (include/pvtrace_hip.h):

    1. Frame.  N is the geometric normal at the hit turned to face the photon (d . N < 0), v = -d, (e1, e2) =
       `ray_basis(N)` (Duff et al. 2017), v_l = (v . e1, v . e2, v . N).
    2. Microfacet normal (GGX visible normals, Heitz 2018): draw u_a, then u_b.
       Vh = normalize(alpha v_l.x, alpha v_l.y, v_l.z); T1 = (-Vh.y, Vh.x, 0) / sqrt(Vh.x^2 + Vh.y^2), or (1, 0, 0)
       when that sum is 0; T2 = Vh x T1; r = sqrt(u_a), phi = 2 pi u_b (pvt_sincos2pi on the device);
       t1 = r cos(phi), s = (1 + Vh.z) / 2, t2 = (1 - s) sqrt(1 - t1^2) + s r sin(phi);
       Nh = t1 T1 + t2 T2 + sqrt(max(0, 1 - t1^2 - t2^2)) Vh; m_l = normalize(alpha Nh.x, alpha Nh.y, max(0, Nh.z));
       m = m_l.x e1 + m_l.y e2 + m_l.z N, so that v . m > 0.
    3. Fresnel about m: cos(theta_m) = v . m clamped to [0, 1], n1 and n2 at the photon's wavelength; the smooth
       branch's Hecht formula, R = 1 where q = n1 / n2 sin(theta_m) >= 1 (total internal reflection about m).
    4. Decision: the reflect-or-transmit draw u as before, only when R > 0.
    5. Direction: reflection d' = d - 2 (d . m) m; transmission by the smooth branch's vector form of Snell's law with
       m in place of the normal.
    6. Fold: a reflected d' with d' . N < 0 or a transmitted d' with d' . N > 0 is mirrored across the tangent plane,
       d' <- d' - 2 (d' . N) N (no draw).
    7. Draw order u_a, u_b, then u (if R > 0); event kinds, recorder selectors and the logged normal (the geometric
       one) follow the smooth rules.

    On the host `reflectivity()` draws u_a and u_b from numpy's global generator and keeps m; `reflected_direction()`
    and `transmitted_direction()` of the same ray use that m.
    """

    def __init__(self, roughness=0.0):
        super(FresnelSurfaceDelegate, self).__init__()
        self._roughness = _check_roughness(roughness)
        self._facet = None   # ((position, direction), m) of the last microfacet drawn

    @property
    def roughness(self):
        return getattr(self, "_roughness", 0.0)   # (subclasses that skip __init__ stay smooth)

    def _rough_here(self, ray, geometry):
        """True when this event samples a microfacet (a rough surface; coated points never do)."""
        return self.roughness > 0.0

    def _indices(self, ray, container, adjacent):
        wl = getattr(ray, "wavelength", None)
        return index_at(container.geometry.material, wl), index_at(adjacent.geometry.material, wl)

    def _microfacet(self, ray, geometry, draw):
        """The microfacet normal of this event: the one reflectivity() drew for the same ray, else (draw=True) a new one."""
        key = (tuple(np.asarray(ray.position, dtype=np.float64).tolist()),
               tuple(np.asarray(ray.direction, dtype=np.float64).tolist()))
        facet = getattr(self, "_facet", None)
        if facet is not None and facet[0] == key and not draw:
            return facet[1]
        ua = np.random.uniform()
        ub = np.random.uniform()
        normal = np.asarray(geometry.normal(ray.position), dtype=np.float64)
        m = ggx_visible_normal(normal, ray.direction, self.roughness, ua, ub)
        self._facet = (key, m)
        return m

    def _smooth_reflectivity(self, surface, ray, geometry, container, adjacent):
        n1, n2 = self._indices(ray, container, adjacent)
        normal = _flipped_normal(geometry, ray)
        cosang = float(np.clip(np.dot(normal, ray.direction), -1.0, 1.0))
        return float(fresnel_reflectivity(math.acos(cosang), n1, n2))

    def reflectivity(self, surface, ray, geometry, container, adjacent):
        if not self._rough_here(ray, geometry):
            return self._smooth_reflectivity(surface, ray, geometry, container, adjacent)
        n1, n2 = self._indices(ray, container, adjacent)
        m = self._microfacet(ray, geometry, draw=True)
        return rough_fresnel_reflectivity(-float(np.dot(np.asarray(ray.direction, dtype=np.float64), m)), n1, n2)

    def reflected_direction(self, surface, ray, geometry, container, adjacent):
        normal = geometry.normal(ray.position)
        if self._rough_here(ray, geometry):
            n1, n2 = self._indices(ray, container, adjacent)
            reflected, _ = rough_directions(ray.direction, normal, self._microfacet(ray, geometry, draw=False), n1, n2)
            return tuple(reflected.tolist())
        return tuple(specular_reflection(ray.direction, normal).tolist())

    def transmitted_direction(self, surface, ray, geometry, container, adjacent):
        n1, n2 = self._indices(ray, container, adjacent)
        if self._rough_here(ray, geometry):
            m = self._microfacet(ray, geometry, draw=False)
            _, transmitted = rough_directions(ray.direction, geometry.normal(ray.position), m, n1, n2)
            if transmitted is None:
                raise ValueError("no transmitted direction: total internal reflection about the microfacet normal")
            return tuple(transmitted.tolist())
        normal = _flipped_normal(geometry, ray)
        return tuple(fresnel_refraction(ray.direction, normal, n1, n2).tolist())


class NullSurfaceDelegate(SurfaceDelegate):
    """Transmits everything without refraction (useful for counting)."""

    def reflectivity(self, surface, ray, geometry, container, adjacent):
        return 0.0

    def reflected_direction(self, surface, ray, geometry, container, adjacent):
        raise NotImplementedError("This surface delegate does not reflect.")

    def transmitted_direction(self, surface, ray, geometry, container, adjacent):
        return ray.direction


def _bracket(axis, x):
    """(lo, hi, t) of the piecewise-linear, end-clamped interpolation of `axis` at `x` (the `interp_clamped`
    convention): lo = hi at and beyond either end, else axis[lo] <= x < axis[hi] and t = (x - axis[lo]) / width."""
    n = len(axis)
    if not x > axis[0]:
        return 0, 0, 0.0
    if not x < axis[n - 1]:
        return n - 1, n - 1, 0.0
    lo = int(np.searchsorted(axis, x, side="right")) - 1
    return lo, lo + 1, (x - axis[lo]) / (axis[lo + 1] - axis[lo])


class ReflectivityTable(object):
    """Reflectivity of a coating as a table R(wavelength, angle of incidence).

    wavelength : strictly increasing wavelengths in nm.
    values : shape (n_angle, n_wavelength), or (n_wavelength,) when `angle` is omitted; finite, in [0, 1].
    angle : strictly increasing angles of incidence in degrees, in [0, 90], measured from the surface normal on the
        side the photon arrives from; None = the reflectivity does not depend on the angle.

    `at(wavelength, angle)` interpolates piecewise-linearly in wavelength, then in angle, clamping at both ends of
    each axis, each step formed as a + t (b - a), so a table holding a constant c evaluates to exactly c.  This is
    what the device computes per photon at the photon's current wavelength.
    """

    def __init__(self, wavelength, values, angle=None):
        wl = np.array(wavelength, dtype=np.float64)
        if wl.ndim != 1 or wl.size < 1:
            raise ValueError("wavelength must be a non-empty 1-D sequence")
        if not np.all(np.isfinite(wl)) or np.any(np.diff(wl) <= 0.0):
            raise ValueError("wavelength must be finite and strictly increasing")
        if angle is None:
            ang = np.zeros(1, dtype=np.float64)
            vals = np.array(values, dtype=np.float64)
            if vals.shape != (wl.size,):
                raise ValueError(
                    f"values must have shape (n_wavelength,) = ({wl.size},) when angle is omitted, got {vals.shape}"
                )
            vals = vals.reshape(1, wl.size)
        else:
            ang = np.array(angle, dtype=np.float64)
            if ang.ndim != 1 or ang.size < 1:
                raise ValueError("angle must be a non-empty 1-D sequence")
            if not np.all(np.isfinite(ang)) or np.any(np.diff(ang) <= 0.0):
                raise ValueError("angle must be finite and strictly increasing")
            if ang[0] < 0.0 or ang[-1] > 90.0:
                raise ValueError("angle must lie in [0, 90] degrees")
            vals = np.array(values, dtype=np.float64)
            if vals.shape != (ang.size, wl.size):
                raise ValueError(
                    f"values must have shape (n_angle, n_wavelength) = ({ang.size}, {wl.size}), got {vals.shape}"
                )
        if not np.all(np.isfinite(vals)) or np.any(vals < 0.0) or np.any(vals > 1.0):
            raise ValueError("values must be finite and in [0, 1]")
        self.wavelength = wl
        self.angle = None if angle is None else ang
        self.values = vals if angle is not None else vals[0]
        self._angle_axis = ang
        self._grid = vals

    def at(self, wavelength, angle=0.0):
        """R at `wavelength` (nm) and angle of incidence `angle` (degrees)."""
        wl_lo, wl_hi, tw = _bracket(self.wavelength, float(wavelength))
        a_lo, a_hi, ta = _bracket(self._angle_axis, float(angle))
        g = self._grid
        r0 = g[a_lo, wl_lo] + tw * (g[a_lo, wl_hi] - g[a_lo, wl_lo])
        r1 = g[a_hi, wl_lo] + tw * (g[a_hi, wl_hi] - g[a_hi, wl_lo])
        return float(r0 + ta * (r1 - r0))


# The absorptivity of a coating A(wavelength, angle of incidence) is tabulated by the same class, with the same contract,
# `at()` and clamping; the alias lets user code say what the numbers are.
AbsorptivityTable = ReflectivityTable


def _coating_sum_exceeds_one(reflectivity, absorptivity):
    """(wavelength, angle, R, A) of a point where R + A > 1, or None.  A table on either side is evaluated with the other
    side on the outer product of the union of the wavelength grids and the union of the angle grids: clamped bilinear
    interpolants take their maximum at such vertices, so the check is exact."""
    tables = [v for v in (reflectivity, absorptivity) if isinstance(v, ReflectivityTable)]
    if not tables:
        r, a = float(reflectivity), float(absorptivity)
        return (None, None, r, a) if r + a > 1.0 else None
    wavelengths = np.unique(np.concatenate([t.wavelength for t in tables]))
    angles = np.unique(np.concatenate([t._angle_axis for t in tables]))

    def at(value, wl, angle):
        return value.at(wl, angle) if isinstance(value, ReflectivityTable) else float(value)

    for angle in angles:
        for wl in wavelengths:
            r, a = at(reflectivity, wl, angle), at(absorptivity, wl, angle)
            if r + a > 1.0:
                return float(wl), float(angle), r, a
    return None


class RefractiveIndexTable(object):
    """Refractive index of a material as a table n(wavelength): dispersion.

    wavelength : strictly increasing wavelengths in nm, at least one.
    values : the index at each wavelength; finite and positive, in (1e-100, 1e100) like every index the engine takes.

    `at(wavelength)` interpolates piecewise-linearly, clamping at both ends, each step formed as a + t (b - a), so a
    table holding a constant c evaluates to exactly c.  This is what the device computes per photon at the photon's
    current wavelength, wherever the scalar index would be used: Fresnel reflectivity, the critical angle, Snell
    refraction and the time of flight (the phase index).
    """

    def __init__(self, wavelength, values):
        wl = np.array(wavelength, dtype=np.float64)
        if wl.ndim != 1 or wl.size < 1:
            raise ValueError("wavelength must be a non-empty 1-D sequence")
        if not np.all(np.isfinite(wl)) or np.any(np.diff(wl) <= 0.0):
            raise ValueError("wavelength must be finite and strictly increasing")
        vals = np.array(values, dtype=np.float64)
        if vals.shape != (wl.size,):
            raise ValueError(f"values must have shape (n_wavelength,) = ({wl.size},), got {vals.shape}")
        if not np.all(np.isfinite(vals)) or np.any(vals <= 1e-100) or np.any(vals >= 1e100):
            # (the bounds the engine holds every index to, scalar or tabulated: the device divides by them)
            raise ValueError("values must be finite and positive, in (1e-100, 1e100)")
        self.wavelength = wl
        self.values = vals

    def at(self, wavelength):
        """n at `wavelength` (nm)."""
        lo, hi, t = _bracket(self.wavelength, float(wavelength))
        a = self.values[lo]
        return float(a + t * (self.values[hi] - a))

    @classmethod
    def from_sellmeier(cls, B, C, wavelength):
        """Tabulate the Sellmeier equation n^2 = 1 + sum_i B_i lam^2 / (lam^2 - C_i) (lam in um, C_i in um^2) at the
        wavelengths `wavelength` (nm).  Host only: the device interpolates the table."""
        B = np.asarray(B, dtype=np.float64)
        C = np.asarray(C, dtype=np.float64)
        if B.ndim != 1 or B.shape != C.shape:
            raise ValueError("B and C must be 1-D sequences of the same length")
        lam2 = (np.asarray(wavelength, dtype=np.float64) * 1e-3) ** 2
        n2 = 1.0 + np.sum(B[:, None] * lam2[None, :] / (lam2[None, :] - C[:, None]), axis=0)
        if not np.all(n2 > 0.0):
            raise ValueError("the Sellmeier equation gives no real index on this grid")
        return cls(wavelength, np.sqrt(n2))


def ray_basis(direction):
    """(e1, e2): the orthonormal basis about the unit vector `direction` = (x, y, z) that tabulated phase functions
    scatter in (Duff et al. 2017, "Building an orthonormal basis, revisited"), branch-free:
    s = copysign(1, z), a = -1 / (s + z), b = x y a,
    e1 = (1 + s x^2 a, s b, -s x), e2 = (b, s + y^2 a, -y).
    `direction` may be (3,) or (n, 3); the device evaluates the same expressions."""
    d = np.asarray(direction, dtype=np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    s = np.copysign(1.0, z)
    a = -1.0 / (s + z)
    b = x * y * a
    e1 = np.stack([1.0 + s * x * x * a, s * b, -s * x], axis=-1)
    e2 = np.stack([b, s + y * y * a, -y], axis=-1)
    return e1, e2


class PhaseFunctionTable(object):
    """A tabulated phase function p(theta), optionally one row per wavelength, sampled about the INCOMING direction.

    angle : scattering angles theta in degrees, strictly increasing from exactly 0 to exactly 180, at least 2.
    values : p(theta) per unit solid angle, unnormalised, finite and >= 0, each row with a positive integral; shape
        (n_angle,) without `wavelength`, else (n_wavelength, n_angle).
    wavelength : None, or strictly increasing finite wavelengths in nm, one per row of `values`.

    Unlike the built-in phase functions, which draw about +z, the scattering angle is measured from the photon's
    incoming direction d.  The sampling contract, the same on the host and on the device (include/pvtrace_hip.h):

    1. Axis and CDF.  mu_j = cos(theta_j), reordered so mu runs from -1 to 1, the ends exactly -1 and 1.  Each row's
       CDF in mu is the trapezoid integral sum 0.5 (p_j + p_j+1)(mu_j+1 - mu_j) with a leading 0, divided by its last
       entry, which is then exactly 1 (the structure of `Distribution(hist=False)`, with the widths of the mu axis).
    2. Row, only when n_wavelength > 1: clamp the photon's wavelength lambda into the table's range, find k with
       lambda_k <= lambda < lambda_k+1, t = (lambda - lambda_k) / (lambda_k+1 - lambda_k) (t = 0 at either clamped
       end, the last row above the range); draw u1 and take row k+1 if u1 < t, else row k: the linear-in-lambda mixture
       of the normalised rows.  u1 is drawn whenever n_wavelength > 1.  Without a wavelength (a light's direction),
       the first row is used, u1 still drawn.
    3. Polar angle: draw u2; j is the first segment with C_j+1 > u2 (segments of zero mass are never chosen);
       mu = mu_j + (u2 - C_j) / (C_j+1 - C_j) (mu_j+1 - mu_j), clamped to [-1, 1].
    4. Azimuth: draw u3, phi = 2 pi u3 (pvt_sincos2pi on the device); the new direction is
       d' = mu d + sqrt(1 - mu^2) (cos(phi) e1 + sin(phi) e2), (e1, e2) = `ray_basis(d)`.
    5. Draw order: u1 (if drawn), u2, u3, in place of the built-ins' phase-function draws; a luminophore's wavelength
       and delay draws follow as before.

    As a light's `direction`, the incoming direction is the light's +z: `sample(n)` gives a bundle, a call without
    arguments one direction.
    """

    def __init__(self, angle, values, wavelength=None):
        ang = np.array(angle, dtype=np.float64)
        if ang.ndim != 1 or ang.size < 2:
            raise ValueError("angle must be a 1-D sequence of at least 2 scattering angles")
        if not np.all(np.isfinite(ang)) or np.any(np.diff(ang) <= 0.0):
            raise ValueError("angle must be finite and strictly increasing")
        if ang[0] != 0.0 or ang[-1] != 180.0:
            raise ValueError("angle must start at exactly 0 and end at exactly 180 degrees")
        vals = np.array(values, dtype=np.float64)
        if wavelength is None:
            if vals.shape != (ang.size,):
                raise ValueError(f"values must have shape (n_angle,) = ({ang.size},), got {vals.shape}")
            wl = None
            rows = vals[None, :]
        else:
            wl = np.array(wavelength, dtype=np.float64)
            if wl.ndim != 1 or wl.size < 1:
                raise ValueError("wavelength must be a non-empty 1-D sequence")
            if not np.all(np.isfinite(wl)) or np.any(np.diff(wl) <= 0.0):
                raise ValueError("wavelength must be finite and strictly increasing")
            if vals.shape != (wl.size, ang.size):
                raise ValueError(
                    f"values must have shape (n_wavelength, n_angle) = ({wl.size}, {ang.size}), got {vals.shape}")
            rows = vals
        if not np.all(np.isfinite(vals)) or np.any(vals < 0.0):
            raise ValueError("values must be finite and >= 0")
        mu = np.cos(np.radians(ang))[::-1].copy()
        mu[0], mu[-1] = -1.0, 1.0
        if np.any(np.diff(mu) <= 0.0):
            raise ValueError("angle: neighbouring angles too close to give distinct cosines")
        p = rows[:, ::-1]
        cdf = np.cumsum(0.5 * (p[:, :-1] + p[:, 1:]) * np.diff(mu)[None, :], axis=1)
        total = cdf[:, -1:]
        if not np.all(np.isfinite(total)) or np.any(total <= 0.0):
            raise ValueError("every row of values must have a positive, finite integral")
        cdf = np.hstack([np.zeros((rows.shape[0], 1)), cdf / total])
        cdf[:, -1] = 1.0
        self.angle = ang
        self.values = vals
        self.wavelength = wl
        self.mu = mu
        self.cdf = cdf

    @property
    def n_wavelength(self):
        return self.cdf.shape[0]

    def rows(self, wavelength, u1):
        """The row each photon takes (step 2): `wavelength` and `u1` scalars or arrays; None = the first row."""
        u1 = np.asarray(u1, dtype=np.float64)
        if self.n_wavelength == 1 or wavelength is None:
            return np.zeros(u1.shape, dtype=np.int64)
        wl = np.broadcast_to(np.asarray(wavelength, dtype=np.float64), u1.shape)
        axis = self.wavelength
        n = axis.size
        lo = np.clip(np.searchsorted(axis, wl, side="right") - 1, 0, n - 1)
        hi = np.minimum(lo + 1, n - 1)
        inside = (wl > axis[0]) & (wl < axis[-1])
        t = np.where(inside, (wl - axis[lo]) / np.where(inside, axis[hi] - axis[lo], 1.0), 0.0)
        lo = np.where(wl < axis[-1], lo, n - 1)
        hi = np.where(inside, hi, lo)
        return np.where(u1 < t, hi, lo)

    def sample_mu(self, u2, row=0):
        """mu = cos(theta) of step 3 for the draws `u2` in the rows `row` (scalars or arrays)."""
        u2 = np.asarray(u2, dtype=np.float64)
        row = np.broadcast_to(np.asarray(row, dtype=np.int64), u2.shape)
        j = np.zeros(u2.shape, dtype=np.int64)
        for r in np.unique(row):   # the last C_j <= u2 is the first segment with C_j+1 > u2
            at = row == r
            j[at] = np.searchsorted(self.cdf[r], u2[at], side="right") - 1
        j = np.minimum(j, self.mu.size - 2)
        cj, cj1 = self.cdf[row, j], self.cdf[row, j + 1]
        mu = self.mu[j] + (u2 - cj) / (cj1 - cj) * (self.mu[j + 1] - self.mu[j])
        return np.clip(mu, -1.0, 1.0)

    def turn(self, direction, mu, u3):
        """Step 4: the direction at polar cosine `mu` and azimuth 2 pi `u3` about the unit vector(s) `direction`."""
        d = np.asarray(direction, dtype=np.float64)
        mu = np.asarray(mu, dtype=np.float64)[..., None]
        phi = 2.0 * np.pi * np.asarray(u3, dtype=np.float64)[..., None]
        e1, e2 = ray_basis(d)
        return mu * d + np.sqrt((1.0 - mu) * (1.0 + mu)) * (np.cos(phi) * e1 + np.sin(phi) * e2)

    def __call__(self, direction=None, wavelength=None):
        """One new direction about `direction` (None: +z, a light's axis) for a photon of `wavelength` (nm), drawn
        from numpy's global generator in the contract's order."""
        u1 = np.random.uniform() if self.n_wavelength > 1 else 0.0
        u2 = np.random.uniform()
        u3 = np.random.uniform()
        d = (0.0, 0.0, 1.0) if direction is None else direction
        mu = self.sample_mu(u2, self.rows(wavelength, u1))
        return self.turn(d, mu, u3)

    def sample(self, n):
        """(n, 3) directions about +z: a light's `direction` delegate, vectorised (engine/emit.py)."""
        n = int(n)
        k = 3 if self.n_wavelength > 1 else 2
        u = np.random.uniform(size=(n, k))
        row = self.rows(None, u[:, 0])
        mu = self.sample_mu(u[:, k - 2], row)
        return self.turn(np.array([0.0, 0.0, 1.0]), mu, u[:, k - 1])


class ScatterLobe(object):
    """Where a coating sends the light it reflects or transmits: a `PhaseFunctionTable` whose angle is measured from an
    axis of the surface event (extension; the reference writes such surfaces as Python delegates).

    table : a `PhaseFunctionTable` p(theta); theta is the angle between the outgoing direction and the axis.
    about : the axis.  As `Coating(reflection=...)`: "normal" or "specular".  As `Coating(transmission=...)`: "normal",
        "refracted" or "straight".

    The rule of a scattering coating, the same on the host and on the device (include/pvtrace_hip.h, "Scattering
    coatings", states the same):

    1. Coverage, R, A and the one outcome draw u are untouched: rules 1-5 of the absorbing coating and the rules of
       where a coating covers.  Beyond the critical angle a transmission lobe about "refracted" behaves as "fresnel": R
       stays 1.  Beyond the critical angle a lobe about "normal" or "straight" behaves as "matched": the coating's R
       applies.
    2. The outgoing normal.  With N the logged geometric normal and d the incoming direction, s = +1 if N . d < 0, else
       -1.  N_out = s N for a reflection and -s N for a transmission.
    3. The axis a.  "normal": N_out.  "specular": d - 2 (d . N) N, as the specular body forms it.  "refracted": the
       Snell direction, as the Fresnel body forms it, at the indices of the photon's wavelength.  "straight": d.
    4. The draws come after u: u1 (only when the table has more than one wavelength row), u2 and u3.  Steps 2-4 of the
       `PhaseFunctionTable` contract are applied about a at the photon's current wavelength, in the world frame, with
       no FMA, and give d'.
    5. The fold: if d' . N_out < 0, then d' <- d' - 2 (d' . N_out) N_out.  The fold takes no draw.  Exactly 0 stays.
    6. Event kind, recorder selector, the logged normal, the `reflections` counter, `Event.DETECT` and the rule that
       roughness applies only where no coating covers stay as for the built-in modes.
    """

    ABOUT = ("normal", "specular", "refracted", "straight")
    REFLECTION_ABOUT = {"normal": 0, "specular": 1}
    TRANSMISSION_ABOUT = {"normal": 0, "refracted": 2, "straight": 3}

    def __init__(self, table, about="normal"):
        if not isinstance(table, PhaseFunctionTable):
            raise ValueError("table must be a PhaseFunctionTable")
        if about not in self.ABOUT:
            raise ValueError(f"about must be one of {list(self.ABOUT)}")
        self.table = table
        self.about = about

    @classmethod
    def lambertian(cls, nodes=257, about="normal"):
        """The cosine lobe: p = cos(theta) up to 90 degrees and 0 beyond, a knot exactly at 90 degrees (`nodes` odd)."""
        nodes = int(nodes)
        if nodes < 3 or nodes % 2 == 0:
            raise ValueError("nodes must be odd and at least 3: 90 degrees is a knot")
        half = nodes // 2
        angle = np.concatenate([np.linspace(0.0, 90.0, half + 1), np.linspace(90.0, 180.0, half + 1)[1:]])
        values = np.where(angle < 90.0, np.cos(np.radians(angle)), 0.0)
        return cls(PhaseFunctionTable(angle, values), about=about)

    @classmethod
    def gaussian(cls, sigma_degrees, about, nodes=1025):
        """A Gaussian gloss lobe p = exp(-theta^2 / (2 sigma^2)) on `nodes` evenly spaced angles."""
        sigma = float(sigma_degrees)
        if not (math.isfinite(sigma) and sigma > 0.0):
            raise ValueError("sigma_degrees must be finite and > 0")
        nodes = int(nodes)
        if nodes < 3:
            raise ValueError("nodes must be at least 3")
        angle = np.linspace(0.0, 180.0, nodes)
        angle[-1] = 180.0
        if not sigma > angle[1] / 8.0:
            raise ValueError("sigma_degrees is too small for the angle grid: raise nodes")
        values = np.exp(-0.5 * (angle / sigma) ** 2)
        return cls(PhaseFunctionTable(angle, values), about=about)

    def turn(self, direction, normal, transmit, wavelength=None, n1=None, n2=None):
        """Rules 2-5 for one photon travelling along `direction` at a point of geometric `normal`: the new direction,
        its draws u1 (if the table has several rows), u2, u3 taken from numpy's global generator in that order."""
        d = np.asarray(direction, dtype=np.float64)
        nrm = np.asarray(normal, dtype=np.float64)
        s = 1.0 if float(np.dot(nrm, d)) < 0.0 else -1.0
        n_out = (-s if transmit else s) * nrm
        if self.about == "normal":
            axis = n_out
        elif self.about == "specular":
            axis = np.asarray(specular_reflection(d, nrm), dtype=np.float64)
        elif self.about == "refracted":
            axis = np.asarray(fresnel_refraction(d, -s * nrm, n1, n2), dtype=np.float64)
        else:
            axis = d
        table = self.table
        u1 = np.random.uniform() if table.n_wavelength > 1 else 0.0
        u2 = np.random.uniform()
        u3 = np.random.uniform()
        mu = table.sample_mu(u2, table.rows(wavelength, u1))
        out = np.asarray(table.turn(axis, mu, u3), dtype=np.float64)
        across = float(np.dot(out, n_out))
        if across < 0.0:
            out = out - 2.0 * across * n_out
        return out


ALIGN_TABLE_NODES = 513   # mu nodes of an aligned luminophore's emission table, uniformly spaced from exactly -1 to exactly 1


class Alignment(object):
    """Uniaxial alignment of a component's transition dipoles: dichroic absorption, dipole emission (extension; the
    reference has no such component).

    director : non-zero 3-vector n in the frame of the node that holds the material; normalised on construction.
    absorption_order, emission_order : the order parameters S = <P2> of the absorption and of the emission dipoles about
        the director, finite and in [-0.5, 1].  0 is the isotropic component, exactly as before; 1 the pure dipole along
        n; -0.5 dipoles in the plane perpendicular to n.

    No polarisation is tracked: both laws are the average over unpolarised light, so the polarisation memory between a
    dipole emission and the next absorption is ignored.  With mu = d . n, the absorption of unpolarised light travelling
    along d and the emission density along d have the same form,

        f(mu; S) = 1 - S P2(mu),   P2(mu) = 1.5 mu^2 - 0.5,   f >= 0,   integral of f / 2 over mu = 1,

    `Alignment.factor(mu, order)`.  The absorption rule, the same on the host and on the device (include/pvtrace_hip.h,
    PvtAlignTables, states the same):

    1. The flattener lowers each aligned component's director ONCE to the scene root's frame as a unit vector n_w: with
       the rows R0, R1, R2 of the node's rotation to the root, n_w,i = (Ri,0 nx + Ri,1 ny) + Ri,2 nz, then divided by
       sqrt((x x + y y) + z z) of the result, without FMA.
    2. At the free-path site mu_k = (dx nx + dy ny) + dz nz, without FMA, clamped to [-1, 1].
    3. f_k = 1.0 - S_k (1.5 (mu_k mu_k) - 0.5), exactly these operations in this order.
    4. A component without alignment has f_k = 1 and is not multiplied.
    5. The depth draw happens where and when an unaligned container draws, on the UNSCALED sum of alpha_k(lambda) (the
       decision of the concentration fields): S = 1 along the director does not change who draws.
    6. tau* = -ln(1 - u); the depth is tau* / sum_k alpha_k f_k.
    7. The depth is +inf when the scaled sum is exactly 0.
    8. The component is picked by the unaligned walk over alpha_k f_k, the two-component shortcut on the first partial
       sum included.
    9. Cached sums of coefficients (the device's tail function) are unscaled ones; the scaled sum is formed per step.

    The emission rule: a `Luminophore` with emission_order S_e != 0 emits about n_w, not about +z and not about the ray.
    f(mu; S_e) is tabulated on `ALIGN_TABLE_NODES` uniform mu nodes as ONE single-row `PhaseFunctionTable` and sampled
    by its rule (steps 3 and 4 there) with the director as the axis: no u1, and the two isotropic draw sites serve as u2
    and u3, so an aligned emission consumes exactly the draws an isotropic one does and the wavelength and delay draws
    follow unchanged.  S_e = 0 is the isotropic phase function, with no table.

    `absorption_order` applies to `Scatterer`, `Absorber`, `Reactor` and `Luminophore`; `emission_order != 0` to
    `Luminophore` only, and not together with an explicit `phase_function`.  Alignment and a `ConcentrationGrid` in one
    material, alignment on the scene's root, the host-buffer `trace_bundle` and the older `pvt_scene_create_*` entries
    are refused.
    """

    def __init__(self, director, absorption_order=0.0, emission_order=0.0):
        try:
            n = np.array(director, dtype=np.float64)
        except (TypeError, ValueError) as exc:
            raise ValueError(f"Alignment: director must be a 3-vector ({exc})") from None
        if n.shape != (3,) or not np.all(np.isfinite(n)):
            raise ValueError("Alignment: director must be a finite 3-vector")
        norm = math.sqrt(float((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]))
        if not norm > 0.0:
            raise ValueError("Alignment: director must not be the zero vector")
        self.director = tuple(float(v) / norm for v in n)
        self.absorption_order = self._order(absorption_order, "absorption_order")
        self.emission_order = self._order(emission_order, "emission_order")
        self._table = None

    @staticmethod
    def _order(value, what):
        try:
            s = float(value)
        except (TypeError, ValueError):
            raise ValueError(f"Alignment: {what} must be a number, got {value!r}") from None
        if not math.isfinite(s):
            raise ValueError(f"Alignment: {what} must be finite, got {value!r}")
        if not -0.5 <= s <= 1.0:
            raise ValueError(f"Alignment: {what} must lie in [-0.5, 1], got {value!r}")
        return s

    @staticmethod
    def factor(mu, order):
        """f(mu; S) = 1.0 - S (1.5 (mu mu) - 0.5), in exactly this operation order (scalars or arrays)."""
        return 1.0 - order * (1.5 * (mu * mu) - 0.5)

    @staticmethod
    def cosine(direction, axis):
        """mu = (dx nx + dy ny) + dz nz clamped to [-1, 1]: step 2 of the absorption rule."""
        mu = (float(direction[0]) * float(axis[0]) + float(direction[1]) * float(axis[1])) + float(direction[2]) * float(axis[2])
        return min(max(mu, -1.0), 1.0)

    @property
    def emission_table(self):
        """The single-row `PhaseFunctionTable` of f(mu; emission_order) on `ALIGN_TABLE_NODES` uniform mu nodes (None
        when emission_order is 0); built once per object, so components that share an `Alignment` share the table."""
        if self.emission_order == 0.0:
            return None
        if self._table is None:
            k = np.arange(ALIGN_TABLE_NODES, dtype=np.float64)
            mu = -1.0 + k * (2.0 / (ALIGN_TABLE_NODES - 1))
            mu[0], mu[-1] = -1.0, 1.0
            table = PhaseFunctionTable.__new__(PhaseFunctionTable)
            values = np.maximum(self.factor(mu, self.emission_order), 0.0)
            cdf = np.cumsum(0.5 * (values[:-1] + values[1:]) * np.diff(mu))
            cdf = np.hstack([0.0, cdf / cdf[-1]])
            cdf[-1] = 1.0
            table.angle = np.degrees(np.arccos(mu))[::-1].copy()
            table.values = values[::-1].copy()
            table.wavelength = None
            table.mu = mu
            table.cdf = cdf[None, :]
            self._table = table
        return self._table

    def emit_direction(self, u2, u3, axis=None):
        """The emitted direction for the draws u2, u3 about `axis` (default: the director): the table's steps 3 and 4."""
        table = self.emission_table
        n = np.asarray(self.director if axis is None else axis, dtype=np.float64)
        return table.turn(n, table.sample_mu(u2), u3)


def _check_alignment(alignment, emitting, phase_function, what):
    if alignment is None:
        return None
    if not isinstance(alignment, Alignment):
        raise ValueError(f"alignment: expected None or an Alignment, got {type(alignment).__name__}")
    if alignment.emission_order != 0.0:
        if not emitting:
            raise ValueError(f"{what}: emission_order != 0 applies to a Luminophore only")
        if phase_function is not None:
            raise ValueError(f"{what}: emission_order != 0 cannot be combined with an explicit phase_function")
    return alignment


def phase_direction(phase_function, ray):
    """A scattered or re-emitted direction: a `PhaseFunctionTable` draws about the ray's own direction at its
    wavelength, the built-ins (and user callables) are called with no arguments, about +z."""
    if isinstance(phase_function, PhaseFunctionTable):
        return phase_function(ray.direction, ray.wavelength)
    return phase_function()


class CoatingPattern(object):
    """Where a coating covers: a mask on a lattice in the node's own frame, the frame `Coating.region` is in.

    mask : an array of three dimensions (nx, ny, nz), each >= 1, of any dtype that is all finite; stored as uint8,
        `value != 0`.  A set cell is covered.
    lower, upper : 3-tuples in the node's frame.  On an axis with ONE cell both entries may be None: that axis is
        unbounded, every point has index 0 there -- a flat pattern on a face is written without bracketing the face's own
        plane (a face at z = +h must not sit on a lattice boundary).  On every other axis both are finite and
        lower < upper.

    Anything else raises `ValueError`.  The cell of a point is `pattern_cell`'s (rule 3 in the `Coating` docstring); a
    point outside the lattice is not covered.
    """

    def __init__(self, mask, lower, upper):
        try:
            raw = np.asarray(mask)
            if raw.dtype == object or raw.dtype.kind not in "biuf":
                raise TypeError(f"dtype {raw.dtype}")
            finite = bool(np.all(np.isfinite(raw))) if raw.dtype.kind == "f" else True
        except (TypeError, ValueError) as exc:
            raise ValueError(f"CoatingPattern: mask must be a numeric array ({exc})") from None
        if raw.ndim != 3 or min(raw.shape) < 1:
            raise ValueError(f"mask must have shape (nx, ny, nz), each axis >= 1, got {raw.shape}")
        if not finite:
            raise ValueError("mask must be finite")
        try:
            lower, upper = tuple(lower), tuple(upper)
        except TypeError:
            raise ValueError("lower and upper must be 3-tuples") from None
        if len(lower) != 3 or len(upper) != 3:
            raise ValueError("lower and upper must be 3-tuples")
        lo, hi, bounded = [], [], []
        for a in range(3):
            if lower[a] is None or upper[a] is None:
                if not (lower[a] is None and upper[a] is None):
                    raise ValueError(f"axis {a}: lower and upper must both be None or both be numbers")
                if raw.shape[a] != 1:
                    raise ValueError(f"axis {a}: only an axis with one cell may be unbounded, it has {raw.shape[a]}")
                lo.append(-math.inf); hi.append(math.inf); bounded.append(False)
                continue
            l, u = check_axis(lower[a], upper[a], f"axis {a}")
            lo.append(l); hi.append(u); bounded.append(True)
        self.mask = np.ascontiguousarray(raw != 0, dtype=np.uint8)
        self.mask.setflags(write=False)
        self.lower = tuple(lo)
        self.upper = tuple(hi)
        self.bounded = tuple(bounded)

    @classmethod
    def like(cls, grid, mask=None):
        """The lattice of a `ConcentrationGrid` (or of anything with a `lattice`); `mask` given separately, or `grid.values != 0`."""
        if mask is None:
            mask = grid.values != 0
        elif np.shape(mask) != grid.lattice.shape:
            raise ValueError(f"mask must have the grid's shape {grid.lattice.shape}, got {np.shape(mask)}")
        return cls(mask, grid.lattice.lower, grid.lattice.upper)

    @property
    def shape(self):
        return self.mask.shape

    @property
    def cell_widths(self):
        """h = (upper - lower) / n per axis; inf on an unbounded axis."""
        return tuple((self.upper[a] - self.lower[a]) / float(self.shape[a]) if self.bounded[a] else math.inf
                     for a in range(3))

    @property
    def coverage(self):
        """The share of set cells."""
        return float(np.count_nonzero(self.mask)) / float(self.mask.size)


def pattern_cell(pattern, local_point):
    """The slot (ix ny + iy) nz + iz of a point of the node's frame in `pattern`'s lattice, or None when the point is
    outside: rule 3 of the `Coating` docstring, `lattice.cell_inside` per bounded axis; an unbounded axis has index 0."""
    h = pattern.cell_widths
    cell = [0, 0, 0]
    for a in range(3):
        if pattern.bounded[a]:
            inside, f = cell_inside(float(local_point[a]), pattern.lower[a], h[a], pattern.shape[a])
            if not inside:
                return None
            cell[a] = int(f)
    return slot(pattern.shape, cell)


class Coating(object):
    """Declarative override of the optics on part of a node's surface.

    The reference expresses coatings as Python subclasses of
    `FresnelSurfaceDelegate` that inspect the hit normal / position per ray
    (e.g. pvtrace/device/lsc.py:22-86, examples/006 Coatings.ipynb cell 3);
    callbacks cannot run on the GPU, so the same behaviours are written as data:

    facet : outward face normal in the node's LOCAL frame the coating covers
        (matched like ``np.allclose``: |n_i - facet_i| <= 1e-8 + 1e-5 |facet_i|), or None: any normal (extension) --
        the normal test is skipped, so a pattern, a region or both can cover part of a sphere or of the slanted side of
        a cylinder or frustum; without pattern and region it covers the whole surface.
    pattern : None, or a `CoatingPattern`: a mask lattice in the node's frame that says where, inside facet and region,
        the coating covers (extension).
    region : optional ((xlo, xhi), (ylo, yhi), (zlo, zhi)) open intervals in the
        local frame restricting where on that face it applies (None = unbounded).
    reflectivity : probability of reflection in [0, 1], a `ReflectivityTable` R(wavelength, angle of incidence),
        or None to keep Fresnel.
    absorptivity : None (the coating absorbs nothing, exactly as before), a probability in [0, 1], or an
        `AbsorptivityTable` (= `ReflectivityTable`) A(wavelength, angle of incidence): the probability that a photon
        ARRIVING at a covered point is absorbed there (extension; the reference has no such coating).  It is per
        incident photon, like the EQE of a solar cell, not a share of the light that was not reflected.
    reflection : "specular" or "lambertian" (cosine-weighted about the outward
        facet normal, in the local frame), or a `ScatterLobe` about "normal" or "specular" (extension): a tabulated
        reflection lobe, under the rule of a scattering coating in the `ScatterLobe` docstring.
    transmission : "fresnel" (Snell refraction) or "matched" (index-matched:
        direction unchanged, e.g. a perfectly coupled solar cell), or a `ScatterLobe` about "normal", "refracted" or
        "straight" (extension): a tabulated transmission lobe, under the same rule.  Beyond the critical angle a lobe
        about "refracted" behaves as "fresnel" (R stays 1), one about "normal" or "straight" as "matched" (the
        coating's R applies): that is what lets a diffusing dot extract guided light.

    The rule of an absorbing coating, the same on the host and on the device (include/pvtrace_hip.h,
    PvtCoatingAbsorbTables, states the same):

    1. R is what the surface computes for the point without absorption: Fresnel, or the coating's scalar or table
       value; beyond the critical angle R stays 1 unless transmission is "matched".
    2. A is the coating's absorptivity at the photon's current wavelength and the angle of incidence the
       reflectivity table uses.
    3. One uniform draw u decides, the draw that decides reflection, taken when R > 0 or A > 0: u < R reflects; else
       u < R + A (one double addition) absorbs; else the photon is transmitted.
    4. Where R + A > 1 the absorbed share is 1 - R and nothing is transmitted (Fresnel R near grazing incidence).
    5. Beyond the critical angle on a "fresnel" coating R = 1: the photon is totally reflected and A never applies.  An
       absorber bonded to the surface is `reflectivity=0.0, transmission="matched"`.

    An absorbed photon ends with an `Event.DETECT` row -- a surface row at the hit point, its direction the INCOMING
    one -- which a recorder with `event="detected"` on the node that was hit counts.  A coating with
    `absorptivity=0.0` traces bit for bit as one without, and no photon draws an additional random number; a point
    with A > 0 whose R is exactly 0 takes the one draw it would not take otherwise.  Where both `reflectivity` and
    `absorptivity` are given, R + A > 1 anywhere is refused.

    Where a coating covers -- the rule, the same on the host and on the device (include/pvtrace_hip.h,
    PvtCoatingPatternTables, states the same):

    1. A coating covers a point when all three hold: its facet matches (or is None); its region contains the point; it
       has no pattern, or the point's cell is set.
    2. The point is the local point the coating match already uses: pos + t on an unrotated node, the row products
       ((R0 x + R1 y) + R2 z) + t otherwise, without FMA (what `VolumeMap` rules 1-3 state).
    3. Per bounded axis h = (upper - lower) / n and i = floor((p - lower) / h).  The point is inside when
       0 <= i <= n - 1 on every bounded axis.  The slot is (ix ny + iy) nz + iz.
    4. A point outside the lattice is not covered.  There is no clamping: a pattern may be smaller than its face.
    5. The first covering coating wins.  Several coatings with disjoint masks give a palette.
    6. The decision draws no random number.  A pattern of all ones whose lattice contains the face traces bit for bit as
       the same coating without a pattern; a pattern of all zeros traces bit for bit as the scene with that coating
       removed.  Coverage is binary: a dot pattern is rendered into the mask at the resolution it needs.
    7. Roughness keeps its rule: it applies where no coating covers, so the holes of a pattern on a rough node are rough.
    """

    REFLECTION_MODES = {"specular": 0, "lambertian": 1}
    TRANSMISSION_MODES = {"fresnel": 0, "matched": 1}

    def __init__(
        self,
        facet,
        reflectivity=None,
        absorptivity=None,
        region=None,
        reflection="specular",
        transmission="fresnel",
        pattern=None,
    ):
        self.facet = None if facet is None else tuple(float(v) for v in facet)
        if self.facet is not None and len(self.facet) != 3:
            raise ValueError("facet must be a 3-vector or None")
        if pattern is not None and not isinstance(pattern, CoatingPattern):
            raise ValueError("pattern must be a CoatingPattern or None")
        self.pattern = pattern
        if isinstance(reflectivity, ReflectivityTable):
            self.reflectivity = reflectivity
        else:
            if reflectivity is not None and not 0.0 <= float(reflectivity) <= 1.0:
                raise ValueError("reflectivity must be in [0, 1], a ReflectivityTable or None")
            self.reflectivity = None if reflectivity is None else float(reflectivity)
        if isinstance(absorptivity, ReflectivityTable):
            self.absorptivity = absorptivity
        else:
            if absorptivity is not None and not 0.0 <= float(absorptivity) <= 1.0:   # (NaN fails both comparisons)
                raise ValueError("absorptivity must be in [0, 1], an AbsorptivityTable or None")
            self.absorptivity = None if absorptivity is None else float(absorptivity)
        if self.reflectivity is not None and self.absorptivity is not None:
            over = _coating_sum_exceeds_one(self.reflectivity, self.absorptivity)
            if over is not None:
                wl, angle, r, a = over
                where = "" if wl is None else f" at {wl:g} nm, {angle:g} degrees"
                raise ValueError(f"reflectivity + absorptivity must not exceed 1: R = {r:g}, A = {a:g}{where}")
        if isinstance(reflection, ScatterLobe):
            if reflection.about not in ScatterLobe.REFLECTION_ABOUT:
                raise ValueError(
                    f"a reflection lobe must be about one of {sorted(ScatterLobe.REFLECTION_ABOUT)}, got {reflection.about!r}")
        elif reflection not in self.REFLECTION_MODES:
            raise ValueError(f"reflection must be one of {sorted(self.REFLECTION_MODES)}")
        if isinstance(transmission, ScatterLobe):
            if transmission.about not in ScatterLobe.TRANSMISSION_ABOUT:
                raise ValueError(
                    f"a transmission lobe must be about one of {sorted(ScatterLobe.TRANSMISSION_ABOUT)}, got {transmission.about!r}")
        elif transmission not in self.TRANSMISSION_MODES:
            raise ValueError(
                f"transmission must be one of {sorted(self.TRANSMISSION_MODES)}"
            )
        self.reflection = reflection
        self.transmission = transmission
        bounds = []
        for axis in range(3):
            pair = None if region is None else region[axis]
            lo, hi = (None, None) if pair is None else pair
            bounds.append(
                (-math.inf if lo is None else float(lo), math.inf if hi is None else float(hi))
            )
        self.region = tuple(bounds)

    @property
    def transmits_matched(self):
        """Beyond the critical angle the coating's R applies: "matched", or a lobe about "normal" or "straight"."""
        t = self.transmission
        return t.about != "refracted" if isinstance(t, ScatterLobe) else t == "matched"

    def covers(self, normal, position):
        """Rule 1 of "where a coating covers" in the class docstring; `position` in the node's frame."""
        for a in range(3):
            if self.facet is not None and abs(normal[a] - self.facet[a]) > 1e-8 + 1e-5 * abs(self.facet[a]):
                return False
            lo, hi = self.region[a]
            if not (lo < position[a] < hi):
                return False
        pattern = getattr(self, "pattern", None)
        if pattern is None:
            return True
        slot = pattern_cell(pattern, position)
        return slot is not None and bool(pattern.mask.reshape(-1)[slot])


class CoatedSurfaceDelegate(FresnelSurfaceDelegate):
    """Fresnel surface with an ordered list of `Coating` overrides; the first
    coating covering the hit point wins, uncovered points are plain Fresnel.
    `roughness` (GGX alpha, see `FresnelSurfaceDelegate`) applies to the
    uncovered points only: a covered point behaves as a smooth one."""

    def __init__(self, coatings=None, roughness=0.0):
        super(CoatedSurfaceDelegate, self).__init__(roughness=roughness)
        self._coatings = [] if coatings is None else list(coatings)

    @property
    def coatings(self):
        return list(self._coatings)

    def _match(self, ray, geometry):
        normal = geometry.normal(ray.position)
        for coating in self.coatings:
            if coating.covers(normal, ray.position):
                return coating
        return None

    def _rough_here(self, ray, geometry):
        return self.roughness > 0.0 and self._match(ray, geometry) is None

    def reflectivity(self, surface, ray, geometry, container, adjacent):
        coating = self._match(ray, geometry)
        if coating is None:
            return super(CoatedSurfaceDelegate, self).reflectivity(surface, ray, geometry, container, adjacent)
        fresnel = self._smooth_reflectivity(surface, ray, geometry, container, adjacent)
        if coating.reflectivity is None:
            return fresnel
        if fresnel == 1.0 and not coating.transmits_matched:
            return 1.0   # beyond the critical angle no refracted ray exists: stays totally reflected
        if isinstance(coating.reflectivity, ReflectivityTable):
            normal = _flipped_normal(geometry, ray)
            cosang = float(np.clip(np.dot(normal, ray.direction), -1.0, 1.0))
            return coating.reflectivity.at(ray.wavelength, math.degrees(math.acos(cosang)))
        return coating.reflectivity

    def absorptivity(self, surface, ray, geometry, container, adjacent):
        """A of the coating covering the hit point at the ray's wavelength and angle of incidence (0 where no coating
        covers it or the coating absorbs nothing): step 2 of the rule in the `Coating` docstring."""
        coating = self._match(ray, geometry)
        a = None if coating is None else getattr(coating, "absorptivity", None)
        if a is None:
            return 0.0
        if isinstance(a, ReflectivityTable):
            normal = _flipped_normal(geometry, ray)
            cosang = float(np.clip(np.dot(normal, ray.direction), -1.0, 1.0))
            return a.at(ray.wavelength, math.degrees(math.acos(cosang)))
        return a

    def reflected_direction(self, surface, ray, geometry, container, adjacent):
        coating = self._match(ray, geometry)
        if coating is not None and isinstance(coating.reflection, ScatterLobe):   # (rules 2-5 of a scattering coating)
            out = coating.reflection.turn(ray.direction, geometry.normal(ray.position), False, getattr(ray, "wavelength", None))
            return tuple(out.tolist())
        return super(CoatedSurfaceDelegate, self).reflected_direction(surface, ray, geometry, container, adjacent)

    def transmitted_direction(self, surface, ray, geometry, container, adjacent):
        coating = self._match(ray, geometry)
        if coating is not None and isinstance(coating.transmission, ScatterLobe):   # (rules 2-5 of a scattering coating)
            n1, n2 = self._indices(ray, container, adjacent)
            out = coating.transmission.turn(ray.direction, geometry.normal(ray.position), True, getattr(ray, "wavelength", None), n1, n2)
            return tuple(out.tolist())
        if coating is not None and coating.transmission == "matched":
            return tuple(ray.direction)
        return super(CoatedSurfaceDelegate, self).transmitted_direction(
            surface, ray, geometry, container, adjacent
        )


class BaseSurface(abc.ABC):
    """What a material's surface answers (reference material/surface.py:180-203): its delegate, and the three verbs."""

    @property
    @abc.abstractmethod
    def delegate(self):
        """An object that implements `SurfaceDelegate`."""

    @abc.abstractmethod
    def is_reflected(self, ray, geometry, container, adjacent):
        """True when the ray is reflected."""

    @abc.abstractmethod
    def reflect(self, ray, geometry, container, adjacent):
        """The reflected ray."""

    @abc.abstractmethod
    def transmit(self, ray, geometry, container, adjacent):
        """The transmitted ray."""


class Surface(BaseSurface):
    def __init__(self, delegate=None):
        super(Surface, self).__init__()
        self._delegate = FresnelSurfaceDelegate() if delegate is None else delegate

    @property
    def delegate(self):
        return self._delegate

    # The per-interaction verbs of the reference's Python tracer (surface.py:224-272), for code that steps rays itself:
    # one uniform draw from numpy's global generator decides, the delegate supplies reflectivity and directions.  (The
    # engine does not call these: it lowers the delegate to tables, `engine/compiler.py`.)
    def is_reflected(self, ray, geometry, container, adjacent):
        r = self.delegate.reflectivity(self, ray, geometry, container, adjacent)
        if not isinstance(r, (int, float)):
            raise ValueError("Reflectivity must be a number.")
        if r == 0.0:
            return False   # (no draw: keeps a seeded sequence in step with the reference's)
        return bool(np.random.uniform() < r)

    def outcome(self, ray, geometry, container, adjacent):
        """"reflect", "absorb" or "transmit": the three-way decision of a surface whose delegate may absorb (the rule in
        the `Coating` docstring).  One draw, the one `is_reflected` takes, when R > 0 or A > 0; a delegate without
        `absorptivity` has A = 0 and this is `is_reflected`, draw for draw."""
        r = self.delegate.reflectivity(self, ray, geometry, container, adjacent)
        if not isinstance(r, (int, float)):
            raise ValueError("Reflectivity must be a number.")
        absorbs = getattr(self.delegate, "absorptivity", None)
        a = 0.0 if absorbs is None else float(absorbs(self, ray, geometry, container, adjacent))
        if r == 0.0 and not a > 0.0:
            return "transmit"   # (no draw: keeps a seeded sequence in step with the reference's)
        u = np.random.uniform()
        if u < r:
            return "reflect"
        return "absorb" if a > 0.0 and u < r + a else "transmit"

    def _turned(self, ray, which, *where):
        direction = getattr(self.delegate, which)(self, ray, *where)
        if not isinstance(direction, tuple):
            raise ValueError(f"Delegate method `{which}` should return a tuple.")
        if len(direction) != 3:
            raise ValueError(f"Delegate method `{which}` should return a tuple of length 3.")
        return replace(ray, direction=direction)

    def reflect(self, ray, geometry, container, adjacent):
        return self._turned(ray, "reflected_direction", geometry, container, adjacent)

    def transmit(self, ray, geometry, container, adjacent):
        return self._turned(ray, "transmitted_direction", geometry, container, adjacent)


# ----------------------------------------------------------------------
# Volume components (reference material/component.py:33-440)

def _spectrum(value, x, hist, what):
    """A constant, an (n, 2) table or a list of callables sampled on `x` -> `Distribution` (the three spellings the
    reference's components accept for a coefficient or an emission spectrum, component.py:64-90, :327-350)."""
    if isinstance(value, np.ndarray):
        return Distribution(x=value[:, 0], y=value[:, 1], hist=hist)
    if isinstance(value, (list, tuple)):
        if x is None:
            raise ValueError(f"{what} given as callables needs `x`, the wavelengths to sample them on.")
        return Distribution.from_functions(x, value, hist=hist)
    if isinstance(value, float):
        return Distribution(x=None, y=value, hist=hist)
    raise ValueError(f"{what}: expected a number, an (n, 2) array or a list of callables, got {type(value).__name__}.")


class ConcentrationGrid(object):
    """A relative-concentration field c(cell) on a voxel lattice, for one volume component: the component's attenuation
    coefficient at a point is alpha(lambda) * c(cell of the point).

    values : finite values >= 0, shape (nx, ny, nz), each axis >= 1 (stored as float64).
    lower, upper : finite 3-vectors, lower < upper on each axis: the lattice's box.

    Anything else raises `ValueError`.  The contract, the same on the host and on the device (include/pvtrace_hip.h):

    1. Frame and cells.  The lattice lies in the frame of the node whose material holds the component (the frame of a
       `Histogram`'s x, y, z).  Cell widths h = (upper - lower) / n per axis; a point p lies in cell
       clamp(floor((p - lower) / h), 0, n - 1) per axis, so a point outside the box takes the nearest edge cell.  Only
       the interior planes lower + i h, i = 1 .. n - 1, are ever crossed.
    2. Lattices.  The components of one material that carry a field share its lattice: the same shape, `lower` and
       `upper` equal bit for bit (their values may differ); a component without a field has c = 1 everywhere.  The
       scene's root node carries no field (`UnsupportedSceneError`).
    3. Free path.  tau* = -ln(1 - u) is drawn where and when an unfielded container draws, on the unscaled sum
       sum_k alpha_k(lambda).  From the photon's position, the march crosses the cells along its direction up to the
       surface distance t0 and accumulates alpha_cell * segment, alpha_cell = sum_k alpha_k(lambda) c_k[cell] in
       component order.  In a cell entered at s_in with accumulated depth tau_in, the photon is absorbed at
       s_in + (tau* - tau_in) / alpha_cell if that lies before the cell's end; cells with alpha_cell = 0 add nothing.
       Otherwise it reaches the surface.
    4. Component.  The same draw and cumulative rule as an unfielded container, over alpha_k c_k[cell] of the cell the
       march absorbed in.

    A 1 x 1 x 1 field of value 1 has no interior planes: the march is (tau* - 0) / alpha with the same alpha, and the
    scene traces draw for draw, bit for bit, as the same scene without fields.
    """

    def __init__(self, values, lower, upper):
        try:
            vals = np.array(values, dtype=np.float64)
        except (TypeError, ValueError) as exc:
            raise ValueError(f"ConcentrationGrid: values must be a numeric array ({exc})") from None
        if vals.ndim != 3 or min(vals.shape) < 1:
            raise ValueError(f"values must have shape (nx, ny, nz), each axis >= 1, got {vals.shape}")
        if not np.all(np.isfinite(vals)):
            raise ValueError("values must be finite")
        if np.any(vals < 0.0):
            raise ValueError("values must be >= 0")
        self.lattice = Lattice(vals.shape, lower, upper, "ConcentrationGrid")
        self.values, self.lower, self.upper = vals, np.array(self.lattice.lower), np.array(self.lattice.upper)

    @property
    def shape(self):
        return self.values.shape

    @property
    def h(self):
        """Cell widths (upper - lower) / n per axis."""
        return np.array(self.lattice.h, dtype=np.float64)

    def same_lattice(self, other):
        """Same shape and bounds bit for bit (values may differ)."""
        return self.lattice.same(other.lattice)

    def cell_of(self, point):
        """(ix, iy, iz) of a point in the node's frame, clamped into the lattice."""
        return tuple(cell_clamped(float(point[a]), self.lower[a], self.h[a], 0, self.shape[a] - 1) for a in range(3))


def _march(lattice, position, direction, tau, t0, alpha_of_cell):
    """The free-path march of `ConcentrationGrid` (step 3) in the lattice's frame -> (absorbed, depth, cell): the
    device's sequence of operations (pvt_trace_kernel.h, field_march_call).  `alpha_of_cell(cell)` is alpha_cell."""
    tin = 0.0
    for cell, s, sout in walk(position, direction, t0, lattice.lower, lattice.h, lattice.shape, slabs=False):
        ac = alpha_of_cell(cell)
        if ac > 0.0:
            depth = s + fmax(tau - tin, 0.0) / ac
            if depth < sout:
                return True, depth, cell
            tin += ac * (sout - s)
    return False, math.inf, None


class Component:
    def __init__(self, name="Component"):
        self.name = name
        self.concentration = None
        self.alignment = None

    def concentration_at(self, cell):
        """Relative concentration in lattice cell `cell` (1 without a field)."""
        grid = getattr(self, "concentration", None)
        return 1.0 if grid is None else float(grid.values[cell])

    def is_radiative(self, ray):
        return False

    def nonradiative_absorb(self, ray):
        return ray


class Scatterer(Component):
    """Scattering centre with attenuation coefficient (cm^-1), constant or spectral."""

    def __init__(self, coefficient, x=None, quantum_yield=1.0, tau_rad=None, tau_nr=None, phase_function=None,
                 hist=False, name="Scatterer", concentration=None, alignment=None):
        super().__init__(name=name)
        self.alignment = _check_alignment(alignment, isinstance(self, Luminophore), phase_function, type(self).__name__)
        if concentration is not None and not isinstance(concentration, ConcentrationGrid):
            raise ValueError(f"concentration: expected None or a ConcentrationGrid, got {type(concentration).__name__}")
        self.concentration = concentration
        if coefficient is None:
            raise ValueError("A component needs an attenuation coefficient.")
        if isinstance(coefficient, (int, np.integer, np.floating)) and not isinstance(coefficient, bool):
            coefficient = float(coefficient)
        self._coefficient = coefficient
        self._abs_dist = _spectrum(coefficient, x, hist, "coefficient")
        # two lifetimes fix the yield; otherwise it is given (reference component.py:92-104)
        both = tau_rad is not None and tau_nr is not None
        qy = tau_nr / (tau_nr + tau_rad) if both else (float("nan") if quantum_yield is None else quantum_yield)
        if not np.isfinite(qy):
            raise ValueError("Give `quantum_yield`, or both `tau_rad` and `tau_nr`.")
        self.quantum_yield, self.tau_rad, self.tau_nr = qy, tau_rad, tau_nr
        self.phase_function = phase_function or isotropic

    def coefficient(self, wavelength):
        return self._abs_dist(wavelength)

    # What happens to an absorbed ray, one numpy draw per decision in the reference's order (component.py:168-196):
    def is_radiative(self, ray):
        return bool(np.random.uniform() < self.quantum_yield)

    def nonradiative_absorb(self, ray):
        """The ray as it ends: with `tau_nr` set its clock runs on by an exponentially distributed delay."""
        if self.tau_nr:
            return replace(ray, duration=ray.duration - np.log(1 - np.random.uniform()) * self.tau_nr)
        return ray

    def emit(self, ray, **kwargs):
        """Scattered: a new direction from the phase function (in the frame the ray is given in; a `PhaseFunctionTable`
        draws about the ray's direction), the scatterer as source."""
        return replace(ray, direction=phase_direction(self.phase_function, ray), source=self.name)


class Absorber(Scatterer):
    """Non-radiative absorber (quantum yield 0)."""

    def __init__(self, coefficient, x=None, tau_nr=None, name="Absorber", hist=False, concentration=None, alignment=None):
        super().__init__(coefficient, x=x, quantum_yield=0.0, tau_rad=0.0, tau_nr=tau_nr, hist=hist, name=name,
                         concentration=concentration, alignment=alignment)

    def is_radiative(self, ray):
        return False   # (and no draw, as in the reference, component.py:236-239)


class Reactor(Absorber):
    """Absorber whose absorptions are tallied as photochemical reactions."""

    def __init__(self, coefficient, x=None, name="Reactor", hist=False, concentration=None, alignment=None):
        super().__init__(coefficient, x=x, hist=hist, name=name, concentration=concentration, alignment=alignment)


class Luminophore(Scatterer):
    """Absorbs and re-emits with a new wavelength drawn from `emission`."""

    def __init__(self, coefficient, emission=None, x=None, hist=False, quantum_yield=1.0, tau_rad=None, tau_nr=None,
                 phase_function=None, name="Luminophore", concentration=None, alignment=None):
        super().__init__(coefficient, x=x, quantum_yield=quantum_yield, tau_rad=tau_rad, tau_nr=tau_nr,
                         phase_function=phase_function, hist=hist, name=name, concentration=concentration,
                         alignment=alignment)
        self._emission = emission
        if emission is None:   # the reference's default line: a Gaussian at 600 nm, 40 nm wide (component.py:330-335)
            emission = [lambda v: gaussian(v, 1.0, 600.0, 40.0)]
        elif isinstance(emission, float):
            raise ValueError("emission: expected an (n, 2) array or a list of callables.")
        self._ems_dist = _spectrum(emission, x, hist, "emission")

    def emit(self, ray, method="kT", T=300.0, **kwargs):
        """Re-emitted (reference component.py:381-440; draws in its order: phase function, wavelength, delay): a new
        direction, a wavelength from the emission spectrum above the point `method` allows -- "kT": from 3/2 kT (at `T` K)
        above the absorbed photon's energy, "redshift": from the absorbed wavelength, "full": the whole spectrum -- and,
        with `tau_rad` set, an exponentially distributed emission delay.  An aligned emitter (`Alignment` with an emission
        order) emits about its director AS GIVEN, in the frame of the node that holds the material: `ray` must be in that
        frame, as `photon_tracer` passes it (a caller holding a ray of another frame turns the director itself and calls
        `alignment.emit_direction(u2, u3, axis=...)`).  Like the reference's it raises when "kT" lands
        outside the spectrum's range; the engine clamps there (differences between the two tracers)."""
        alignment = getattr(self, "alignment", None)
        if alignment is not None and alignment.emission_order != 0.0:
            # (an aligned emitter: the table's u2, u3 about the director, which is given in the frame the ray is in)
            u2 = np.random.uniform()
            u3 = np.random.uniform()
            direction = alignment.emit_direction(u2, u3)
        else:
            direction = phase_direction(self.phase_function, ray)
        nm = ray.wavelength
        if method == "kT":
            nm = 1240.0 / (1240.0 / nm + 3 / 2 * KB_EV * T)
            start = self._ems_dist.lookup(nm)
        elif method == "redshift":
            start = self._ems_dist.lookup(nm)
        elif method == "full":
            start = 0.0
        else:
            raise ValueError(f"emit method {method!r}: use 'kT', 'redshift' or 'full'")
        wavelength = self._ems_dist.sample(np.random.uniform(start, 1.0))
        delay = -np.log(1 - np.random.uniform()) * self.tau_rad if self.tau_rad else 0.0
        return replace(ray, direction=direction, wavelength=wavelength, source=self.name, duration=ray.duration + delay)


class Material(object):
    """refractive_index : a number, or a `RefractiveIndexTable` n(wavelength); stored as given."""

    def __init__(self, refractive_index, surface=None, components=None):
        self.refractive_index = refractive_index
        self.surface = Surface() if surface is None else surface
        self.components = [] if components is None else components

    def refractive_index_at(self, wavelength):
        """The refractive index at `wavelength` (nm), a float for either form of `refractive_index`."""
        return float(index_at(self, wavelength))

    def total_attenutation_coefficient(self, wavelength):
        return float(np.sum([c.coefficient(wavelength) for c in self.components]))

    # The volume decisions of the reference's Python tracer (material.py:22-63), one numpy draw each:
    def penetration_depth(self, wavelength):
        """How far a photon of this wavelength gets before something absorbs it: exponential with the summed
        coefficient; inf for a clear medium, 0 for an opaque one."""
        alpha = self.total_attenutation_coefficient(wavelength)
        if np.isclose(alpha, 0.0):
            return float("inf")
        if not np.isfinite(alpha):
            return 0.0
        return -np.log(1 - np.random.uniform()) / alpha

    def is_absorbed(self, ray, full_distance):
        """(absorbed before `full_distance`?, the sampled depth)"""
        depth = self.penetration_depth(ray.wavelength)
        return (depth < full_distance, depth)

    def component(self, wavelength):
        """Which component took the photon: each in proportion to its coefficient at this wavelength."""
        weights = np.array([c.coefficient(wavelength) for c in self.components])
        if np.any(weights < 0.0):
            raise ValueError("Must be positive.")
        steps = np.cumsum(weights)
        ladder = np.hstack([0, steps / max(steps)])
        at = np.interp(np.random.uniform(), ladder, list(range(len(self.components) + 1)))
        return self.components[int(np.floor(at))]

    # Concentration fields (`ConcentrationGrid`): the same decisions over the cells of the components' lattice, asked
    # with the ray in the frame of the node that holds this material.  Only a container with a field takes these.
    @property
    def concentration_lattice(self):
        """The lattice the components' fields share (a `ConcentrationGrid`), None when no component has one; ValueError
        when two fields of this material differ in shape or bounds."""
        grids = [c.concentration for c in self.components if getattr(c, "concentration", None) is not None]
        if not grids:
            return None
        for g in grids[1:]:
            if not grids[0].same_lattice(g):
                raise ValueError("the concentration fields of one material must share their lattice: the same shape, "
                                 "lower and upper bit for bit")
        return grids[0]

    def cell_coefficients(self, wavelength, cell):
        """alpha_k(wavelength) c_k[cell] of every component, in component order."""
        return [c.coefficient(wavelength) * c.concentration_at(cell) for c in self.components]

    def is_absorbed_in(self, local_ray, distance):
        """(absorbed before `distance`?, the depth, the lattice cell absorbed in or None): tau* = -ln(1 - u) drawn when
        and as `penetration_depth` draws, on the unscaled sum, then the march of `ConcentrationGrid` from the ray's
        position and direction given in this material's node frame."""
        lattice = self.concentration_lattice
        alpha = self.total_attenutation_coefficient(local_ray.wavelength)
        if np.isclose(alpha, 0.0):
            return False, float("inf"), None
        if not np.isfinite(alpha):
            return 0.0 < distance, 0.0, lattice.cell_of(local_ray.position)
        tau = -np.log(1 - np.random.uniform())
        wl = local_ray.wavelength
        return _march(lattice, local_ray.position, local_ray.direction, tau, distance,
                      lambda cell: float(np.sum(self.cell_coefficients(wl, cell))))

    def component_at(self, wavelength, cell):
        """Which component took the photon in lattice cell `cell`: `component`'s draw and rule over alpha_k c_k[cell]."""
        weights = np.array(self.cell_coefficients(wavelength, cell))
        if np.any(weights < 0.0):
            raise ValueError("Must be positive.")
        steps = np.cumsum(weights)
        ladder = np.hstack([0, steps / max(steps)])
        at = np.interp(np.random.uniform(), ladder, list(range(len(self.components) + 1)))
        return self.components[int(np.floor(at))]

    # Aligned components (`Alignment`): the same decisions with every coefficient scaled by its component's factor
    # f(mu_k; S_k), asked with the ray's direction in the frame of the node that holds this material (the frame the
    # directors are in).  Only a container with an aligned component takes these.
    @property
    def has_alignment(self):
        return any(getattr(c, "alignment", None) is not None for c in self.components)

    def alignment_factors(self, direction):
        """f_k of every component for a ray travelling along `direction` (1.0 for a component without alignment)."""
        out = []
        for c in self.components:
            a = getattr(c, "alignment", None)
            out.append(1.0 if a is None else float(Alignment.factor(Alignment.cosine(direction, a.director), a.absorption_order)))
        return out

    def aligned_coefficients(self, wavelength, direction):
        """alpha_k(wavelength) f_k of every component, in component order."""
        return [c.coefficient(wavelength) * f for c, f in zip(self.components, self.alignment_factors(direction))]

    def total_attenutation_coefficient_along(self, wavelength, direction):
        total = 0.0
        for term in self.aligned_coefficients(wavelength, direction):
            total = total + float(term)
        return total

    def penetration_depth_along(self, wavelength, direction):
        """`penetration_depth` for a ray along `direction`: the draw is decided on the UNSCALED sum as there, the depth
        is tau* over the scaled sum, inf when that is exactly 0."""
        alpha = self.total_attenutation_coefficient(wavelength)
        if np.isclose(alpha, 0.0):
            return float("inf")
        if not np.isfinite(alpha):
            return 0.0
        tau = -np.log(1 - np.random.uniform())
        scaled = self.total_attenutation_coefficient_along(wavelength, direction)
        return float("inf") if scaled == 0.0 else tau / scaled

    def is_absorbed_along(self, local_ray, full_distance):
        """(absorbed before `full_distance`?, the sampled depth), the ray given in this material's node frame."""
        depth = self.penetration_depth_along(local_ray.wavelength, local_ray.direction)
        return (depth < full_distance, depth)

    def component_along(self, wavelength, direction):
        """Which component took the photon: `component`'s draw and rule over alpha_k f_k."""
        weights = np.array(self.aligned_coefficients(wavelength, direction))
        if np.any(weights < 0.0):
            raise ValueError("Must be positive.")
        steps = np.cumsum(weights)
        ladder = np.hstack([0, steps / max(steps)])
        at = np.interp(np.random.uniform(), ladder, list(range(len(self.components) + 1)))
        return self.components[int(np.floor(at))]
