"""Scenes, rays and checks of the closed-form law tests, shared by tests/test_laws_referee.py (the CPU referee) and
tests/test_gpu_laws.py (the HIP engine).

Each case is a function `case(backend)`: it builds a scene from the project's public classes, traces rays through
`backend` and asserts that what comes out follows the closed form of tests/laws.py, computed from the scene's own
tables.  A backend says how to trace and emit and how many photons to spend: `backend.n_hist` for laws read from
per-event log rows, `backend.n_tally` for laws read from recorders and histograms.

Where the contract's rule differs from textbook physics the case asserts the contract's rule and says so.
"""
import math

import numpy as np

from pvtrace_amd import (
    Absorber, Box, CoatedSurfaceDelegate, Coating, Light, Luminophore, Material, Node, Reactor, ReflectivityTable,
    RefractiveIndexTable, Scatterer, Scene, Surface, isotropic, lambertian,
)
from pvtrace_amd.engine import Histogram, Recorder
from pvtrace_amd.light import CircularMask, ConstantWavelengthMask, CubeMask, RectangularMask, SpectrumWavelengthMask
from pvtrace_amd.material import Cone, Distribution, HenyeyGreenstein, gaussian
from tests import laws as L

GENERATE, REFLECT, TRANSMIT, ABSORB, NONRADIATIVE, SCATTER, EMIT, EXIT, REACT, KILL = range(10)
EMIT_METHOD = {"kT": 0, "redshift": 1, "full": 2}


def recorder_index(compiled, name):
    return compiled.recorder_names.index(name)


def tally(data, compiled, name):
    return int(data["rec_distinct"][recorder_index(compiled, name)])


def hist_counts(data, compiled, name):
    r = recorder_index(compiled, name)
    h = int(compiled.rec_hist_start[r])
    off, nb = int(compiled.hist_offset[h]), int(compiled.hist_na[h]) * int(compiled.hist_nb[h])
    return np.asarray(data["rec_bins"][off:off + nb])


def rows(data, k, max_events):
    """Row k of every recorded ray (record_every = 1) -> dict of columns, and the mask of rays that have that row."""
    counts = np.asarray(data["counts"])
    idx = np.arange(counts.size) * max_events + k
    have = counts > k
    out = {key: np.asarray(data[key])[idx] for key in ("kind", "position", "direction", "wavelength", "duration")}
    return out, have


# -- Fresnel -----------------------------------------------------------------------------------------------------------
BLOCK = 10.0
N_GLASS = 1.5
INDEX_TABLE = RefractiveIndexTable([400.0, 500.0, 650.0, 800.0], [1.62, 1.51, 1.47, 1.40])


def block_scene(index=N_GLASS, coatings=None):
    """A 10 cm cube of index `index` (a number or a RefractiveIndexTable) in an n = 1 world, optionally coated; a
    `reflected` and an `entering` recorder on it."""
    world = Node(name="world", geometry=Box((100.0, 100.0, 100.0), material=Material(refractive_index=1.0)))
    surface = Surface() if coatings is None else Surface(delegate=CoatedSurfaceDelegate(coatings))
    block = Node(name="block", parent=world,
                 geometry=Box((BLOCK, BLOCK, BLOCK), material=Material(refractive_index=index, surface=surface)))
    block.recorders = [Recorder("reflected", event="reflected"), Recorder("entering", event="entering")]
    return Scene(world)


def outside_ray(theta, wavelength=555.0):
    """(start, direction, wavelength) of a ray onto the centre of the top face from outside, at `theta` (radians)
    from the normal, in the xz plane."""
    d = (math.sin(theta), 0.0, -math.cos(theta))
    return (-20.0 * d[0], 0.0, BLOCK / 2 + 20.0 * math.cos(theta)), d, wavelength


def inside_ray(theta, wavelength=555.0):
    """A ray from inside the block onto the centre of its top face at `theta` from the normal."""
    d = (math.sin(theta), 0.0, math.cos(theta))
    return (-3.0 * d[0], 0.0, BLOCK / 2 - 3.0 * d[2]), d, wavelength


def reflected_from_outside(backend, scene, theta, wavelength, r_expected, what):
    """Tally mode: reflected ~ Binomial(n, R) and reflected + entering = n exactly."""
    n = backend.n_tally
    data, compiled = backend.trace_pencil(scene, *outside_ray(theta, wavelength), n, seed=11, record_every=0)
    refl, ent = tally(data, compiled, "reflected"), tally(data, compiled, "entering")
    assert refl + ent == n, (what, refl, ent, n)
    L.assert_binomial(refl, n, r_expected, what)


def first_surface_from_inside(backend, scene, theta, wavelength, r_expected, what):
    """Log rows: the first surface event of rays from inside is REFLECT with probability R."""
    n = backend.n_hist
    data, _ = backend.trace_pencil(scene, *inside_ray(theta, wavelength), n, seed=12, record_every=1, max_events=3)
    row, have = rows(data, 1, 3)
    assert have.all()
    kinds = row["kind"]
    assert np.all((kinds == REFLECT) | (kinds == TRANSMIT)), what
    L.assert_binomial(int(np.sum(kinds == REFLECT)), n, r_expected, what)


THETA_C = math.asin(1.0 / N_GLASS)
ULP = math.ulp(THETA_C)
FRESNEL_OUTSIDE = {"0deg": 0.0, "30deg": math.radians(30.0), "brewster": L.brewster(1.0, N_GLASS),
                   "80deg": math.radians(80.0), "89.9deg": math.radians(89.9)}
FRESNEL_INSIDE = {"30deg": math.radians(30.0), "critical-16ulp": THETA_C - 16 * ULP,
                  "critical+16ulp": THETA_C + 16 * ULP, "60deg": math.radians(60.0)}


def fresnel_outside(backend, key):
    """Scalar n = 1.5 from outside: reflected fraction = Hecht's R(theta) (at Brewster R = R_s / 2 = 0.074).  At 5
    sigma n_tally = 1e6 (referee) resolves R off by 1e-3 absolute at R ~ 0.04, 1e7 (GPU) by 3e-4."""
    theta = FRESNEL_OUTSIDE[key]
    reflected_from_outside(backend, block_scene(), theta, 555.0, L.fresnel_r(theta, 1.0, N_GLASS), ("fresnel out", key))


def fresnel_inside(backend, key):
    """Scalar n = 1.5 from inside: R(theta) below the critical angle; 16 ulps beyond it every ray reflects, exactly
    (16 ulps is ~1.8e-15 rad, an order above the rounding of the traced angle).  n_hist = 4e5 (referee) resolves R
    off by 2e-3 absolute at R ~ 0.06, 1e6 (GPU) by 1.2e-3."""
    theta = FRESNEL_INSIDE[key]
    first_surface_from_inside(backend, block_scene(), theta, 555.0, L.fresnel_r(theta, N_GLASS, 1.0), ("fresnel in", key))


DISPERSION_WL = {"node": 500.0, "mid-cell": 575.0, "below": 350.0, "above": 900.0}


def fresnel_dispersive(backend, key):
    """n(lambda) from a RefractiveIndexTable, at 60 degrees from outside and 35 degrees from inside: R = Hecht's R at the
    exact piecewise-linear n (clamped outside the table).  From outside dR/dn ~ 0.3 at 60 degrees: n_tally = 1e6
    (referee) resolves n off by ~6e-3, 1e7 (GPU) by 2e-3; the inside case, nearer TIR (dR/dn ~ 1.5 at n ~ 1.6), n_hist =
    4e5 resolves ~2e-3."""
    wl = DISPERSION_WL[key]
    n_exact = L.lerp_exact(wl, INDEX_TABLE.wavelength, INDEX_TABLE.values)
    scene = block_scene(INDEX_TABLE)
    theta = math.radians(60.0)
    reflected_from_outside(backend, scene, theta, wl, L.fresnel_r(theta, 1.0, n_exact), ("n(wl) out", key))
    theta = math.radians(35.0)
    first_surface_from_inside(backend, block_scene(INDEX_TABLE), theta, wl, L.fresnel_r(theta, n_exact, 1.0),
                              ("n(wl) in", key))


# -- coatings ----------------------------------------------------------------------------------------------------------
COAT_WL = [450.0, 550.0, 650.0]
COAT_ANGLE = [0.0, 30.0, 60.0]
COAT_VALUES = [[0.10, 0.50, 0.20], [0.40, 0.90, 0.30], [0.80, 0.15, 0.60]]
COAT_TABLE = ReflectivityTable(COAT_WL, COAT_VALUES, angle=COAT_ANGLE)
# (wavelength, angle of incidence in degrees) from outside
COAT_OUTSIDE = {"nodes": (550.0, 30.0), "mid-cells": (500.0, 45.0), "below-both": (400.0, 0.0),
                "above-wl": (700.0, 15.0), "above-angle": (600.0, 75.0)}


def coated_block(transmission="fresnel"):
    return block_scene(coatings=[Coating((0, 0, 1), reflectivity=COAT_TABLE, transmission=transmission)])


def coating_table_outside(backend, key):
    """A ReflectivityTable coating on the top face, from outside: reflected fraction = the exact bilinear R(lambda,
    theta) at the arriving angle, both axes clamped.  n_tally = 1e6 (referee) resolves R off by 2.5e-3 absolute at
    R ~ 0.5, 1e7 (GPU) by 8e-4."""
    wl, deg = COAT_OUTSIDE[key]
    r = L.bilinear_exact(wl, deg, COAT_WL, COAT_ANGLE, COAT_VALUES)
    reflected_from_outside(backend, coated_block(), math.radians(deg), wl, r, ("coating out", key))


def coating_table_inside(backend, key):
    """The same coating from inside the n = 1.5 block.  'arriving': at 25 degrees the table is read at 25 degrees (the
    photon's own angle), not at the 39.3 degrees it would leave at (R 0.70 against 0.82 at 600 nm).  'tir-fresnel':
    beyond the critical angle a Fresnel-transmitting coating reflects every ray.  'tir-matched': an index-matched
    coating has a transmitted ray there, so the table decides (R(600 nm, 50 deg)).  n_hist = 4e5 (referee): R off by
    3.6e-3 absolute; 1e6 (GPU): 2.3e-3."""
    wl = 600.0
    if key == "arriving":
        deg, scene = 25.0, coated_block()
        r = L.bilinear_exact(wl, deg, COAT_WL, COAT_ANGLE, COAT_VALUES)
    elif key == "tir-fresnel":
        deg, scene, r = 50.0, coated_block(), 1.0
    else:
        deg, scene = 50.0, coated_block("matched")
        r = L.bilinear_exact(wl, deg, COAT_WL, COAT_ANGLE, COAT_VALUES)
    first_surface_from_inside(backend, scene, math.radians(deg), wl, r, ("coating in", key))


SIDE_POSE = (0.6, (0.3, -1.0, 0.4))   # the block's rotation (angle, axis) in the Lambertian coating case


def lambertian_coating(backend):
    """A scalar R = 0.3 coating with Lambertian reflection on the +x face of a rotated block: the reflected fraction
    is 0.3, and the reflected directions, in the face's frame, have sin^2 theta uniform on [0, 1] and a uniform
    azimuth about the face normal.  n_hist = 4e5 (referee): R off by 3.6e-3 absolute; the KS on 1.2e5 reflections
    resolves a CDF shift of 8e-3 (a hemisphere-uniform reflection differs by 0.25); 1e6 (GPU): 5e-3."""
    world = Node(name="world", geometry=Box((100.0, 100.0, 100.0), material=Material(refractive_index=1.0)))
    coat = Coating((1, 0, 0), reflectivity=0.3, reflection="lambertian")
    block = Node(name="block", parent=world, geometry=Box((BLOCK, BLOCK, BLOCK), material=Material(
        refractive_index=N_GLASS, surface=Surface(delegate=CoatedSurfaceDelegate([coat])))))
    block.location = (1.0, -2.0, 0.5)
    block.rotate(*SIDE_POSE)
    R = L.rotation(*SIDE_POSE)
    normal = R @ np.array([1.0, 0.0, 0.0])
    centre = R @ np.array([BLOCK / 2, 0.0, 0.0]) + np.array([1.0, -2.0, 0.5])
    tangent = R @ np.array([0.0, 0.6, 0.8])
    d = -math.cos(0.7) * normal + math.sin(0.7) * tangent
    n = backend.n_hist
    data, _ = backend.trace_pencil(Scene(world), centre - 20.0 * d, d, 555.0, n, seed=13, record_every=1, max_events=3)
    row, have = rows(data, 1, 3)
    refl = row["kind"] == REFLECT
    L.assert_binomial(int(refl.sum()), n, 0.3, "lambertian coating R")
    local = L.to_local(row["direction"][refl], R)
    assert np.all(local[:, 0] > 0.0)
    L.assert_ks(1.0 - local[:, 0] ** 2, L.lambertian_sin2_cdf(), "lambertian coating sin^2")
    L.assert_ks(L.azimuth(local, axis=0), L.uniform_cdf(-math.pi, math.pi), "lambertian coating azimuth")


# -- Beer-Lambert ------------------------------------------------------------------------------------------------------
SPEC_X = [400.0, 500.0, 600.0, 700.0]
ABS_Y = [0.2, 1.0, 0.5, 0.1]
REACT_Y = [0.6, 0.3, 0.9, 0.4]
ZBINS = 40


def slab_scene(absorber, reactor, length):
    """An n = 1 slab (1 x 1 x length) in an n = 1 world -- no Fresnel anywhere -- holding one Absorber and one Reactor;
    `exit`, `lost` and `reacted` recorders (the last two with a depth histogram) and `killed`."""
    world = Node(name="world", geometry=Box((10.0, 10.0, 3.0 * length), material=Material(refractive_index=1.0)))
    world.recorders = [Recorder("exit", event="exit")]
    slab = Node(name="slab", parent=world, geometry=Box((1.0, 1.0, length), material=Material(
        refractive_index=1.0, components=[absorber, reactor])))
    slab.recorders = [Recorder(name, event=name, histograms=[Histogram("z", -length / 2, length / 2, ZBINS)])
                      for name in ("lost", "reacted")] + [Recorder("killed", event="killed")]
    return Scene(world)


def beer_lambert_check(backend, scene, length, alphas, wl, what):
    n = backend.n_tally
    start = (0.0, 0.0, length / 2 + 0.25 * length)
    data, compiled = backend.trace_pencil(scene, start, (0.0, 0.0, -1.0), wl, n, seed=14, record_every=0)
    counts = [tally(data, compiled, k) for k in ("exit", "lost", "reacted")]
    assert sum(counts) + tally(data, compiled, "killed") == n, (what, counts)
    probs = L.absorption_outcomes(alphas, length)
    L.assert_multinomial(counts, probs, what)
    alpha = sum(alphas)
    if alpha > L.ALPHA_ZERO and probs[0] < 1.0:
        F = L.truncated_exponential_cdf(alpha, length)
        edges = np.linspace(-length / 2, length / 2, ZBINS + 1)
        # depth below the top face d = L/2 - z: bin [z_k, z_k+1) holds depths (L/2 - z_k+1, L/2 - z_k]
        p = F(length / 2 - edges[:-1]) - F(length / 2 - edges[1:])
        for name, k in (("lost", 1), ("reacted", 2)):
            h = hist_counts(data, compiled, name)
            assert h.sum() == counts[k], (what, name)
            if counts[k] > 200:
                L.assert_chi2(h, p / p.sum(), (what, name, "depth"))
    return counts


BEER_WL = {"node": 500.0, "mid-cell": 550.0, "below": 350.0, "above": 800.0, "off-grid": 432.1}


def beer_lambert_spectra(backend, key, hist=False):
    """Beer-Lambert at a wavelength of the absorber's and reactor's tables (interpolated, or with hist=True the step
    rule): exit / lost / reacted are multinomial with exp(-alpha L) and the shares alpha_i / alpha, and the depth
    histograms of lost and reacted are the truncated exponential.  n_tally = 1e6 (referee) resolves alpha_i off by
    ~0.5 % (alpha L ~ 1.2), the histograms (~3e5 each) a ~2 % change of decay length; 1e7 (GPU) ~0.15 % and ~0.6 %."""
    wl = BEER_WL[key]
    look = L.step_exact if hist else L.lerp_exact
    alphas = [look(wl, SPEC_X, ABS_Y), look(wl, SPEC_X, REACT_Y)]
    x = np.array(SPEC_X)
    scene = slab_scene(Absorber(np.column_stack((x, ABS_Y)), hist=hist, name="dye"),
                       Reactor(np.column_stack((x, REACT_Y)), hist=hist, name="reactor"), 1.0)
    beer_lambert_check(backend, scene, 1.0, alphas, wl, ("beer-lambert", key, "hist" if hist else "linear"))


BEER_CONST = {"alpha-above-zero": (0.7e-8, 0.5e-8, 1e8), "alpha-below-zero": (0.5e-8, 0.3e-8, 1e8),
              "alpha-L-20": (12.0, 8.0, 1.0)}


def beer_lambert_limits(backend, key):
    """The clear-medium threshold ALPHA_ZERO = 1e-8 of the contract and deep attenuation.  alpha = 1.2e-8 through a
    1e8 cm slab (alpha L = 1.2) follows Beer-Lambert; alpha = 0.8e-8 draws no depth at all, so every photon escapes
    (exactly; Beer-Lambert would absorb 55 %); alpha L = 20: P(escape) = 2e-9, so no escapes at these n (1e6 referee,
    1e7 GPU; a single escape fails)."""
    a, b, length = BEER_CONST[key]
    scene = slab_scene(Absorber(a, name="dye"), Reactor(b, name="reactor"), length)
    counts = beer_lambert_check(backend, scene, length, [a, b], 555.0, ("beer-lambert", key))
    if key == "alpha-L-20":
        assert counts[0] == 0


# -- phase functions ---------------------------------------------------------------------------------------------------
def medium_scene(component):
    """A 1000 cm n = 1 cube of `component` in a larger n = 1 world: a photon started at its centre is absorbed long
    before any surface."""
    world = Node(name="world", geometry=Box((1e4, 1e4, 1e4), material=Material(refractive_index=1.0)))
    Node(name="medium", parent=world, geometry=Box((1e3, 1e3, 1e3), material=Material(
        refractive_index=1.0, components=[component])))
    return Scene(world)


PHASES = {"isotropic": isotropic, "hg+0.9": HenyeyGreenstein(0.9), "hg+0.3": HenyeyGreenstein(0.3),
          "hg-0.6": HenyeyGreenstein(-0.6), "cone-0.6": Cone(0.6), "lambertian": lambertian}


def phase_function(backend, key):
    """The first SCATTER direction of a qy = 1 Scatterer, photons travelling along +x.  The contract draws phase
    directions in the WORLD frame about +z, not about the incident ray (the reference's rule; textbook scattering
    would be about +x here), so the laws are read off d_z: HG's mu-CDF and mean g, isotropic mu uniform, the cone's
    sin theta = sqrt(U) sin theta_max (not uniform in solid angle), Lambertian sin^2 theta uniform; every azimuth
    uniform.  At 5 sigma n_hist = 4e5 (referee) resolves a mean cosine off by 2e-3 at g = 0.9 (g off by 0.2 %), 4e-3
    at g = 0.3 (1.3 %); 1e6 (GPU) by 1.3e-3 and 2.5e-3 (g scaled by 0.98 is caught at every g on the GPU)."""
    phase = PHASES[key]
    n = backend.n_hist
    data, _ = backend.trace_pencil(medium_scene(Scatterer(1.0, quantum_yield=1.0, phase_function=phase)),
                                   (0.0, 0.0, 0.0), (1.0, 0.0, 0.0), 555.0, n, seed=15, record_every=1, max_events=3)
    row, have = rows(data, 2, 3)
    assert have.all() and np.all(row["kind"] == SCATTER), key
    d = row["direction"]
    mu = d[:, 2]
    L.assert_ks(L.azimuth(d), L.uniform_cdf(-math.pi, math.pi), (key, "azimuth"))
    if key == "isotropic":
        L.assert_ks(mu, L.isotropic_mu_cdf(), key)
        L.assert_mean(mu, 0.0, key)
    elif key.startswith("hg"):
        g = phase.g
        L.assert_ks(mu, L.hg_mu_cdf(g), key)
        L.assert_mean(mu, g, key)
    elif key.startswith("cone"):
        tm = phase.theta_max
        assert np.all(mu >= 0.0)
        L.assert_ks(np.sqrt(np.maximum(1.0 - mu * mu, 0.0)), L.cone_sin_cdf(tm), key)
        L.assert_mean(mu, 2.0 * (1.0 - math.cos(tm) ** 3) / (3.0 * math.sin(tm) ** 2), key)
    else:
        assert np.all(mu >= 0.0)
        L.assert_ks(1.0 - mu * mu, L.lambertian_sin2_cdf(), key)
        L.assert_mean(mu, 2.0 / 3.0, key)


# -- re-emission -------------------------------------------------------------------------------------------------------
EMS_X = np.arange(400.0, 801.0, 5.0)
EMS_Y = gaussian(EMS_X, 1.0, 600.0, 40.0)
HIST_X = np.arange(500.0, 721.0, 20.0)
HIST_Y = np.array([0.2, 1.0, 3.0, 5.0, 4.0, 6.0, 2.5, 1.5, 0.7, 0.3, 0.1, 0.05])
TAU_RAD, TAU_NR = 4e-9, 12e-9
LAMBDA_ABS = 560.0


def luminophore(hist=False):
    x, y = (HIST_X, HIST_Y) if hist else (EMS_X, EMS_Y)
    return Luminophore(5.0, emission=np.column_stack((x, y)), hist=hist, tau_rad=TAU_RAD, tau_nr=TAU_NR, name="dye")


def trapezoid_cdf(x, y):
    c = np.concatenate(([0.0], np.cumsum((y[1:] + y[:-1]) / 2.0 * np.diff(x))))
    return c / c[-1]


REEMISSION = {"full": ("full", False), "redshift": ("redshift", False), "kT": ("kT", False),
              "hist-full": ("full", True), "hist-redshift": ("redshift", True)}


def reemission(backend, key):
    """Pencil at 560 nm into a strongly absorbing Luminophore (tau_rad 4 ns, tau_nr 12 ns, so qy = 0.75).  The first
    ABSORB is followed by EMIT with probability qy; the EMIT wavelength follows the compiled emission CDF -- the whole
    spectrum ('full'), from 560 nm up ('redshift'), from 1240 / (1240 / 560 + 1.5 k_B 300 K) = 550.2 nm up ('kT'),
    or the hist=True step rule -- by chi-square; EMIT - ABSORB duration ~ Exp(tau_rad) and NONRADIATIVE - ABSORB
    ~ Exp(tau_nr) by KS.  The compiled CDF is first checked against a trapezoid integral of the spectrum (uniform
    x steps, so the spacing cancels).  n_hist = 4e5 (referee; 3e5 emissions): the kT start resolved to well under
    1 nm (1.0 instead of 1.5 k_B T moves it 3 nm), tau_rad to ~1 %, qy to 3.4e-3 absolute; 1e6 (GPU) ~1.6x finer."""
    method, hist = REEMISSION[key]
    n = backend.n_hist
    scene = medium_scene(luminophore(hist))
    data, compiled = backend.trace_pencil(scene, (0.0, 0.0, 0.0), (1.0, 0.0, 0.0), LAMBDA_ABS, n, seed=16,
                                          record_every=1, max_events=3, emit_method=EMIT_METHOD[method])
    absorb, _ = rows(data, 1, 3)
    after, have = rows(data, 2, 3)
    assert have.all() and np.all(absorb["kind"] == ABSORB)
    emitted = after["kind"] == EMIT
    assert np.all(emitted | (after["kind"] == NONRADIATIVE))
    L.assert_binomial(int(emitted.sum()), n, TAU_NR / (TAU_NR + TAU_RAD), (key, "qy"))
    delay = after["duration"] - absorb["duration"]
    L.assert_ks(delay[emitted], L.exponential_cdf(TAU_RAD), (key, "tau_rad"))
    L.assert_ks(delay[~emitted], L.exponential_cdf(TAU_NR), (key, "tau_nr"))

    x, cdf = np.asarray(compiled.ems_x), np.asarray(compiled.ems_cdf)
    wl = after["wavelength"][emitted]
    start = {"full": None, "redshift": LAMBDA_ABS, "kT": L.kt_start(LAMBDA_ABS)}[method]
    if hist:
        assert np.allclose(cdf, np.cumsum(HIST_Y) / HIST_Y.sum(), rtol=0, atol=1e-15)
        probs = L.hist_emission_probabilities(x, cdf, start)
        k = np.searchsorted(x, wl)
        assert np.all(x[np.minimum(k, x.size - 1)] == wl), (key, "hist wavelengths are table nodes")
        L.assert_chi2(np.bincount(k, minlength=x.size), probs, (key, "wavelength"))
    else:
        assert np.allclose(cdf, trapezoid_cdf(EMS_X, EMS_Y), rtol=0, atol=1e-14)
        if start is not None:
            assert wl.min() >= start - 1e-9, (key, wl.min(), start)
        edges = np.arange(402.5, 800.0, 5.0)
        counts = np.bincount(np.searchsorted(edges, wl, side="right"), minlength=edges.size + 1)
        L.assert_chi2(counts, L.bin_probabilities(L.emission_cdf(x, cdf, start), edges), (key, "wavelength"))


# -- device emission ---------------------------------------------------------------------------------------------------
LIGHT_SPEC = Distribution(EMS_X, EMS_Y)
LIGHT_SPEC_HIST = Distribution(HIST_X, HIST_Y, hist=True)
# name: (wavelength, position, direction, location, (angle, axis))
LIGHTS = {
    "rect-cone": (ConstantWavelengthMask(500.0), RectangularMask(1.5, 0.7), Cone(0.5), (1.0, 2.0, 3.0),
                  (0.7, (1.0, 1.0, 0.0))),
    "disc-lambertian": (SpectrumWavelengthMask(LIGHT_SPEC), CircularMask(2.0), lambertian, (-2.0, 0.5, 1.0),
                        (2.1, (0.2, -1.0, 0.5))),
    "cube-isotropic": (SpectrumWavelengthMask(LIGHT_SPEC_HIST), CubeMask(1.0, 2.0, 0.5), isotropic, (0.0, -3.0, 0.0),
                       (1.0, (0.0, 0.0, 1.0))),
    "point-hg": (None, None, HenyeyGreenstein(0.7), (0.5, 0.5, -1.0), (-0.9, (1.0, 0.0, 0.0))),
}


def lights_scene():
    world = Node(name="world", geometry=Box((100.0, 100.0, 100.0), material=Material(refractive_index=1.0)))
    for name, (wl, pos, dirn, loc, (angle, axis)) in LIGHTS.items():
        node = Node(name=name, parent=world, light=Light(wavelength=wl, position=pos, direction=dirn, name=name))
        node.location = loc
        node.rotate(angle, axis)
    return Scene(world)


def emitted_light_laws(pos, dirs, wl, name, what):
    """Samples of one light, in world coordinates, against its mask / direction / wavelength laws in the light's
    frame (the pose restated by Rodrigues' formula, not read from the node)."""
    wmask, pmask, dmask, loc, (angle, axis) = LIGHTS[name]
    R = L.rotation(angle, axis)
    lp, ld = L.to_local(pos, R, loc), L.to_local(dirs, R)
    assert np.allclose(np.linalg.norm(ld, axis=1), 1.0, atol=1e-12), what
    if isinstance(pmask, CubeMask):
        for a, half in enumerate((pmask.x, pmask.y, pmask.z)):
            L.assert_ks(lp[:, a], L.uniform_cdf(-half, half), (what, "cube", a))
    else:
        assert np.all(np.abs(lp[:, 2]) < 1e-9), (what, "mask in the light's plane", np.abs(lp[:, 2]).max())
        if isinstance(pmask, RectangularMask):
            L.assert_ks(lp[:, 0], L.uniform_cdf(-pmask.x, pmask.x), (what, "rect x"))
            L.assert_ks(lp[:, 1], L.uniform_cdf(-pmask.y, pmask.y), (what, "rect y"))
        elif isinstance(pmask, CircularMask):
            r2 = (lp[:, 0] ** 2 + lp[:, 1] ** 2) / pmask.radius ** 2
            L.assert_ks(r2, L.uniform_cdf(0.0, 1.0), (what, "disc r^2"))
            L.assert_ks(L.azimuth(lp), L.uniform_cdf(-math.pi, math.pi), (what, "disc azimuth"))
        else:
            assert np.all(np.abs(lp) < 1e-9), (what, "point")
    mu = ld[:, 2]
    L.assert_ks(L.azimuth(ld), L.uniform_cdf(-math.pi, math.pi), (what, "direction azimuth"))
    if isinstance(dmask, Cone):
        assert np.all(mu > 0.0)
        L.assert_ks(np.sqrt(np.maximum(1.0 - mu * mu, 0.0)), L.cone_sin_cdf(dmask.theta_max), (what, "cone"))
    elif dmask is lambertian:
        assert np.all(mu >= -1e-12)
        L.assert_ks(1.0 - mu * mu, L.lambertian_sin2_cdf(), (what, "lambertian"))
    elif dmask is isotropic:
        L.assert_ks(mu, L.isotropic_mu_cdf(), (what, "isotropic"))
    else:
        L.assert_ks(mu, L.hg_mu_cdf(dmask.g), (what, "hg"))
    if wmask is None:
        assert np.all(wl == 555.0)
    elif isinstance(wmask, ConstantWavelengthMask):
        assert np.all(wl == wmask.nanometers)
    elif wmask.distribution.hist:
        dist = wmask.distribution
        k = np.searchsorted(dist._x, wl)
        assert np.all(dist._x[np.minimum(k, dist._x.size - 1)] == wl), what
        L.assert_chi2(np.bincount(k, minlength=dist._x.size), L.hist_emission_probabilities(dist._x, dist._cdf),
                      (what, "spectrum hist"))
    else:
        dist = wmask.distribution
        assert np.allclose(dist._cdf, trapezoid_cdf(dist._x, dist._y), rtol=0, atol=1e-14)
        edges = np.arange(402.5, 800.0, 5.0)
        counts = np.bincount(np.searchsorted(edges, wl, side="right"), minlength=edges.size + 1)
        L.assert_chi2(counts, L.bin_probabilities(L.piecewise_cdf(dist._x, dist._cdf), edges), (what, "spectrum"))
    return lp, ld


def device_emission(backend, name):
    """Per-ray-stream emission (the referee's `emit`, the GPU's emission kernel) of four posed lights, rays
    round-robin: each light's samples against its mask, direction and wavelength laws after undoing the pose, and by
    two-sample KS against the host `emit_bundle` of the same scene (itself bit-identical to the reference's emitter),
    on the local x, y (r^2 for the disc), polar cosine and wavelength.  n_hist / 4 per light: 1e5 on the referee
    resolves a CDF shift of 8.5e-3 (one-sample) and 1.2e-2 (two-sample) -- a disc drawn as r = R U is off by 0.25 --,
    2.5e5 on the GPU 5.4e-3 and 7.6e-3."""
    scene = lights_scene()
    n = backend.n_hist
    k = list(LIGHTS).index(name)
    pos, dirs, wl = backend.emit(scene, n, emit_seed=17)
    sel = slice(k, n, len(LIGHTS))
    lp, ld = emitted_light_laws(pos[sel], dirs[sel], wl[sel], name, ("device emission", name))
    from pvtrace_amd.engine.emit import emit_bundle

    hpos, hdirs, hwl, _ = emit_bundle(scene, n, seed=18)
    wmask, pmask, dmask, loc, (angle, axis) = LIGHTS[name]
    R = L.rotation(angle, axis)
    hp, hd = L.to_local(hpos[sel], R, loc), L.to_local(hdirs[sel], R)
    what = ("device vs host emitter", name)
    if isinstance(pmask, CircularMask):
        L.assert_ks2(lp[:, 0] ** 2 + lp[:, 1] ** 2, hp[:, 0] ** 2 + hp[:, 1] ** 2, what)
    elif pmask is not None:
        L.assert_ks2(lp[:, 0], hp[:, 0], what)
        L.assert_ks2(lp[:, 1], hp[:, 1], what)
    L.assert_ks2(ld[:, 2], hd[:, 2], what)
    if isinstance(wmask, SpectrumWavelengthMask):
        L.assert_ks2(wl[sel], hwl[sel], what)


# -- recorder identities -----------------------------------------------------------------------------------------------
def recorder_scene():
    """A luminophore slab (with a reactor and a background absorber) under a lamp; every recorder three times: no
    source filter, `lights`, `components`.  Each event here happens at most once per photon (a convex slab alone in
    the world: a photon enters, reflects off the outside, escapes, ends once), so the filters partition every tally."""
    x = np.arange(400.0, 801.0, 5.0)
    world = Node(name="world", geometry=Box((50.0, 50.0, 50.0), material=Material(refractive_index=1.0)))
    slab = Node(name="slab", parent=world, geometry=Box((5.0, 5.0, 1.0), material=Material(refractive_index=1.5, components=[
        Luminophore(np.column_stack((x, 3.0 * gaussian(x, 1.0, 520.0, 40.0))),
                    emission=np.column_stack((x, gaussian(x, 1.0, 610.0, 35.0))), quantum_yield=0.9, name="dye"),
        Reactor(0.05, name="reactor"), Absorber(0.05, name="host")])))
    hist = lambda: [Histogram("wavelength", 400.0, 800.0, 40), Histogram("z", -0.5, 0.5, 10)]
    specs = [("entering", None), ("reflected", None), ("escaping", None), ("escaping", (0, 0, 1)),
             ("escaping", (1, 0, 0)), ("lost", None), ("reacted", None), ("killed", None)]
    recs = []
    for i, (event, facet) in enumerate(specs):
        for src in (None, "lights", "components"):
            recs.append(Recorder(f"{event}{i}:{src}", event=event, facet=facet, histograms=hist(), source=src))
    slab.recorders = recs
    world.recorders = [Recorder(f"exit:{src}", event="exit", histograms=[Histogram("wavelength", 400.0, 800.0, 40)],
                                source=src) for src in (None, "lights", "components")]
    world.recorders += [Recorder(f"killed-world:{src}", event="killed", source=src) for src in (None, "lights", "components")]
    lamp = Node(name="lamp", parent=world, light=Light(wavelength=ConstantWavelengthMask(520.0),
                                                         position=RectangularMask(2.0, 2.0), name="lamp"))
    lamp.location = (0.0, 0.0, 3.0)
    lamp.rotate(math.pi, (1.0, 0.0, 0.0))
    return Scene(world)


def recorder_identities(backend):
    """For every recorder, histogram slot and crossing count: `lights` + `components` = unfiltered, exactly (moment
    sums to 1e-12 relative); every photon ends in exactly one terminal recorder: exit + lost + reacted + killed = n.
    Tally mode, maxsteps 12 so that some photons are killed; n_tally photons (1e6 referee, 1e7 GPU): exact, so any
    photon counted twice or not at all fails."""
    scene = recorder_scene()
    n = backend.n_tally
    data, compiled = backend.trace_emitted(scene, n, seed=20, emit_seed=19, maxsteps=12, emit_method=0)
    names = compiled.recorder_names
    bases = sorted({nm.rsplit(":", 1)[0] for nm in names})
    for base in bases:
        a, b, c = (recorder_index(compiled, f"{base}:{s}") for s in ("None", "lights", "components"))
        for key in ("rec_distinct", "rec_crossings"):
            assert data[key][a] == data[key][b] + data[key][c], (base, key)
        assert np.allclose(data["rec_sums"][a], data["rec_sums"][b] + data["rec_sums"][c], rtol=1e-12, atol=0), base
        for h in range(int(compiled.rec_hist_n[a])):
            ha, hb, hc = (int(compiled.rec_hist_start[r]) + h for r in (a, b, c))
            size = int(compiled.hist_na[ha]) * int(compiled.hist_nb[ha])
            seg = lambda hh: np.asarray(data["rec_bins"][int(compiled.hist_offset[hh]):int(compiled.hist_offset[hh]) + size])
            assert np.array_equal(seg(ha), seg(hb) + seg(hc)), (base, h)
    t = lambda nm: int(data["rec_distinct"][recorder_index(compiled, nm)])
    terminal = t("exit:None") + t("lost5:None") + t("reacted6:None") + t("killed7:None") + t("killed-world:None")
    assert terminal == n, (terminal, n)
    assert t("exit:components") > 0 and t("lost5:components") > 0 and t("reacted6:lights") > 0
    assert t("killed7:None") + t("killed-world:None") > 0
