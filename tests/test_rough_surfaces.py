"""Rough Fresnel interfaces (FresnelSurfaceDelegate / CoatedSurfaceDelegate `roughness`, the GGX width alpha) on the host:
the keyword's validation, the flattener (alpha = 0 lowers to exactly today's tables and passes no PvtSurfaceTables), the
host microfacet sampler held to the closed-form GGX distribution of visible normals, the host tracer's fold and the
refusal of the host-buffer entry.  No GPU needed.  The closed forms below (GGX D, Smith G1, the VNDF, and the
reflection / refraction densities of Walter et al. 2007) are written from the physics, not from the sampler."""
import math

import numpy as np
import pytest

from pvtrace_amd import Box, CoatedSurfaceDelegate, Coating, Material, Node, Ray, Scene, Surface
from pvtrace_amd.algorithm import photon_tracer
from pvtrace_amd.engine import native
from pvtrace_amd.engine.compiler import UnsupportedSceneError, compile_scene
from pvtrace_amd.material import FresnelSurfaceDelegate, NullSurfaceDelegate, ggx_visible_normal, rough_fresnel_reflectivity
from tests import laws as L

REFLECT, TRANSMIT = 1, 2
BLOCK = 10.0


# -- closed forms ---------------------------------------------------------------------------------------------------
def ggx_d(cos_m, a):
    """GGX (Trowbridge-Reitz): alpha^2 / (pi ((alpha^2 - 1) cos^2 + 1)^2), i.e. 1 / (pi alpha^2 cos^4 (1 + tan^2 /
    alpha^2)^2), for cos > 0."""
    c2 = np.clip(cos_m, 0.0, 1.0) ** 2
    return np.where(cos_m > 0.0, a * a / (math.pi * ((a * a - 1.0) * c2 + 1.0) ** 2), 0.0)


def smith_g1(cos_v, a):
    t2 = (1.0 - cos_v * cos_v) / (cos_v * cos_v)
    return 2.0 / (1.0 + math.sqrt(1.0 + a * a * t2))


def vndf(v, m, a):
    """D_v(m) = G1(v) max(0, v.m) D(m) / (v.N), N = +z, per unit solid angle of m."""
    vm = m @ v
    return smith_g1(v[2], a) * np.maximum(vm, 0.0) * ggx_d(m[..., 2], a) / v[2]


def hecht_r(c, n1, n2):
    """Unpolarised Fresnel reflectance in Hecht's sin / tan form from cos(theta_i) (vectorised; 1 beyond TIR)."""
    c = np.clip(c, 0.0, 1.0)
    s = np.sqrt(1.0 - c * c)
    st = n1 / n2 * s
    out = np.ones_like(c)
    ok = st < 1.0
    ti = np.arccos(c[ok])
    tt = np.arcsin(st[ok])
    with np.errstate(divide="ignore", invalid="ignore"):
        rs = (np.sin(ti - tt) / np.sin(ti + tt)) ** 2
        rp = (np.tan(ti - tt) / np.tan(ti + tt)) ** 2
        r = 0.5 * (rs + rp)
    r = np.where(ti == 0.0, ((n1 - n2) / (n1 + n2)) ** 2, r)
    out[ok] = r
    return out


def sphere_grid(nt=240, nphi=480, upper=True, th_edges=None, sub=24):
    """Midpoints (directions, solid angles, theta, phi) of a (theta, phi) grid over the upper (z > 0) or lower
    hemisphere: nt even steps in theta, or `sub` steps inside each bin of `th_edges` (bin edges then fall on cells)."""
    if th_edges is None:
        th_edges, sub = np.array([0.0, 0.5 * math.pi]), nt
    lo, hi = np.asarray(th_edges[:-1]), np.asarray(th_edges[1:])
    k = (np.arange(sub) + 0.5) / sub
    th = (lo[:, None] + (hi - lo)[:, None] * k[None, :]).ravel()
    dth = np.repeat((hi - lo) / sub, sub)
    ph = -math.pi + (np.arange(nphi) + 0.5) * (2.0 * math.pi / nphi)
    T, P = np.meshgrid(th, ph, indexing="ij")
    z = np.cos(T) if upper else -np.cos(T)
    dirs = np.stack([np.sin(T) * np.cos(P), np.sin(T) * np.sin(P), z], axis=-1)
    dw = np.sin(T) * dth[:, None] * (2.0 * math.pi / nphi)
    return dirs, dw, T, P


def reflect_probability(v, a, n1, n2):
    """P(REFLECT) = the quadrature of R(v.m) over the VNDF."""
    m, dw, _, _ = sphere_grid()
    return float(np.sum(vndf(v, m, a) * hecht_r(m @ v, n1, n2) * dw))


def reflected_density(v, o, a, n1, n2):
    """Density of the reflected direction o (before the fold): D_v(h) R(v.h) / (4 v.h), h = normalize(v + o)."""
    h = v + o
    h = h / np.linalg.norm(h, axis=-1, keepdims=True)
    vh = h @ v
    ok = (vh > 0.0) & (h[..., 2] > 0.0)
    return np.where(ok, vndf(v, h, a) * hecht_r(vh, n1, n2) / (4.0 * np.where(ok, vh, 1.0)), 0.0)


def transmitted_density(v, o, a, n1, n2):
    """Density of the transmitted direction o (before the fold), Walter et al. 2007: h = -(n1 v + n2 o) normalised
    (turned to +z), D_v(h) (1 - R(v.h)) n2^2 |o.h| / (n1 v.h + n2 o.h)^2."""
    h = -(n1 * v + n2 * o)
    h = h / np.linalg.norm(h, axis=-1, keepdims=True)
    h = np.where(h[..., 2:3] < 0.0, -h, h)
    vh, oh = h @ v, np.sum(o * h, axis=-1)
    ok = (vh > 0.0) & (oh < 0.0)
    den = (n1 * vh + n2 * oh) ** 2
    jac = np.where(ok, n2 * n2 * np.abs(oh) / np.where(ok, den, 1.0), 0.0)
    return np.where(ok, vndf(v, h, a) * (1.0 - hecht_r(vh, n1, n2)) * jac, 0.0)


def folded_bin_probs(density, v, a, n1, n2, upper, ct_edges, ph_edges):
    """Bin probabilities of the FOLDED directions over (cos theta, phi) bins of the hemisphere they end in: the density
    there plus the density mirrored from the other side."""
    o, dw, T, P = sphere_grid(upper=upper, th_edges=np.arccos(ct_edges[::-1]), sub=40)
    mirror = o * np.array([1.0, 1.0, -1.0])
    p = (density(v, o, a, n1, n2) + density(v, mirror, a, n1, n2)) * dw
    ct = np.abs(o[..., 2])
    i = np.clip(np.searchsorted(ct_edges, ct, side="right") - 1, 0, len(ct_edges) - 2)
    j = np.clip(np.searchsorted(ph_edges, P, side="right") - 1, 0, len(ph_edges) - 2)
    probs = np.zeros((len(ct_edges) - 1, len(ph_edges) - 1))
    np.add.at(probs, (i, j), p)
    return probs.ravel() / probs.sum(), float(p.sum())


def direction_bins(d, ct_edges, ph_edges):
    ct = np.abs(d[:, 2])
    ph = np.arctan2(d[:, 1], d[:, 0])
    i = np.clip(np.searchsorted(ct_edges, ct, side="right") - 1, 0, len(ct_edges) - 2)
    j = np.clip(np.searchsorted(ph_edges, ph, side="right") - 1, 0, len(ph_edges) - 2)
    return np.bincount(i * (len(ph_edges) - 1) + j, minlength=(len(ct_edges) - 1) * (len(ph_edges) - 1))


CT_EDGES = np.linspace(0.0, 1.0, 11)
PH_EDGES = np.linspace(-math.pi, math.pi, 13)


def rough_block_scene(alpha, index=1.5, coatings=None):
    """A 10 cm cube of `index` with a rough surface of GGX width alpha in an n = 1 world."""
    from pvtrace_amd.engine import Recorder

    world = Node(name="world", geometry=Box((100.0, 100.0, 100.0), material=Material(refractive_index=1.0)))
    delegate = (FresnelSurfaceDelegate(roughness=alpha) if coatings is None
                else CoatedSurfaceDelegate(coatings, roughness=alpha))
    block = Node(name="block", parent=world,
                 geometry=Box((BLOCK, BLOCK, BLOCK), material=Material(refractive_index=index, surface=Surface(delegate))))
    block.recorders = [Recorder("reflected", event="reflected"), Recorder("entering", event="entering")]
    return Scene(world)


def outside_ray(theta):
    d = (math.sin(theta), 0.0, -math.cos(theta))
    return (-20.0 * d[0], 0.0, BLOCK / 2 + 20.0 * math.cos(theta)), d


# -- 1. the keyword ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [-1e-9, -0.5, 1.0000001, 2.0, float("nan"), float("inf"), -float("inf")])
@pytest.mark.parametrize("cls", [FresnelSurfaceDelegate, CoatedSurfaceDelegate])
def test_roughness_outside_0_1_is_refused(cls, bad):
    with pytest.raises(ValueError, match="roughness"):
        cls(roughness=bad)


def test_roughness_defaults_to_zero_and_keeps_the_old_constructors():
    assert FresnelSurfaceDelegate().roughness == 0.0
    assert CoatedSurfaceDelegate().roughness == 0.0
    assert CoatedSurfaceDelegate([Coating((0.0, 0.0, 1.0), reflectivity=1.0)]).roughness == 0.0
    assert FresnelSurfaceDelegate(roughness=1.0).roughness == 1.0
    assert CoatedSurfaceDelegate(None, 0.25).roughness == 0.25
    assert not hasattr(NullSurfaceDelegate(), "roughness")
    with pytest.raises(TypeError):
        NullSurfaceDelegate(roughness=0.1)


# -- 2. lowering ------------------------------------------------------------------------------------------------------
def _block(delegate):
    world = Node(name="world", geometry=Box((100.0, 100.0, 100.0), material=Material(refractive_index=1.0)))
    Node(name="block", parent=world,
         geometry=Box((BLOCK, BLOCK, BLOCK), material=Material(refractive_index=1.5, surface=Surface(delegate))))
    return Scene(world)


def test_zero_roughness_compiles_to_the_tables_of_today():
    for old, new in ((FresnelSurfaceDelegate(), FresnelSurfaceDelegate(roughness=0.0)),
                     (CoatedSurfaceDelegate([Coating((0.0, 0.0, 1.0), reflectivity=0.5)]),
                      CoatedSurfaceDelegate([Coating((0.0, 0.0, 1.0), reflectivity=0.5)], roughness=0.0))):
        a, b = compile_scene(_block(old)).tables(), compile_scene(_block(new)).tables()
        assert a.keys() == b.keys()
        for k in a:
            assert np.asarray(a[k]).dtype == np.asarray(b[k]).dtype and np.array_equal(a[k], b[k]), k
        c = compile_scene(_block(new))
        assert not np.any(c.surface_roughness) and not c.has_roughness
        assert native.surface_tables_struct(c) == (None, {})


def test_rough_nodes_lower_their_alpha_and_the_struct_carries_it():
    c = compile_scene(_block(FresnelSurfaceDelegate(roughness=0.3)))
    assert c.surface_roughness.dtype == np.float64 and list(c.surface_roughness) == [0.0, 0.3]
    assert c.has_roughness
    st, keep = native.surface_tables_struct(c)
    assert st.n_nodes == 2 and [st.node_roughness[i] for i in range(2)] == [0.0, 0.3]
    assert np.array_equal(keep["node_roughness"], c.surface_roughness)
    # (everything else as for the smooth scene)
    smooth = compile_scene(_block(FresnelSurfaceDelegate())).tables()
    rough = c.tables()
    for k in smooth:
        if k != "surface_roughness":
            assert np.array_equal(smooth[k], rough[k]), k


def test_null_surfaces_lower_no_roughness():
    c = compile_scene(_block(NullSurfaceDelegate()))
    assert not np.any(c.surface_roughness)


def test_surface_tables_struct_matches_the_header_and_the_entry_is_exported():
    import ctypes as C
    import os

    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pvtrace_hip.h")).read()
    assert "int pvt_scene_create_rough(" in text and "typedef struct PvtSurfaceTables" in text
    assert "pvt_scene_create_rough" in native.ABI_SYMBOLS
    assert C.sizeof(native.PvtSurfaceTables) == 16 and native.PvtSurfaceTables.node_roughness.offset == 8


def test_host_buffer_entry_refuses_rough_scenes():
    from pvtrace_amd.engine import _kernel

    c = compile_scene(_block(FresnelSurfaceDelegate(roughness=0.2)))
    with pytest.raises(UnsupportedSceneError, match="rough"):
        _kernel._host_buffer_scene(c)
    with pytest.raises(UnsupportedSceneError, match="rough"):
        _kernel.trace_bundle(c, np.zeros((1, 3)), np.array([[1.0, 0.0, 0.0]]), np.array([555.0]), 0, 10, 4, 0, 1, 1)
    _kernel._host_buffer_scene(compile_scene(_block(FresnelSurfaceDelegate(roughness=0.0))))   # smooth: as before


# -- 3. the host sampler against the VNDF ------------------------------------------------------------------------------
@pytest.mark.parametrize("theta_v, alpha", [(0.3, 0.1), (1.2, 0.4), (0.7, 0.05), (1.45, 1.0), (0.9, 0.7)])
def test_host_sampler_follows_the_ggx_visible_normals(theta_v, alpha):
    rng = np.random.default_rng(int(1000 * theta_v + 100 * alpha))
    n = 200_000
    v = np.array([math.sin(theta_v), 0.0, math.cos(theta_v)])
    m = ggx_visible_normal((0.0, 0.0, 1.0), -v, alpha, rng.uniform(size=n), rng.uniform(size=n))
    assert np.allclose(np.linalg.norm(m, axis=1), 1.0, atol=1e-12)
    assert np.all(m @ v > 0.0)
    # bins in theta_m spread by alpha (uniform in atan(tan(theta) / alpha)), uniform in phi_m
    th_edges = np.arctan(alpha * np.tan(np.linspace(0.0, 0.5 * math.pi, 13)))
    th_edges[-1] = 0.5 * math.pi
    grid, dw, T, P = sphere_grid(nphi=480, th_edges=th_edges, sub=40)
    p = vndf(v, grid, alpha) * dw
    assert abs(p.sum() - 1.0) < 2e-3, p.sum()   # (the closed form integrates to 1)
    i = np.clip(np.searchsorted(th_edges, T, side="right") - 1, 0, 11)
    j = np.clip(np.searchsorted(PH_EDGES, P, side="right") - 1, 0, 11)
    probs = np.zeros((12, 12))
    np.add.at(probs, (i, j), p)
    tm = np.arccos(np.clip(m[:, 2], -1.0, 1.0))
    pm = np.arctan2(m[:, 1], m[:, 0])
    counts = np.bincount(np.clip(np.searchsorted(th_edges, tm, side="right") - 1, 0, 11) * 12 +
                         np.clip(np.searchsorted(PH_EDGES, pm, side="right") - 1, 0, 11), minlength=144)
    L.assert_chi2(counts, probs.ravel() / probs.sum(), ("VNDF", theta_v, alpha))


def test_host_sampler_is_frame_independent():
    """The same draws about a tilted normal give the same m up to the rotation: v . m and N . m agree."""
    rng = np.random.default_rng(3)
    n = 50_000
    N = np.array([0.3, -0.5, 0.8])
    N /= np.linalg.norm(N)
    v = np.array([0.9, 0.1, 0.2]) + 0.0
    v -= 0.0
    v /= np.linalg.norm(v)
    if v @ N < 0:
        v = -v
    a = 0.35
    m = ggx_visible_normal(-N, -v, a, rng.uniform(size=n), rng.uniform(size=n))   # normal given pointing away: turned
    assert np.all(m @ v > 0.0) and np.all(m @ N >= 0.0)
    L.assert_ks2(m @ N, ggx_visible_normal((0.0, 0.0, 1.0), -np.array([math.sqrt(1 - (v @ N) ** 2), 0.0, v @ N]), a,
                                           rng.uniform(size=n), rng.uniform(size=n))[:, 2], "cos theta_m")


def test_rough_reflectivity_is_hecht_about_the_microfacet():
    for c in (1.0, 0.8, 0.5, 0.2, 0.01):
        assert rough_fresnel_reflectivity(c, 1.0, 1.5) == pytest.approx(float(hecht_r(np.array([c]), 1.0, 1.5)[0]), rel=1e-12, abs=1e-15)
    assert rough_fresnel_reflectivity(0.5, 1.5, 1.0) == 1.0   # 60 degrees inside n = 1.5: TIR about m
    assert rough_fresnel_reflectivity(1.2, 1.0, 1.5) == pytest.approx(0.04)   # (clamped to 1)


# -- 4. the host tracer ---------------------------------------------------------------------------------------------
def test_host_follow_folds_every_reflection_back_and_every_transmission_through():
    scene = rough_block_scene(0.6)
    np.random.seed(5)
    seen = {REFLECT: 0, TRANSMIT: 0}
    for k in range(400):
        theta = math.radians(5.0 + (k % 8) * 11.0)
        start, d = outside_ray(theta)
        prev = None
        for ray, event, meta in photon_tracer.step_forward(scene, Ray(start, d, 555.0), maxsteps=12, backend="host"):
            if event.name in ("REFLECT", "TRANSMIT"):
                nrm = np.asarray(meta["normal"], float)
                before, after = float(np.dot(prev, nrm)), float(np.dot(ray.direction, nrm))
                if event.name == "REFLECT":
                    assert before * after < 0.0, (k, before, after)
                    seen[REFLECT] += 1
                else:
                    assert before * after > 0.0, (k, before, after)
                    seen[TRANSMIT] += 1
            prev = np.asarray(ray.direction, float)
    assert seen[REFLECT] > 50 and seen[TRANSMIT] > 300


def test_host_reflected_fraction_is_the_vndf_quadrature():
    alpha, theta = 0.4, math.radians(70.0)
    scene = rough_block_scene(alpha)
    np.random.seed(9)
    n, refl = 4000, 0
    start, d = outside_ray(theta)
    for _ in range(n):
        history = photon_tracer.follow(scene, Ray(start, d, 555.0), maxsteps=2, backend="host")
        refl += history[1][1].name == "REFLECT"
    v = -np.asarray(d)
    L.assert_binomial(refl, n, reflect_probability(v, alpha, 1.0, 1.5), "host P(reflect)")


def test_host_coated_points_draw_nothing():
    """A covered point behaves as a smooth one: the same numpy stream gives the same history as roughness 0."""
    coat = [Coating((0.0, 0.0, 1.0), reflectivity=0.3)]
    out = []
    for alpha in (0.0, 0.5):
        scene = rough_block_scene(alpha, coatings=coat)
        np.random.seed(17)
        start, d = outside_ray(math.radians(30.0))
        hist = photon_tracer.follow(scene, Ray(start, d, 555.0), maxsteps=1, backend="host")
        out.append([(tuple(r.direction), e.name) for r, e in hist[:2]] + [np.random.uniform()])
    assert out[0] == out[1]
