"""Coating reflectivity tables on the GPU, by properties that need no referee (the GPU against the C referee on scenes
with varying tables is tests/test_gpu_table_parity.py): a table holding a constant must give, bit for bit, what the
scalar coating gives (same draws, same events); step tables decide hand-traced rays exactly as the host tracer does; a mid-cell photon beam is reflected at the
bilinear value; a table too large for LDS gives the same results wherever the library or the caller puts it; and the
reference's own Python tracer, calling a selective-mirror delegate written as the reference lets users write one, pins
the outcome fractions of a Lumogen F Red slab (tests/golden/coating_table_tracer.npz)."""
import math

import numpy as np
import pytest

from pvtrace_amd import (
    Box, CoatedSurfaceDelegate, Coating, Light, Luminophore, Material, Node, ReflectivityTable, Scene, Surface,
    rectangular_mask,
)
from pvtrace_amd.data import lumogen_f_red_305
from pvtrace_amd.engine import Recorder, _kernel, compile_scene
from pvtrace_amd.engine.emit import emit_bundle
from tests import coating_table_scene as S
from tests import scenes
from tests.util import assert_bundles_identical, load_golden

pytestmark = pytest.mark.gpu


def constant_table(value):
    return ReflectivityTable([300.0, 550.0, 1000.0], np.full((3, 3), float(value)), angle=[0.0, 45.0, 90.0])


def with_tables(scene, make=constant_table):
    """The same scene with every scalar coating replaced by `make(value)` (modes and regions kept).  Surfaces are
    replaced, not changed in place: the scalar scene stays as it was."""
    for node in scene.root.preorder():
        g = node.geometry
        if g is None or not isinstance(g.material.surface.delegate, CoatedSurfaceDelegate):
            continue
        coatings = []
        for c in g.material.surface.delegate.coatings:
            r = make(c.reflectivity) if isinstance(c.reflectivity, float) else c.reflectivity
            coatings.append(Coating(c.facet, reflectivity=r, region=c.region, reflection=c.reflection,
                                    transmission=c.transmission))
        g.material.surface = Surface(delegate=CoatedSurfaceDelegate(coatings))
    return scene


def lsc_with_cells():
    from pvtrace_amd import LSC

    lsc = LSC((5.0, 5.0, 1.0))
    lsc.add_solar_cell({"left", "right", "near", "far"})
    lsc.add_back_surface_mirror()
    lsc._make_scene()
    return lsc._scene


def coated_tiles():
    """tiles6 (37 nodes: the node-grid kernels) with a partial mirror (R = 0.3, Lambertian) on every tile's top face."""
    scene = scenes.tiles6()
    for node in scene.root.preorder():
        if node is scene.root or node.geometry is None:
            continue
        m = node.geometry.material
        m.surface = Surface(delegate=CoatedSurfaceDelegate([Coating((0, 0, 1), reflectivity=0.3, reflection="lambertian")]))
    return scene


EQUIVALENCE_SCENES = {
    "coated_slab": scenes.coated_slab,        # mirror quadrant, R = 1, with a region
    "lsc_cells": lsc_with_cells,              # solar cells (R = 0, index matched) and a back-surface mirror
    "partial_lambertian": lambda: with_partial(scenes.coated_slab()),
    "tiles": coated_tiles,
}


def with_partial(scene):
    """coated_slab with R = 0.4 Lambertian on the bottom face too: draws at every hit there."""
    slab = [n for n in scene.root.children if n.geometry is not None][0]
    coatings = slab.geometry.material.surface.delegate.coatings
    coatings.append(Coating((0, 0, -1), reflectivity=0.4, reflection="lambertian"))
    slab.geometry.material.surface = Surface(delegate=CoatedSurfaceDelegate(coatings))
    return scene


def trace_pair(build, n, mode, seed=17, emit_seed=5):
    record_every, max_events, maxsteps, emit_method = mode
    scalar = build()
    pos, dirs, wl, _ = emit_bundle(scalar, n, seed=emit_seed)
    cs, ct = compile_scene(scalar), compile_scene(with_tables(build()))
    assert cs.n_coat_tables == 0 and ct.n_coat_tables == ct.n_coatings > 0
    args = (pos, dirs, wl, seed, maxsteps, max_events, emit_method, 1, record_every)
    return _kernel.trace_bundle(ct, *args), _kernel.trace_bundle(cs, *args)


@pytest.mark.parametrize("tables", [None, "heads", "global"])
@pytest.mark.parametrize("mode", [(0, 16, 1000, 0), (1, 64, 1000, 0), (3, 48, 1000, 2)])
@pytest.mark.parametrize("name", sorted(EQUIVALENCE_SCENES))
def test_constant_table_is_bit_identical_to_the_scalar_coating(name, mode, tables, monkeypatch):
    if tables is not None:
        monkeypatch.setenv("PVT_TABLES", tables)
    n = 40000 if mode[0] == 0 else 6000
    got, want = trace_pair(EQUIVALENCE_SCENES[name], n, mode)
    assert_bundles_identical(got, want, sums_rtol=1e-12, what=(name, mode, tables))
    assert int(np.sum(want["rec_distinct"])) > 0


def test_constant_table_on_the_resident_scene_entry_and_a_device_list():
    """engine.simulate (pvt_scene_create + device emission) and pvt_trace_bundle_multi take the tables through the same
    packer."""
    from pvtrace_amd import engine

    a = engine.simulate(scenes.coated_slab(), 200000, seed=9, emit_seed=10, record_every=0)
    b = engine.simulate(with_tables(scenes.coated_slab()), 200000, seed=9, emit_seed=10, record_every=0)
    for name, rec in a.recorders.items():
        assert rec.rays == b.recorders[name].rays and rec.crossings == b.recorders[name].crossings, name
    scalar = scenes.coated_slab()
    pos, dirs, wl, _ = emit_bundle(scalar, 20000, seed=2)
    args = (pos, dirs, wl, 4, 1000, 32, 0, 1, 2)
    want = _kernel.trace_bundle(compile_scene(scalar), *args)
    got = _kernel.trace_bundle(compile_scene(with_tables(scenes.coated_slab())), *args, devices=[0, 0])
    assert_bundles_identical(got, want, sums_rtol=1e-12)


# -- hand-traced rays ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(S.STEP_CASES)))
def test_step_tables_decide_hand_traced_rays_as_on_the_host(case):
    from pvtrace_amd.algorithm import photon_tracer

    make, theta, wl, reflected = S.STEP_CASES[case]
    scene = S.step_scene(make(ReflectivityTable))
    host = photon_tracer.follow(scene, S.step_ray(theta, wl), backend="host")
    gpu = photon_tracer.follow(scene, S.step_ray(theta, wl), backend="gpu", seed=3)
    assert [e for _, e in gpu] == [e for _, e in host]
    assert [e.name for _, e in host] == (["GENERATE", "REFLECT", "EXIT"] if reflected else ["GENERATE", "TRANSMIT", "TRANSMIT", "EXIT"])
    for (rg, _), (rh, _) in zip(gpu, host):
        assert np.allclose(rg.position, rh.position, rtol=0, atol=1e-12)
        assert np.allclose(rg.direction, rh.direction, rtol=0, atol=1e-12)
        assert rg.wavelength == rh.wavelength
    # ids and every column of the event log: those of the same block whose top face has the scalar R the step gives
    ray = S.step_ray(theta, wl)
    args = (np.array([ray.position]), np.array([ray.direction]), np.array([wl]), 3, 1000, 16, 0, 1, 1)
    got = _kernel.trace_bundle(compile_scene(scene), *args)
    want = _kernel.trace_bundle(compile_scene(S.step_scene(1.0 if reflected else 0.0)), *args)
    assert_bundles_identical(got, want, sums_rtol=1e-12)


# -- the interpolation is bilinear -----------------------------------------------------------------------------------
def beam_block(table):
    world = Node(name="world", geometry=Box((10.0, 10.0, 10.0), material=Material(refractive_index=1.0)))
    block = Node(name="block", parent=world, geometry=Box((4.0, 4.0, 1.0), material=Material(
        refractive_index=1.5, surface=Surface(delegate=CoatedSurfaceDelegate([Coating((0, 0, 1), reflectivity=table)])))))
    block.recorders = [Recorder("bounced", event="reflected", facet=(0, 0, 1))]
    return Scene(world)


def beam(n, theta_deg, wl, seed=0):
    rng = np.random.default_rng(seed)
    t = math.radians(theta_deg)
    d = np.array([math.sin(t), 0.0, -math.cos(t)])
    pos = np.column_stack([rng.uniform(-1.0, 1.0, n) - 2.0 * d[0] / -d[2], rng.uniform(-1.0, 1.0, n), np.full(n, 2.5)])
    return pos, np.tile(d, (n, 1)), np.full(n, float(wl))


def test_mid_cell_reflectivity_is_bilinear():
    wls, angs = [500.0, 600.0], [0.0, 40.0]
    values = np.array([[0.1, 0.5], [0.7, 0.3]])          # (angle, wavelength)
    wl, theta = 530.0, 28.0                              # t = 0.3 along the wavelength, 0.7 along the angle
    tw, ta = 0.3, 0.7
    r0 = values[0, 0] + tw * (values[0, 1] - values[0, 0])
    r1 = values[1, 0] + tw * (values[1, 1] - values[1, 0])
    want = r0 + ta * (r1 - r0)
    n = 10 ** 6
    pos, dirs, wlv = beam(n, theta, wl)
    compiled = compile_scene(beam_block(ReflectivityTable(wls, values, angle=angs)))
    out = _kernel.trace_bundle(compiled, pos, dirs, wlv, 21, 1000, 8, 0, 1, 0)
    got = out["rec_distinct"][0] / n
    sigma = math.sqrt(want * (1 - want) / n)
    assert abs(got - want) < 5 * sigma, (got, want, sigma)
    # nearest-neighbour answers (grid nodes, or linear along one axis with the other axis rounded) are far away
    for other in (*values.ravel(), values[1, 0] + tw * (values[1, 1] - values[1, 0]), values[0, 0] + ta * (values[1, 0] - values[0, 0])):
        assert abs(got - other) > 20 * sigma, other


# -- a table larger than LDS -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("tables", [None, "heads", "global"])
def test_table_larger_than_lds_gives_the_same_result_wherever_it_lives(tables, monkeypatch):
    rng = np.random.default_rng(8)
    wl_axis = np.linspace(300.0, 1000.0, 4000)
    ang_axis = np.linspace(0.0, 90.0, 8)
    values = np.clip(0.5 + 0.4 * np.sin(wl_axis / 37.0)[None, :] * np.cos(np.radians(ang_axis))[:, None]
                     + 0.05 * rng.uniform(-1, 1, (8, 4000)), 0.0, 1.0)   # 36 008 doubles: 288 KB
    table = ReflectivityTable(wl_axis, values, angle=ang_axis)

    def build():
        scene, slab = S.build(Node, Scene, Box, Material, Surface, Light, rectangular_mask, lambda: S.PUMP_NM,
                              S.components(Luminophore, lumogen_f_red_305),
                              delegate=CoatedSurfaceDelegate([Coating((0, 0, 1), reflectivity=table)]))
        slab.recorders = [Recorder("top", event="escaping", facet=(0, 0, 1)), Recorder("lost", event="lost"),
                          Recorder("bounced", event="reflected", facet=(0, 0, 1))]
        return scene

    scene = build()
    pos, dirs, wl, _ = emit_bundle(scene, 20000, seed=4)
    compiled = compile_scene(scene)
    results = {}
    for mode in ((0, 16, 1000, 0), (2, 64, 1000, 0)):
        want = _kernel.trace_bundle(compiled, pos, dirs, wl, 6, mode[2], mode[1], mode[3], 1, mode[0])
        if tables is not None:
            monkeypatch.setenv("PVT_TABLES", tables)
        got = _kernel.trace_bundle(compiled, pos, dirs, wl, 6, mode[2], mode[1], mode[3], 1, mode[0])
        monkeypatch.delenv("PVT_TABLES", raising=False)
        assert_bundles_identical(got, want, sums_rtol=1e-12, what=(tables, mode))
        results[mode] = got
    assert results[(0, 16, 1000, 0)]["rec_distinct"][2] > 0


# -- anchored to the reference's Python tracer -----------------------------------------------------------------------
def gpu_outcome_fractions(delegate, n=10 ** 6, seed=13):
    from pvtrace_amd import engine
    from pvtrace_amd.light import ConstantWavelengthMask

    scene, slab = S.build(Node, Scene, Box, Material, Surface, Light, rectangular_mask, ConstantWavelengthMask(S.PUMP_NM),
                          S.components(Luminophore, lumogen_f_red_305), delegate=delegate)
    edges = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0))
    slab.recorders = ([Recorder("top", event="escaping", facet=(0, 0, 1)), Recorder("bounced", event="reflected", facet=(0, 0, 1)),
                       Recorder("bottom", event="escaping", facet=(0, 0, -1)), Recorder("lost", event="lost"),
                       Recorder("killed", event="killed")]
                      + [Recorder(f"edge{k}", event="escaping", facet=f) for k, f in enumerate(edges)])
    r = engine.simulate(scene, n, seed=seed, record_every=0).recorders
    counts = np.array([r["top"].rays + r["bounced"].rays, r["bottom"].rays, sum(r[f"edge{k}"].rays for k in range(4)),
                       r["lost"].rays, r["killed"].rays], dtype=float)
    return counts / n


def two_sample_sigmas(p_a, n_a, p_b, n_b):
    p = (p_a * n_a + p_b * n_b) / (n_a + n_b)
    return np.abs(p_a - p_b) / np.sqrt(np.maximum(p * (1 - p), 1e-12) * (1.0 / n_a + 1.0 / n_b))


def test_selective_mirror_against_the_references_python_tracer():
    g = load_golden("coating_table_tracer.npz")
    ref = {k: np.bincount(g[f"{k}/outcome"].astype(int), minlength=5) for k in ("mirror", "plain")}
    n_ref = {k: int(v.sum()) for k, v in ref.items()}
    table = ReflectivityTable(S.MIRROR_WAVELENGTH, S.MIRROR_VALUE, angle=S.MIRROR_ANGLE)
    n = 10 ** 6
    mirror = gpu_outcome_fractions(CoatedSurfaceDelegate([Coating((0, 0, 1), reflectivity=table)]), n)
    plain = gpu_outcome_fractions(None, n)
    assert abs(mirror.sum() - 1.0) < 1e-3 and abs(plain.sum() - 1.0) < 1e-3   # every photon ends in one class
    z_mirror = two_sample_sigmas(mirror, n, ref["mirror"] / n_ref["mirror"], n_ref["mirror"])
    assert np.all(z_mirror[:4] < 4.0), dict(zip(S.CLASSES, z_mirror))
    z_plain = two_sample_sigmas(plain, n, ref["plain"] / n_ref["plain"], n_ref["plain"])
    assert np.all(z_plain[:4] < 4.0), dict(zip(S.CLASSES, z_plain))
    # power: the slab without the mirror is far from the reference's mirror run
    z_power = two_sample_sigmas(plain, n, ref["mirror"] / n_ref["mirror"], n_ref["mirror"])
    assert z_power.max() > 10.0, dict(zip(S.CLASSES, z_power))
