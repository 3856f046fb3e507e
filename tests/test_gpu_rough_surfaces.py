"""Rough Fresnel interfaces (GGX width alpha, `FresnelSurfaceDelegate(roughness=...)`) on the GPU.  The CPU referee
does not know roughness, so the engine is held to closed-form laws (the VNDF quadrature of R, the microfacet reflection
density, Walter et al.'s refraction Jacobian; tests/test_rough_surfaces.py writes them), to the host Python tracer in
distribution, and to itself: alpha = 0 is today's engine bit for bit, a ray's history does not depend on the launch, the
mode or the kernel variant that traces it."""
import math

import numpy as np
import pytest
import torch

from pvtrace_amd import Box, CoatedSurfaceDelegate, Coating, Material, Node, Ray, Scene, Surface
from pvtrace_amd.algorithm import photon_tracer
from pvtrace_amd.engine import Session, compile_scene, native
from pvtrace_amd.engine.emit import emit_bundle
from pvtrace_amd.material import FresnelSurfaceDelegate
from tests import laws as L
from tests import scenes
from tests.broken_tables import BAD_ROUGHNESS, surface_tables
from tests.law_cases import INDEX_TABLE, rows
from tests.test_gpu_laws import Gpu
from tests.test_rough_surfaces import (
    CT_EDGES, PH_EDGES, direction_bins, folded_bin_probs, outside_ray, reflect_probability, reflected_density,
    rough_block_scene, transmitted_density,
)

pytestmark = pytest.mark.gpu

B = Gpu()
REFLECT, TRANSMIT = 1, 2
HIST_KEYS = ("counts", "kind", "position", "direction", "wavelength", "duration")
TALLY_KEYS = ("rec_distinct", "rec_crossings", "rec_bins")


def inside_ray(theta):
    d = (math.sin(theta), 0.0, math.cos(theta))
    return (-3.0 * d[0], 0.0, 5.0 - 3.0 * d[2]), d


def first_surface_event(scene, start, d, wavelength=555.0, n=None, seed=11):
    n = B.n_hist if n is None else n
    data, _ = B.trace_pencil(scene, start, d, wavelength, n, seed=seed, record_every=1, max_events=3)
    row, have = rows(data, 1, 3)
    assert have.all()
    assert np.all((row["kind"] == REFLECT) | (row["kind"] == TRANSMIT))
    return row["kind"], row["direction"]


# -- 1. alpha = 0 changes nothing -------------------------------------------------------------------------------------
def _smooth_pair(build):
    return build(FresnelSurfaceDelegate()), build(FresnelSurfaceDelegate(roughness=0.0))


def _block(delegate):
    world = Node(name="world", geometry=Box((100.0, 100.0, 100.0), material=Material(refractive_index=1.0)))
    Node(name="block", parent=world,
         geometry=Box((10.0, 10.0, 10.0), material=Material(refractive_index=1.5, surface=Surface(delegate))))
    return Scene(world)


def test_zero_roughness_traces_exactly_as_today():
    old, new = _smooth_pair(_block)
    for theta in (0.3, 1.1):
        start, d = outside_ray(theta)
        a, _ = B.trace_pencil(old, start, d, 555.0, 100_000, seed=5, record_every=1, max_events=24)
        b, _ = B.trace_pencil(new, start, d, 555.0, 100_000, seed=5, record_every=1, max_events=24)
        for k in HIST_KEYS:
            assert np.array_equal(a[k], b[k]), k
    old, new = with_roughness(scenes.lsc_equivalent(), None), with_roughness(scenes.lsc_equivalent(), 0.0)
    assert not compile_scene(new).has_roughness
    pos, dirs, wl, _ = emit_bundle(old, 200_000, seed=3)
    out = []
    for scene in (old, new):
        with Session(scene, emission="host") as s:
            r = s.collect(s.submit(len(wl), 7, host_rays=(pos, dirs, wl, ["r"] * len(wl)), record_every=0))
            out.append({k: np.asarray(r.data[k]).copy() for k in TALLY_KEYS})
    for k in TALLY_KEYS:
        assert np.array_equal(out[0][k], out[1][k]), k


# -- 2. reflection law --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [0.1, 0.4])
def test_reflection_follows_the_microfacet_law(alpha):
    theta = math.radians(55.0)
    start, d = outside_ray(theta)
    kind, out = first_surface_event(rough_block_scene(alpha), start, d)
    v = -np.asarray(d)
    L.assert_binomial(int(np.sum(kind == REFLECT)), kind.size, reflect_probability(v, alpha, 1.0, 1.5),
                      ("P(reflect)", alpha))
    refl = out[kind == REFLECT]
    assert np.all(refl[:, 2] > 0.0)   # (folded: every reflection leaves on the incoming side)
    probs, _ = folded_bin_probs(reflected_density, v, alpha, 1.0, 1.5, True, CT_EDGES, PH_EDGES)
    L.assert_chi2(direction_bins(refl, CT_EDGES, PH_EDGES), probs, ("reflected directions", alpha))


# -- 3. transmission law --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [0.1, 0.4])
def test_transmission_follows_the_refraction_jacobian_and_the_host_tracer(alpha):
    theta = math.radians(55.0)
    start, d = outside_ray(theta)
    scene = rough_block_scene(alpha)
    kind, out = first_surface_event(scene, start, d)
    v = -np.asarray(d)
    trans = out[kind == TRANSMIT]
    assert np.all(trans[:, 2] < 0.0)
    probs, _ = folded_bin_probs(transmitted_density, v, alpha, 1.0, 1.5, False, CT_EDGES, PH_EDGES)
    L.assert_chi2(direction_bins(trans, CT_EDGES, PH_EDGES), probs, ("transmitted directions", alpha))
    # the host tracer, same contract, numpy's stream: the same distribution
    np.random.seed(int(100 * alpha))
    host = []
    for _ in range(3000):
        hist = photon_tracer.follow(scene, Ray(start, d, 555.0), maxsteps=2, backend="host")
        if hist[1][1].name == "TRANSMIT":
            host.append(hist[1][0].direction)
    host = np.asarray(host)
    L.assert_ks2(trans[:200_000, 2], host[:, 2], ("polar", alpha))
    L.assert_ks2(np.arctan2(trans[:200_000, 1], trans[:200_000, 0]), np.arctan2(host[:, 1], host[:, 0]), ("azimuth", alpha))


# -- 4. escape beyond the critical angle ----------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [0.1, 0.4])
def test_escape_beyond_the_critical_angle_is_one_minus_the_vndf_reflectance(alpha):
    theta = math.radians(60.0)   # (critical angle of n = 1.5: 41.8 degrees; a smooth face traps every ray)
    start, d = inside_ray(theta)
    kind, out = first_surface_event(rough_block_scene(alpha), start, d)
    v = np.array([-math.sin(theta), 0.0, math.cos(theta)])   # (mirrored so that the face's normal towards it is +z)
    p_escape = 1.0 - reflect_probability(v, alpha, 1.5, 1.0)
    assert p_escape > 0.01
    L.assert_binomial(int(np.sum(kind == TRANSMIT)), kind.size, p_escape, ("escape", alpha))
    assert np.all(out[kind == TRANSMIT][:, 2] > 0.0) and np.all(out[kind == REFLECT][:, 2] < 0.0)
    smooth, _ = first_surface_event(rough_block_scene(0.0), start, d, n=10_000)
    assert np.all(smooth == REFLECT)


# -- 5. dispersion ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wl, n_exact", [(500.0, 1.51), (800.0, 1.40)])
def test_a_dispersive_rough_face_uses_n_at_the_photons_wavelength(wl, n_exact):
    alpha, theta = 0.3, math.radians(65.0)
    start, d = outside_ray(theta)
    kind, _ = first_surface_event(rough_block_scene(alpha, index=INDEX_TABLE), start, d, wavelength=wl)
    v = -np.asarray(d)
    L.assert_binomial(int(np.sum(kind == REFLECT)), kind.size, reflect_probability(v, alpha, 1.0, n_exact), ("n(wl)", wl))


# -- 6. coated points ---------------------------------------------------------------------------------------------------
def test_coated_points_draw_nothing():
    coat = [Coating((0.0, 0.0, 1.0), reflectivity=1.0)]   # a mirror on the top face: these rays meet nothing else
    start, d = outside_ray(math.radians(35.0))
    a, _ = B.trace_pencil(rough_block_scene(0.0, coatings=coat), start, d, 555.0, 100_000, seed=3, record_every=1,
                          max_events=8)
    b, _ = B.trace_pencil(rough_block_scene(0.3, coatings=coat), start, d, 555.0, 100_000, seed=3, record_every=1,
                          max_events=8)
    assert np.all(a["kind"].reshape(-1, 8)[:, 1] == REFLECT)
    for k in HIST_KEYS:
        assert np.array_equal(a[k], b[k]), k


# -- 7. invariance ------------------------------------------------------------------------------------------------------
def with_roughness(scene, alpha):
    """Every Fresnel-family surface of `scene` at GGX width alpha (None: untouched)."""
    if alpha is None:
        return scene
    stack = [scene.root]
    while stack:
        node = stack.pop()
        stack.extend(node.children)
        g = node.geometry
        if g is None or g.material is None:
            continue
        delegate = g.material.surface.delegate
        if isinstance(delegate, FresnelSurfaceDelegate):
            delegate._roughness = float(alpha)
    return scene


DET_SCENES = {"lsc": scenes.lsc_equivalent, "tiles6": scenes.tiles6, "mesh_lsc": scenes.mesh_lsc}


def _submit(session, rays, seed, **kw):
    pos, dirs, wl = rays
    return session.collect(session.submit(len(wl), seed, host_rays=(pos, dirs, wl, ["r"] * len(wl)), **kw))


@pytest.mark.parametrize("name", sorted(DET_SCENES))
def test_ray_histories_do_not_depend_on_the_launch(name):
    scene = with_roughness(DET_SCENES[name](), 0.3)
    assert compile_scene(scene).has_roughness
    n, every, seed, me = 1_000_000, 15_625, 23, 48
    pos, dirs, wl, _ = emit_bundle(scene, n, seed=24)
    with Session(scene, emission="host") as s:
        big = _submit(s, (pos, dirs, wl), seed, record_every=every, max_events=me, emit_method="kT")
        data = {k: np.asarray(big.data[k]) for k in HIST_KEYS}
        assert np.any(data["kind"] == REFLECT) and np.any(data["kind"] == TRANSMIT)
        for j in range(0, n // every, 4):   # the same ray alone, in a launch of one: traced in the tail
            i = j * every
            one = _submit(s, (pos[i:i + 1], dirs[i:i + 1], wl[i:i + 1]), seed, record_every=1, max_events=me,
                          emit_method="kT", ray_offset=i)
            k = int(data["counts"][j])
            assert int(one.data["counts"][0]) == k, (name, i)
            for key in HIST_KEYS[1:]:
                assert np.array_equal(np.asarray(one.data[key])[:k], data[key][j * me:j * me + k]), (name, i, key)
        m = 8192
        hist = _submit(s, (pos[:m], dirs[:m], wl[:m]), seed, record_every=1, max_events=512, maxsteps=200,
                       emit_method="kT")
        tally = _submit(s, (pos[:m], dirs[:m], wl[:m]), seed, record_every=0, maxsteps=200, emit_method="kT")
        for key in TALLY_KEYS:
            assert np.array_equal(np.asarray(hist.data[key]), np.asarray(tally.data[key])), (name, key)


def test_rough_scenes_change_the_tallies():
    scene = scenes.lsc_equivalent()
    pos, dirs, wl, _ = emit_bundle(scene, 100_000, seed=4)
    out = []
    for alpha in (None, 0.3):
        with Session(with_roughness(scenes.lsc_equivalent(), alpha), emission="host") as s:
            out.append(np.asarray(_submit(s, (pos, dirs, wl), 9, record_every=0).data["rec_distinct"]).copy())
    assert not np.array_equal(out[0], out[1])


def test_carried_launches_give_the_totals_of_one_launch():
    scene = with_roughness(scenes.lsc_equivalent(), 0.3)
    compiled = compile_scene(scene)
    n, seed = 200_003, 29
    pos, dirs, wl, _ = emit_bundle(scene, n, seed=30)
    dscene = native.DeviceScene(compiled, device=0)
    try:
        dev = torch.device("cuda", 0)
        rays = tuple(torch.from_numpy(a).to(dev) for a in (pos, dirs, wl))
        whole = dscene.new_tallies()
        dscene.trace(rays, n, seed, whole)
        parts = dscene.new_tallies()
        edges = [0, 70_000, 70_064, 150_000, n]
        for a, b in zip(edges[:-1], edges[1:]):
            dscene.trace(tuple(t[a:b] for t in rays), b - a, seed, parts, ray_offset=a, carry_out=True)
        dscene.trace(None, 0, 0, parts)
        torch.cuda.synchronize()
        ints_a, ints_b = whole.ints.cpu().numpy(), parts.ints.cpu().numpy()
        assert np.array_equal(ints_a, ints_b)
        assert ints_a.sum() > 0
    finally:
        dscene.close()


def test_device_emission_split_launches_equal_one_launch():
    scene = with_roughness(scenes.lsc_equivalent(), 0.3)
    n = 300_000
    with Session(scene, emission="device") as s:
        one = s.collect(s.submit(n, 13, record_every=0, emit_seed=21))
        whole = {k: np.asarray(one.data[k]).copy() for k in TALLY_KEYS}
        total = None
        for a, b in ((0, 100_000), (100_000, n)):
            r = s.collect(s.submit(b - a, 13, record_every=0, emit_seed=21, ray_offset=a))
            part = {k: np.asarray(r.data[k]).copy() for k in TALLY_KEYS}
            total = part if total is None else {k: total[k] + part[k] for k in TALLY_KEYS}
    for k in TALLY_KEYS:
        assert np.array_equal(whole[k], total[k]), k
    assert whole["rec_distinct"].sum() > 0


def test_the_packer_refuses_bad_roughness():
    import ctypes as C

    compiled = compile_scene(rough_block_scene(0.2))
    lib = native.load_library()
    st, keep = native.scene_tables_struct(compiled)
    for bad in BAD_ROUGHNESS:
        rt, alpha = surface_tables(bad)
        handle = C.c_void_p()
        rc = lib.pvt_scene_create_rough(C.byref(st), None, None, C.byref(rt), 0, C.byref(handle))
        assert rc != 0 and not handle.value, bad
    rt, zeros = surface_tables(0.0)
    handle = C.c_void_p()
    assert lib.pvt_scene_create_rough(C.byref(st), None, None, C.byref(rt), 0, C.byref(handle)) == 0
    lib.pvt_scene_destroy(handle)
