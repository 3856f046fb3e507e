"""Solids of revolution of a conic (`pvtrace_amd.Conicoid`, PVT_GEOM_CONICOID) on the GPU.  The oracle does not know the
shape; the engine is held to the host class bit for bit (itself held to an exact rational reference,
tests/test_conicoid.py), to the host tracer's geometry step by step, to two per-ray focus laws, to two closed-form laws,
and to itself across launch shapes.

1. The first surface event of every ray of tests/conicoid_cases.py's families -- logged distance, position and normal -- is what
   the host class gives, `np.array_equal`, in the node's own frame and through a rotated and translated node (the host
   applies the node's matrices in the kernel's operation order).  Ambiguous rays are set aside, at most 2 % of a family.
2. Every STEP of 2 048 engine histories in a dyed dome of index 1.5 (with a bead inside it) is a step of the host tracer's
   own interface search, as tests/test_gpu_frustum.py's test of that name.
3. Focus laws, 4 096 rays each, on a perfect mirror of index 1 in a world of index 1: a paraboloid sends every
   axis-parallel ray through its focus, a prolate spheroid every ray from one focus through the other.  The test proves
   the law itself in rationals, holds the logged point to B(t) and the logged direction to the exact reflected one within
   eight times the host tracer's own worst deviation on the same rays (not less than 16 * 2^-53).  Observed on an MI355X,
   worst deviation in u = 2^-53: paraboloid, host tracer 6.74, engine 6.74 (allowed 53.9); prolate spheroid, host tracer
   23.01, engine 7.99 (allowed 184.1).
4. The solid-angle partition of a point source on a dome's axis and the mean chord 4V/S at 200 000 rays, from recorders
   and from the log, within 4 standard errors; observed: z = +0.07 (base), -0.07 (side); 25 240 chords, z = -1.45.
5. Launch shapes: tally against history launches, device against host emission, carried launches, two shards on one GPU,
   a mesh and a polyhedron beside a dome, a 3 x 3 array with and without PVT_NO_GRID.
6. A recorder and a mirror on a dome's base fire there and nowhere else; a pole never yields a cap normal.
7. The entries: every older one refuses the type, the newest takes it without polyhedron tables, the packer refuses each
   malformed parameter set with its own message, the host-buffer entry refuses first.
8. examples/dome_lens.py.
"""
import ctypes
import functools
import importlib.util
import math
import os
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

from pvtrace_amd import (
    Absorber, Box, CoatedSurfaceDelegate, Coating, Conicoid, Light, Luminophore, Material, Mesh, Node, Polyhedron, Ray, Scene,
    Sphere, Surface, cone,
)
from pvtrace_amd.algorithm import photon_tracer
from pvtrace_amd.data import lumogen_f_red_305
from pvtrace_amd.engine import Recorder, Session, _kernel, compile_scene, native, simulate
from pvtrace_amd.engine.compiler import UnsupportedSceneError
from pvtrace_amd.engine.emit import emit_bundle
from tests import conicoid_cases as C
from tests.test_conicoid import (
    conicoid, dome_array, exact_first_reflections, focus_cases, host_direction_deviation, mirror_scene,
)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERATE, REFLECT, TRANSMIT, ABSORB, EXIT = 0, 1, 2, 3, 7
TALLY_KEYS = ("rec_distinct", "rec_crossings", "rec_bins")
LOG_KEYS = ("counts", "kind", "hit", "container", "adjacent", "position", "direction", "normal", "wavelength", "travelled",
            "duration")
X = np.arange(400, 800)
U = 2.0 ** -53


def air(radius=50.0):
    return Node(name="world", geometry=Sphere(radius=radius, material=Material(refractive_index=1.0)))


def dye():
    return Luminophore(coefficient=np.column_stack((X, lumogen_f_red_305.absorption(X) * 5.0)),
                       emission=np.column_stack((X, lumogen_f_red_305.emission(X))), quantum_yield=1.0, name="Lumogen F Red 305")


def trace(scene, pos, dirs, wl=555.0, seed=3, record_every=1, max_events=8, **kw):
    """-> (columns of the result, variant of the launch)"""
    n = len(pos)
    wl = np.full(n, float(wl)) if np.isscalar(wl) else np.asarray(wl, dtype=np.float64)
    with Session(scene, emission="host") as s:
        r = s.collect(s.submit(n, seed, max_events=max_events, record_every=record_every,
                               host_rays=(np.ascontiguousarray(pos), np.ascontiguousarray(dirs), wl, ["r"] * n), **kw))
        keys = TALLY_KEYS + (LOG_KEYS if record_every else ())
        return {k: np.asarray(r.data[k]).copy() for k in keys}, s.dscene.launch_info()["variant"]


# -- 1. bit for bit against the host class ----------------------------------------------------------------------------------
def posed(node, pose):
    if pose is not None:
        angle, axis, shift = pose
        node.rotate(angle, axis)
        node.translate(shift)
    return node


def check_first_events(scene, shape, families, node_name="solid"):
    """Every family's rays, given in the node's frame, sent through `scene` in its world: the first surface event on the
    node against the host class.  -> rays judged."""
    compiled = compile_scene(scene)
    node = list(compiled.node_names).index(node_name)
    l2w, w2l = compiled.local_to_world[node], compiled.world_to_local[node]
    params = C.SHAPES[shape]
    solid = conicoid(shape)
    local = [C.rays(shape, f) for f in families]
    o = np.vstack([r[0] for r in local])
    d = np.vstack([r[1] for r in local])
    pos = o @ l2w[:3, :3].T + l2w[:3, 3]
    dirs = d @ l2w[:3, :3].T
    assert len(pos) <= 4096
    data, variant = trace(scene, pos, dirs, max_events=4)
    assert variant == "rough"
    row1 = np.arange(len(pos)) * 4 + 1
    kind, hit = data["kind"][row1], data["hit"][row1]
    position, normal, distance = data["position"][row1], data["normal"][row1], data["travelled"][row1]
    judged = 0
    for f, family in enumerate(families):
        ambiguous = 0
        for i in range(f * C.N_RAYS, (f + 1) * C.N_RAYS):
            ol, dl = C.to_local(w2l, pos[i], dirs[i])   # the node's frame as the kernel reaches it
            if C.exact_crossings(params, ol, dl)[1]:
                ambiguous += 1
                continue
            ts = solid._ray_distances(ol, dl)
            if not ts:
                assert hit[i] != node, (shape, family, i)
                continue
            t = min(ts)
            assert hit[i] == node and kind[i] in (REFLECT, TRANSMIT), (shape, family, i, kind[i], hit[i])
            assert distance[i] == t, (shape, family, i, distance[i], t)      # (a fresh ray has travelled 0: the row holds t itself)
            want = pos[i] + dirs[i] * t
            assert np.array_equal(position[i], want), (shape, family, i, position[i], want)
            n_local = solid.normal(C.to_local(w2l, want, dirs[i])[0])
            assert np.array_equal(normal[i], C.rotate(l2w[:3, :3], n_local)), (shape, family, i, normal[i], n_local)
            judged += 1
        assert ambiguous <= C.MAX_AMBIGUOUS * C.N_RAYS, (shape, family, ambiguous)
    return judged


@pytest.mark.parametrize("pose", sorted(C.POSES))
@pytest.mark.parametrize("shape", sorted(C.SHAPES))
def test_first_surface_event_is_the_host_class_bit_for_bit(shape, pose):
    world = air()
    posed(Node(name="solid", parent=world, geometry=conicoid(shape, material=Material(refractive_index=1.5))), C.POSES[pose])
    assert check_first_events(Scene(world), shape, C.families_of(shape)) > 1000


# -- 2. the host tracer's geometry, step by step -------------------------------------------------------------------------
def nested_scene():
    world = Node(name="world", geometry=Box((40.0, 40.0, 40.0), material=Material(refractive_index=1.0)))
    block = Node(name="block", parent=world, geometry=Box((5.0, 5.0, 5.0), material=Material(refractive_index=1.2)))
    dome = Node(name="dome", parent=block,
                geometry=Conicoid.spherical_cap(1.5, 1.0, material=Material(refractive_index=1.5, components=[dye()])))
    dome.rotate(0.3, (1.0, 1.0, 0.0))
    bead = Node(name="bead", parent=dome, geometry=Sphere(0.2, material=Material(refractive_index=1.8)))
    bead.location = (0.1, 0.0, -0.15)
    return Scene(world)


def test_every_step_of_an_engine_history_is_a_step_of_the_host_tracers_geometry():
    scene = nested_scene()
    rng = np.random.default_rng(8)
    n, me = 2048, 64
    pos = np.column_stack((rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n), np.full(n, -8.0)))
    dirs = C._unit(np.column_stack((rng.normal(0.0, 0.1, n), rng.normal(0.0, 0.1, n), np.ones(n))))
    with Session(scene, emission="host") as s:
        result = s.collect(s.submit(n, 17, max_events=me, maxsteps=30, record_every=1,
                                    host_rays=(pos, dirs, np.full(n, 480.0), ["r"] * n)))
        assert s.dscene.launch_info()["variant"] == "rough"
    steps = surface_steps = absorptions = 0
    seen = set()
    for history in result.histories():
        for (before, _, _), (after, event, meta) in zip(history[:-1], history[1:]):
            if event.name in ("EMIT", "SCATTER", "NONRADIATIVE", "REACT", "KILL"):
                continue   # (no flight: the row follows an ABSORB where it stands, or ends the ray)
            found = photon_tracer._interface_ahead(scene, before)
            assert found is not None
            hit, container, _, distance = found
            steps += 1
            if event.name == "ABSORB":
                assert meta["container"] == container.name
                assert after.travelled - before.travelled < distance
                absorptions += 1
                continue
            assert (meta["hit"], meta["container"]) == (hit.name, container.name), (before, meta)
            want = np.asarray(before.position) + distance * np.asarray(before.direction)
            assert np.allclose(after.position, want, rtol=0, atol=1e-12), (before, after)
            if event.name in ("REFLECT", "TRANSMIT"):
                at = Ray(position=tuple(want), direction=before.direction, wavelength=before.wavelength)
                local = at.representation(scene.root, hit)
                normal = hit.vector_to_node(hit.geometry.normal(local.position), scene.root)
                assert np.allclose(meta["normal"], normal, rtol=0, atol=1e-12), (before, meta)
                surface_steps += 1
                seen.add(hit.name)
    assert seen >= {"block", "dome"}
    assert steps > 2 * n and surface_steps > 2 * n and absorptions > 100, (steps, surface_steps, absorptions)


# -- 3. the focus laws, ray by ray ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["paraboloid", "prolate"])
def test_a_mirror_sends_every_ray_through_the_focus(case):
    name, maker, params, origins, directions, focus = next(c for c in focus_cases() if c[0] == case)
    assert len(origins) == 4096
    exact = exact_first_reflections(params, origins, directions, focus)      # (proves the law in rationals, ray by ray)
    host_worst = host_direction_deviation(maker, params, origins, directions, exact)
    allowed = max(8.0 * host_worst, 16.0 * U)
    data, variant = trace(mirror_scene(maker), origins, directions, max_events=8, maxsteps=3)
    assert variant == "rough"
    row1 = np.arange(len(origins)) * 8 + 1
    assert np.all(data["kind"][row1] == REFLECT) and np.all(data["hit"][row1] == 1)
    gpu_worst = 0.0
    for i, (crossing, point, reflected) in enumerate(exact):
        span = float(crossing.bound) + 4 * U * (1.0 + abs(float(crossing.t)))     # (B, and forming o + t*d)
        assert all(abs(float(Fr(float(got)) - want)) <= span for got, want in zip(data["position"][row1[i]], point)), i
        gpu_worst = max(gpu_worst, max(abs(float(Fr(float(got)) - want)) for got, want in zip(data["direction"][row1[i]], reflected)))
    print(f"{name}: worst deviation from the exact reflected direction: host tracer {host_worst / U:.2f} u, engine "
          f"{gpu_worst / U:.2f} u (allowed {allowed / U:.1f} u)")
    assert gpu_worst <= allowed, (gpu_worst / U, allowed / U)


# -- 4. the two laws -----------------------------------------------------------------------------------------------------------
N_LAW = 200_000


def z_binomial(k, n, p):
    return (k - n * p) / math.sqrt(n * p * (1.0 - p))


def test_solid_angle_partition_from_recorders_and_from_the_log():
    scene = C.law_scene(recorders=True)
    pos, dirs = C.point_source_rays(N_LAW)
    data, variant = trace(scene, pos, dirs, max_events=4)
    assert variant == "rough"
    names = [r.name for r in compile_scene(scene).recorder_specs]
    tally = {name: int(data["rec_distinct"][i]) for i, name in enumerate(names)}
    assert tally["all"] == N_LAW and tally["top"] == 0      # (the top is a pole: no ray leaves through a cap there)
    where = C.which_surface(data["position"][np.arange(N_LAW) * 4 + 1])
    from_log = [int(np.sum(where == j)) for j in range(2)]
    from_tally = [tally["base"], tally["all"] - tally["base"]]
    assert from_log == from_tally
    for name, k, p in zip(("base", "side"), from_tally, C.partition_probabilities()):
        z = z_binomial(k, N_LAW, p)
        print(f"{name}: {k} of {N_LAW}, expected {N_LAW * p:.1f}, z = {z:+.2f}")
        assert abs(z) <= 4.0, (name, k, z)
    tallies_only, _ = trace(scene, pos, dirs, record_every=0)
    assert np.array_equal(tallies_only["rec_distinct"], data["rec_distinct"])


def test_mean_chord_from_the_log():
    scene = C.law_scene(recorders=True)
    pos, dirs = C.chord_rays(N_LAW)
    data, _ = trace(scene, pos, dirs, max_events=4)
    counts = data["counts"]
    assert set(np.unique(counts).tolist()) <= {2, 4}
    through = np.flatnonzero(counts == 4)
    p_in, p_out = data["position"][through * 4 + 1], data["position"][through * 4 + 2]
    chords = np.sqrt(np.sum((p_out - p_in) ** 2, axis=1))
    z = (chords.mean() - C.mean_chord()) / (chords.std(ddof=1) / math.sqrt(len(chords)))
    print(f"{len(chords)} chords, mean {chords.mean():.5f}, 4V/S = {C.mean_chord():.5f}, z = {z:+.2f}")
    assert len(chords) > 20_000 and abs(z) <= 4.0, z
    names = [r.name for r in compile_scene(scene).recorder_specs]
    assert int(data["rec_distinct"][names.index("all")]) == len(chords)   # (every chord ends in one escape)


# -- 5. launch shapes --------------------------------------------------------------------------------------------------------
STEPS, ROWS = 50, 2 * 50 + 8   # a step writes at most two rows; GENERATE and the closing row come on top


def guide_scene(mesh=False, prism=False):
    """A dyed PMMA dome under a lamp, in air; optionally beside a mesh and a polyhedron."""
    world = air(20.0)
    recorders = [Recorder("top", event="escaping", facet=(0.0, 0.0, 1.0)), Recorder("base", event="escaping", facet=(0.0, 0.0, -1.0)),
                 Recorder("escaping", event="escaping"), Recorder("entering", event="entering"), Recorder("lost", event="lost")]
    dome = Node(name="solid", parent=world, recorders=recorders,
                geometry=conicoid("dome", material=Material(refractive_index=1.5, components=[dye(), Absorber(0.05, name="host")])))
    dome.location = (0.0, 0.2, 0.0)   # (unrotated: a recorder's facet is matched in the root's frame)
    if mesh:
        gem = Node(name="gem", parent=world, geometry=Mesh.icosphere(1, 0.6, material=Material(refractive_index=1.6)))
        gem.location = (2.5, 0.0, 0.0)
    if prism:
        nut = Node(name="nut", parent=world, geometry=Polyhedron.regular_prism(6, 0.6, 0.8, material=Material(refractive_index=1.4)))
        nut.location = (-2.5, 0.0, 0.0)
    light = Node(name="Light", parent=world, light=Light(direction=functools.partial(cone, np.radians(25)), name="Light"))
    light.location = (0.3, 0.0, -4.0)
    return Scene(world)


def test_tally_history_device_emission_and_carried_launches_agree():
    scene = guide_scene()
    n = 4096
    with Session(scene, emission="device") as s:
        assert s.emission == "device"
        # (a recorded ray whose log is full is killed untallied, as in the reference: the log holds every step's rows)
        tally = s.collect(s.submit(n, 13, record_every=0, emit_seed=21, maxsteps=STEPS))
        hist = s.collect(s.submit(n, 13, record_every=1, max_events=ROWS, emit_seed=21, maxsteps=STEPS))
        assert s.dscene.launch_info()["variant"] == "rough"
        device = {k: np.asarray(tally.data[k]).copy() for k in TALLY_KEYS}
        for k in TALLY_KEYS:
            assert np.array_equal(device[k], np.asarray(hist.data[k])), k
        first = np.arange(n) * ROWS
        assert np.all(np.asarray(hist.data["kind"])[first] == GENERATE)
        rays = tuple(np.asarray(hist.data[k])[first].copy() for k in ("position", "direction", "wavelength"))
    host, _ = trace(scene, *rays, seed=13, record_every=0, maxsteps=STEPS)
    for k in TALLY_KEYS:
        assert np.array_equal(device[k], host[k]), k
    assert device["rec_distinct"].min() > 0
    # two carried launches equal one
    dscene = native.DeviceScene(compile_scene(scene), device=0)
    try:
        dev = torch.device("cuda", 0)
        drays = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in rays)
        whole, parts = dscene.new_tallies(), dscene.new_tallies()
        dscene.trace(drays, n, 13, whole, maxsteps=STEPS)
        cut = 1_033
        dscene.trace(tuple(t[:cut] for t in drays), cut, 13, parts, ray_offset=0, carry_out=True, maxsteps=STEPS)
        dscene.trace(tuple(t[cut:] for t in drays), n - cut, 13, parts, ray_offset=cut, carry_out=False, maxsteps=STEPS)
        torch.cuda.synchronize()
        assert np.array_equal(whole.ints.cpu().numpy(), parts.ints.cpu().numpy()) and int(whole.ints.sum()) > 0
    finally:
        dscene.close()


def test_two_shards_on_one_gpu_equal_one_launch_and_the_host_buffer_entry_refuses():
    scene = guide_scene()
    n = 4096
    sharded = simulate(scene, n, seed=4, record_every=0, emission="device", emit_seed=8, devices=[0, 0])
    whole = simulate(scene, n, seed=4, record_every=0, emission="device", emit_seed=8)
    for k in TALLY_KEYS:
        assert np.array_equal(np.asarray(sharded.data[k]), np.asarray(whole.data[k])), k
    assert np.asarray(whole.data["rec_distinct"]).min() > 0
    pos, dirs, wl, _ = emit_bundle(scene, 16, seed=6)
    with pytest.raises(UnsupportedSceneError, match="Conicoid"):
        _kernel.trace_bundle(compile_scene(scene), pos, dirs, wl, 4, 100, 16, 0, 1, 1)


def test_a_mesh_and_a_polyhedron_beside_a_conicoid():
    world = air()
    Node(name="solid", parent=world, geometry=conicoid("dome", material=Material(refractive_index=1.5)))
    gem = Node(name="gem", parent=world, geometry=Mesh.icosphere(1, 0.8, material=Material(refractive_index=1.6)))
    gem.location = (0.0, 12.0, 0.0)   # (beyond the reach of the families' rays before they meet the dome)
    nut = Node(name="nut", parent=world, geometry=Polyhedron.regular_prism(6, 0.6, 0.8, material=Material(refractive_index=1.4)))
    nut.location = (0.0, -12.0, 0.0)
    scene = Scene(world)
    compiled = compile_scene(scene)
    assert compiled.has_conicoid and compiled.has_polyhedron and compiled.n_mesh_faces > 0
    assert check_first_events(scene, "dome", ["outside", "inside", "rims"]) > 500
    lit = guide_scene(mesh=True, prism=True)
    pos, dirs, wl, _ = emit_bundle(lit, 4096, seed=2)
    pos[::3] = (2.5, 0.0, -4.0)    # (every third ray from below the gem ...)
    pos[1::3] = (-2.5, 0.0, -4.0)  # (... and every third from below the prism)
    a, variant = trace(lit, pos, dirs, wl, seed=5, record_every=0, maxsteps=STEPS)
    b, _ = trace(lit, pos, dirs, wl, seed=5, record_every=1, max_events=ROWS, maxsteps=STEPS)
    assert variant == "rough"
    for k in TALLY_KEYS:
        assert np.array_equal(a[k], b[k]), k
    names = list(compile_scene(lit).node_names)
    assert all(np.any(b["hit"] == names.index(name)) for name in ("solid", "gem", "nut")) and a["rec_distinct"].min() > 0


def test_an_array_of_domes_with_and_without_the_grid_switch(monkeypatch):
    scene = dome_array()
    scene.root.children[1].recorders = [Recorder("in", event="entering"), Recorder("out", event="escaping")]
    compiled = compile_scene(scene)
    assert compiled.geom_type.shape[0] >= 8
    rng = np.random.default_rng(3)
    n = 4096
    pos = np.column_stack((rng.uniform(-3.0, 3.0, n), rng.uniform(-3.0, 3.0, n), np.full(n, 5.0)))
    dirs = C._unit(np.column_stack((rng.normal(0.0, 0.3, n), rng.normal(0.0, 0.3, n), -np.ones(n))))
    out = []
    for switch in (False, True):
        if switch:
            monkeypatch.setenv("PVT_NO_GRID", "1")
        dscene = native.DeviceScene(compiled, device=0)
        try:
            dev = torch.device("cuda", 0)
            rays = tuple(torch.from_numpy(a).to(dev) for a in (pos, dirs, np.full(n, 555.0)))
            tallies = dscene.new_tallies()
            dscene.trace(rays, n, 9, tallies)
            torch.cuda.synchronize()
            out.append(tallies.ints.cpu().numpy().copy())
            assert dscene.launch_info()["variant"] == "rough"
        finally:
            dscene.close()
    assert np.array_equal(out[0], out[1]) and out[0].sum() > 0      # (identical: there is no grid either way)


# -- 6. facets -----------------------------------------------------------------------------------------------------------------
def test_a_base_mirror_and_recorder_fire_at_the_base_and_a_pole_yields_no_cap_normal():
    world = air()
    mirror = Surface(CoatedSurfaceDelegate([Coating((0.0, 0.0, -1.0), reflectivity=1.0)]))
    cap = Conicoid.spherical_cap(*C.LAW_CAP, material=Material(refractive_index=1.0, surface=mirror))
    params = (cap.length,) + cap.profile
    recorders = lambda: [Recorder("base", event="escaping", facet=(0.0, 0.0, -1.0)),      # noqa: E731
                         Recorder("top", event="escaping", facet=(0.0, 0.0, 1.0)), Recorder("all", event="escaping")]
    Node(name="solid", parent=world, geometry=cap, recorders=recorders())
    scene = Scene(world)
    families = ("outside", "inside", "rims", "pole", "paraxial")
    o = np.vstack([C.rays(params, f)[0] for f in families])
    d = np.vstack([C.rays(params, f)[1] for f in families])
    data, variant = trace(scene, o, d, max_events=8)
    assert variant == "rough"
    row1 = np.arange(len(o)) * 8 + 1
    kind, normal = data["kind"][row1], data["normal"][row1]
    on_solid = data["hit"][row1] == 1
    base = on_solid & (normal[:, 2] == -1.0) & (normal[:, 0] == 0.0) & (normal[:, 1] == 0.0)
    assert base.sum() > 100 and (on_solid & ~base).sum() > 300
    assert np.all(kind[base] == REFLECT)                 # the mirror: every ray that reaches the base, from either side
    assert np.all(kind[on_solid & ~base] == TRANSMIT)    # an n = 1 surface in an n = 1 world anywhere else: none is reflected
    every = data["normal"][(data["hit"] == 1) & np.isin(data["kind"], (REFLECT, TRANSMIT))]
    assert len(every) > 1000 and not np.any(every[:, 2] == 1.0)      # the pole end: the gradient, never (0, 0, 1)
    # the base mirrors from both sides, so nothing ever leaves through it: its recorder stays silent, like the pole's
    assert int(data["rec_distinct"][0]) == 0 and int(data["rec_distinct"][1]) == 0 and int(data["rec_distinct"][2]) > 500
    # without the mirror the base's recorder counts exactly the rays the log shows leaving through the base
    bare = air()
    Node(name="solid", parent=bare, geometry=Conicoid.spherical_cap(*C.LAW_CAP, material=Material(refractive_index=1.0)),
         recorders=recorders())
    plain, _ = trace(Scene(bare), o, d, max_events=8)
    rows = (plain["hit"] == 1) & (plain["kind"] == TRANSMIT) & (plain["container"] == 1)
    through_base = rows & (plain["normal"][:, 2] == -1.0)
    assert int(plain["rec_distinct"][0]) == int(through_base.sum()) > 100
    assert int(plain["rec_distinct"][1]) == 0 and int(plain["rec_distinct"][2]) == int(rows.sum())


# -- 7. the entries ------------------------------------------------------------------------------------------------------------
def _create(compiled, entry, mutate=None):
    """Call a creation entry with the scene's own structs -> (return code, message, whether a scene came back)."""
    lib = native.load_library()
    st, keep = native.scene_tables_struct(compiled)
    count = dict(native.CREATION_ENTRIES, **dict([native.NEWEST_ENTRY]))[entry]
    made = [native.marshal(t, compiled) for t in native.EXTENSION_TABLES[:count]]
    if mutate is not None:
        mutate(keep)
    handle = ctypes.c_void_p()
    rc = getattr(lib, entry)(ctypes.byref(st), *[None if m is None else ctypes.byref(m) for m, _ in made], 0, ctypes.byref(handle))
    message = (lib.pvt_last_error() or b"").decode() if rc != 0 else ""
    came_back = bool(handle.value)
    if rc == 0:
        lib.pvt_scene_destroy(handle)
    del keep
    return rc, message, came_back, made


def test_older_entries_refuse_the_type_and_malformed_parameters_are_refused_each_with_its_own_message():
    assert native.NEWEST_ENTRY == ("pvt_scene_create_polyhedra", 10) and len(native.CREATION_ENTRIES) == 11
    fresh = lambda: compile_scene(guide_scene())     # noqa: E731  (the structs point INTO the lowered tables)
    for entry in native.CREATION_ENTRIES:
        assert _create(fresh(), entry)[:3] == (-1, "unknown geometry type", False), entry
    rc, message, came_back, made = _create(fresh(), native.NEWEST_ENTRY[0])
    assert (rc, message, came_back) == (0, "", True) and made[-1] == (None, {})      # (NULL polyhedron tables)
    assert native.load_library().pvt_abi_version() == 13

    def params(*values):
        def mutate(keep):
            keep["geom_params"].reshape(-1, 4)[1] = values
        return mutate

    cases = [
        (params(math.nan, 1.0, 0.0, -1.0), "must be finite numbers"), (params(1.0, 1.0, math.inf, 0.0), "must be finite numbers"),
        (params(0.0, 1.0, 0.0, 0.0), "length must be > 0"), (params(-1.0, 1.0, 0.0, 0.0), "length must be > 0"),
        (params(1.0, 0.0, 0.0, 1.0), "no interior or is pinched"), (params(1.0, -1.0, 0.0, 0.0), "no interior or is pinched"),
        (params(1.0, 0.1, 1.0, 0.0), "negative at an end"), (params(3.0, 1.0, 0.0, -1.0), "negative at an end"),
        (params(4.0, 0.01, 0.0, 1.0), "not convex"), (params(1.0, 1.0, 0.0, 1.0), "not convex"),
    ]
    for mutate, text in cases:
        compiled = fresh()
        rc, message, came_back, _ = _create(compiled, native.NEWEST_ENTRY[0], mutate)
        assert rc == -1 and text in message and not came_back, (text, rc, message)
        L, p0, p1, p2 = compiled.geom_params[1]
        assert message == Conicoid.parameter_problem(L, (p0, p1, p2)), message      # the same words as the class
    assert len({text for _, text in cases}) == 5


# -- 8. the example -------------------------------------------------------------------------------------------------------------
def test_the_dome_lens_example_runs():
    spec = importlib.util.spec_from_file_location("dome_lens", os.path.join(ROOT, "examples", "dome_lens.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    rows = module.main(photons=20_000)
    flat, hemisphere = rows["flat"]["escaping"], rows["dome 1.00"]["escaping"]
    print(f"flat cover {flat:.3f}, hemisphere {hemisphere:.3f}")
    assert hemisphere > flat
    # the closed forms of the example's docstring, within 4 binomial sigma of 20 000 photons (0.24 % at p = 0.127): a flat
    # face lets out at most the critical cone's 12.7 % -- the flat cover's top and every cover's base -- and the hemisphere
    # at least 0.96 (1 - 0.127) = 83.8 % on the first pass (what it reflects gets further chances: no upper bound but 1)
    sigma = math.sqrt(0.127 * 0.873 / 20_000)
    assert flat <= 0.127 + 4.0 * sigma and all(row["base"] <= 0.127 + 4.0 * sigma for row in rows.values() if row["height"] in (None, 1.0))
    assert hemisphere >= 0.96 * (1.0 - 0.127) - 4.0 * sigma
    total = hemisphere + rows["dome 1.00"]["base"] + rows["dome 1.00"]["lost"]
    assert 0.999 < total <= 1.0 + 1e-12      # every photon ends somewhere (but for one that runs out of steps)
