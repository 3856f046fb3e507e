"""Convex polyhedra (`pvtrace_amd.Polyhedron`, PVT_GEOM_POLYHEDRON) on the GPU.  The oracle does not know the shape; the
engine is held to the host class bit for bit (itself held to an exact rational reference, tests/test_polyhedron.py), to the
host tracer's geometry step by step, to two closed-form laws, and to itself across launch shapes.

 1. The first surface event of every ray of tests/polyhedron_cases.py's families -- logged position and normal -- is what
    the host class gives, `np.array_equal`, per shape, in the node's own frame and through a rotated and translated node.
    Ambiguous rays are set aside, at most 2 % of a family.
 2. Every step of an engine history is a step of the host class's geometry (the method of tests/test_gpu_frustum.py): a
    dyed hexagonal plate holding a tetrahedron of another index, beside a box that shares a face with it.  On the shared
    face both nodes are crossed at ONE distance; the engine orders crossings by the classes' own distances, the host tracer
    by |point - origin|, so which of the two names the interface there is rounding noise to the method: only there, and
    only between those two nodes, the engine's node stands in (3 of 2899 steps on an MI355X), everything else held as elsewhere.
 3. The solid-angle partition over the faces of a point source inside, from `facet=facet_normal(k)` recorders and from
    the log, against the exact solid angles of the faces, within 4 standard errors (the frustum test's bound).
 4. The mean chord 4V/S under isotropic uniform illumination, from the log, within 4 standard errors.
 5. A tally launch, a history launch, device emission, the 256-recorder variant and carried launches all agree.
 6. A ray alone plus the rest equals the whole launch.
 7. A mesh beside a polyhedron (the MESH + ROUGH variant).
 8. A polyhedron as the scene's root.
 9. A polyhedron that does not contain its node's origin.
10. A mirror coating on one side face reflects there and nowhere else; a `detected` recorder on another counts its DETECT rows.
11. Two shards on one GPU equal one launch; the host-buffer entry refuses the shape.
12. Every creation entry before `pvt_scene_create_polyhedra` refuses type 5 with the old message; the new entry with NULL
    tables builds the scene `pvt_scene_create_aligned` builds; each malformed table is refused with its own message.
13. The example runs.
"""
import ctypes
import functools
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from pvtrace_amd import (
    Absorber, Box, CoatedSurfaceDelegate, Coating, Light, Luminophore, Material, Mesh, Node, Polyhedron, Ray, Scene, Sphere,
    Surface, cone,
)
from pvtrace_amd.algorithm import photon_tracer
from pvtrace_amd.data import lumogen_f_red_305
from pvtrace_amd.engine import Recorder, Session, _kernel, compile_scene, native, simulate
from pvtrace_amd.engine.compiler import UnsupportedSceneError
from tests import polyhedron_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERATE, REFLECT, TRANSMIT, ABSORB, EXIT, DETECT = 0, 1, 2, 3, 7, 10
TALLY_KEYS = ("rec_distinct", "rec_crossings", "rec_bins")
LOG_KEYS = ("counts", "kind", "hit", "container", "adjacent", "position", "direction", "normal", "wavelength", "travelled",
            "duration")
X = np.arange(400, 800)


def air(radius=50.0):
    return Node(name="world", geometry=Sphere(radius=radius, material=Material(refractive_index=1.0)))


def dye():
    return Luminophore(coefficient=np.column_stack((X, lumogen_f_red_305.absorption(X) * 5.0)),
                       emission=np.column_stack((X, lumogen_f_red_305.emission(X))), quantum_yield=1.0, name="Lumogen F Red 305")


def solid(name, **material):
    """The polyhedron of tests/polyhedron_cases.py's shape `name`, row for row, with a material of its own."""
    return C.shape(name).copy(material=Material(**material))


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


def check_first_events(scene, shape, ray_sets, node_name="solid"):
    """Ray sets of C.N_RAYS rays each, given in the node's frame, sent through `scene` in its world: the first surface event
    on the node against the host class `shape`.  -> rays judged."""
    compiled = compile_scene(scene)
    node = list(compiled.node_names).index(node_name)
    l2w, w2l = compiled.local_to_world[node], compiled.world_to_local[node]
    o = np.vstack([r[0] for r in ray_sets])
    d = np.vstack([r[1] for r in ray_sets])
    pos = o @ l2w[:3, :3].T + l2w[:3, 3]
    dirs = d @ l2w[:3, :3].T
    assert len(pos) <= 4096
    data, variant = trace(scene, pos, dirs, max_events=4)
    assert variant == "rough"
    row1 = np.arange(len(pos)) * 4 + 1
    kind, hit = data["kind"][row1], data["hit"][row1]
    position, normal = data["position"][row1], data["normal"][row1]
    judged = 0
    for f in range(len(ray_sets)):
        ambiguous = 0
        for i in range(f * C.N_RAYS, (f + 1) * C.N_RAYS):
            ol, dl = C.to_local(w2l, pos[i], dirs[i])   # the node's frame as the kernel reaches it
            if C.exact_crossings(shape.planes, ol, dl)[1]:
                ambiguous += 1
                continue
            ts = shape._ray_distances(ol, dl)
            if not ts:
                assert hit[i] != node, (f, i)
                continue
            t = min(ts)
            assert hit[i] == node and kind[i] in (REFLECT, TRANSMIT), (f, i, kind[i], hit[i])
            want = pos[i] + dirs[i] * t
            assert np.array_equal(position[i], want), (f, i, position[i], want)
            n_local = shape.normal(C.to_local(w2l, want, dirs[i])[0])
            assert np.array_equal(normal[i], C.rotate(l2w[:3, :3], n_local)), (f, i, normal[i], n_local)
            judged += 1
        assert ambiguous <= C.MAX_AMBIGUOUS * C.N_RAYS, (f, ambiguous)
    return judged


@pytest.mark.parametrize("pose", sorted(C.POSES))
@pytest.mark.parametrize("shape", C.SHAPES)
def test_first_surface_event_is_the_host_class_bit_for_bit(shape, pose):
    world = air()
    body = solid(shape, refractive_index=1.5)
    posed(Node(name="solid", parent=world, geometry=body), C.POSES[pose])
    families = C.families_of(shape)
    assert len(families) == (4 if shape == "tetra" else 5)
    assert check_first_events(Scene(world), body, [C.rays(shape, f) for f in families]) > 200 * len(families)


# -- 2. the host tracer's geometry, step by step -------------------------------------------------------------------------
HEXAGON = [(1.75, -1.0), (1.75, 1.0), (0.0, 2.0), (-1.75, 1.0), (-1.75, -1.0), (0.0, -2.0)]   # its +x side lies at x = 1.75 exactly


def nested_scene():
    world = Node(name="world", geometry=Box((40.0, 40.0, 40.0), material=Material(refractive_index=1.0)))
    plate = Node(name="plate", parent=world,
                 geometry=Polyhedron.prism(HEXAGON, 1.0, material=Material(refractive_index=1.5, components=[dye()])))
    gem = Node(name="gem", parent=plate,
               geometry=Polyhedron.from_vertices(0.375 * C.TETRA, material=Material(refractive_index=1.8)))
    gem.location = (-0.4, 0.2, 0.05)
    gem.rotate(0.4, (1.0, -1.0, 0.5))
    block = Node(name="block", parent=world, geometry=Box((1.0, 2.0, 1.0), material=Material(refractive_index=1.3)))
    block.location = (2.25, 0.0, 0.0)      # its -x face IS the plate's +x face
    return Scene(world)


def want_x(ray, distance):
    return float(ray.position[0]) + distance * float(ray.direction[0])


def test_every_step_of_an_engine_history_is_a_step_of_the_host_tracers_geometry():
    scene = nested_scene()
    assert scene.root.children[0].geometry.planes[0].tolist() == [1.0, 0.0, 0.0, 1.75]
    names = {"world", "plate", "gem", "block"}
    rng = np.random.default_rng(8)
    n, me = 512, 64
    pos = np.column_stack((rng.uniform(-1.2, 1.2, n), rng.uniform(-0.8, 0.8, n), np.full(n, -8.0)))
    dirs = C._unit(np.column_stack((rng.normal(0.0, 0.1, n), rng.normal(0.0, 0.1, n), np.ones(n))))
    side = slice(0, n, 4)      # every fourth ray comes in through the plate's -x side and heads for the shared face
    m = len(pos[side])
    pos[side] = np.column_stack((np.full(m, -8.0), rng.uniform(-0.7, 0.7, m), rng.uniform(-0.4, 0.4, m)))
    dirs[side] = C._unit(np.column_stack((np.ones(m), rng.normal(0.0, 0.03, m), rng.normal(0.0, 0.03, m))))
    with Session(scene, emission="host") as s:
        result = s.collect(s.submit(n, 17, max_events=me, maxsteps=30, record_every=1,
                                    host_rays=(pos, dirs, np.full(n, 480.0), ["r"] * n)))
        assert s.dscene.launch_info()["variant"] == "rough"
    steps = surface_steps = absorptions = shared = 0
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
            if meta["hit"] != hit.name:
                # The shared face: plate and block are crossed at ONE distance there.  The engine orders crossings by the
                # classes' own distances t (held bit for bit by the first test), the host tracer by |point - origin|, which
                # rounds differently, so which of the two coincident nodes names the interface is noise to the method.
                # Only there, and only between those two, the engine's node stands in; everything else is held as elsewhere
                ahead = scene.intersections(before.position, before.direction)
                twins = [x.hit for x in ahead if x.hit.name == meta["hit"] and abs(x.distance - distance) <= 1e-12]
                assert twins and {hit.name, meta["hit"]} == {"plate", "block"}, (before, meta, hit.name)
                assert abs(want_x(before, distance) - 1.75) <= 1e-12, (before, meta)
                hit = twins[0]
                shared += 1
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
    assert names >= seen >= {"plate", "gem", "block"}
    print(f"{steps} steps, {surface_steps} at surfaces, {absorptions} absorptions, {shared} named by the twin on the shared face")
    assert steps > 2000 and surface_steps > 1500 and absorptions > 100, (steps, surface_steps, absorptions)


# -- 3, 4. the two laws ------------------------------------------------------------------------------------------------------
N_LAW = 20_000


def law_scene():
    """An n = 1 hexagonal plate in an n = 1 world: every ray goes straight through, and what is counted is geometry alone."""
    world = air(20.0)
    plate = solid("hexagon", refractive_index=1.0)
    node = Node(name="plate", parent=world, geometry=plate)
    node.recorders = [Recorder(f"face-{k}", event="escaping", facet=plate.facet_normal(k)) for k in range(len(plate.planes))]
    node.recorders.append(Recorder("all", event="escaping"))
    return Scene(world), plate


def z_binomial(k, n, p):
    return (k - n * p) / math.sqrt(n * p * (1.0 - p))


def test_solid_angle_partition_over_the_faces_from_recorders_and_from_the_log():
    scene, plate = law_scene()
    assert plate.contains(C.LAW_SOURCE)
    shares = C.solid_angle_fractions(plate, C.LAW_SOURCE)
    assert len(shares) == 8 and abs(sum(shares) - 1.0) < 1e-12 and min(shares) > 0.01
    pos, dirs = C.point_source_rays(N_LAW)
    data, variant = trace(scene, pos, dirs, max_events=4)
    assert variant == "rough"
    names = [r.name for r in compile_scene(scene).recorder_specs]
    tally = {name: int(data["rec_distinct"][i]) for i, name in enumerate(names)}
    assert tally["all"] == N_LAW
    first = data["position"][np.arange(N_LAW) * 4 + 1]
    where = np.argmin(np.abs(first @ plate.planes[:, :3].T - plate.planes[:, 3]), axis=1)
    from_log = [int(np.sum(where == k)) for k in range(8)]
    from_tally = [tally[f"face-{k}"] for k in range(8)]
    assert from_log == from_tally and sum(from_tally) == N_LAW
    for k, (count, p) in enumerate(zip(from_tally, shares)):
        z = z_binomial(count, N_LAW, p)
        print(f"face {k}: {count} of {N_LAW}, expected {N_LAW * p:.1f}, z = {z:+.2f}")
        assert abs(z) <= 4.0, (k, count, z)
    tallies_only, _ = trace(scene, pos, dirs, record_every=0)
    assert np.array_equal(tallies_only["rec_distinct"], data["rec_distinct"])


def test_mean_chord_from_the_log():
    scene, plate = law_scene()
    assert plate.bounding_radius < 2.0
    pos, dirs = C.chord_rays(N_LAW)
    data, _ = trace(scene, pos, dirs, max_events=4)
    counts = data["counts"]
    assert set(np.unique(counts).tolist()) <= {2, 4}
    through = np.flatnonzero(counts == 4)
    p_in, p_out = data["position"][through * 4 + 1], data["position"][through * 4 + 2]
    chords = np.sqrt(np.sum((p_out - p_in) ** 2, axis=1))
    expected = 4.0 * plate.volume / plate.surface_area
    z = (chords.mean() - expected) / (chords.std(ddof=1) / math.sqrt(len(chords)))
    print(f"{len(chords)} chords, mean {chords.mean():.5f}, 4V/S = {expected:.5f}, z = {z:+.2f}")
    assert len(chords) > 2000 and abs(z) <= 4.0, z
    names = [r.name for r in compile_scene(scene).recorder_specs]
    assert int(data["rec_distinct"][names.index("all")]) == len(chords)   # (every chord ends in one escape)


# -- 5, 6. launch shapes ---------------------------------------------------------------------------------------------------
STEPS, ROWS = 50, 2 * 50 + 8   # a step writes at most two rows; GENERATE and the closing row come on top


def guide_scene(extra_recorders=0, mesh=False):
    """A dyed hexagonal PMMA plate under a lamp, in air; optionally with many recorders, or beside a mesh."""
    world = air(20.0)
    plate = solid("hexagon", refractive_index=1.5, components=[dye(), Absorber(0.05, name="host")])
    top, bottom, side = plate.facet_normal(7), plate.facet_normal(6), plate.facet_normal(2)
    assert top == (0.0, 0.0, 1.0) and bottom == (0.0, 0.0, -1.0)
    recorders = [Recorder("top", event="escaping", facet=top), Recorder("side", event="escaping", facet=side),
                 Recorder("escaping", event="escaping"), Recorder("entering", event="entering"), Recorder("lost", event="lost")]
    recorders += [Recorder(f"more-{i}", event="escaping", facet=side if i % 2 else top) for i in range(extra_recorders)]
    node = Node(name="plate", parent=world, recorders=recorders, geometry=plate)
    node.location = (0.0, 0.2, 0.0)   # (unrotated: a recorder's facet is matched in the root's frame)
    if mesh:
        gem = Node(name="gem", parent=world, geometry=Mesh.icosphere(1, 0.6, material=Material(refractive_index=1.6)))
        gem.location = (2.5, 0.0, 0.0)
    light = Node(name="Light", parent=world, light=Light(direction=functools.partial(cone, np.radians(25)), name="Light"))
    light.location = (0.3, 0.0, -2.0)
    return Scene(world)


def test_tally_history_device_emission_wide_recorder_and_carried_launches_agree():
    scene = guide_scene()
    n = 4096
    with Session(scene, emission="device") as s:
        assert s.emission == "device"
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
    wide, variant = trace(guide_scene(extra_recorders=70), *rays, seed=13, record_every=0, maxsteps=STEPS)   # (> 64 recorders: the wide seen-mask kernels)
    assert variant == "rough"
    assert np.array_equal(wide["rec_distinct"][:5], device["rec_distinct"])
    assert np.array_equal(wide["rec_distinct"][5:7], device["rec_distinct"][[0, 1]])
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


def test_a_ray_alone_plus_the_rest_equals_the_whole_launch():
    scene = guide_scene()
    n, alone = 2048, 700
    from pvtrace_amd.engine.emit import emit_bundle

    pos, dirs, wl, _ = emit_bundle(scene, n, seed=6)
    with Session(scene, emission="host") as s:
        def submit(lo, hi, record_every, **kw):
            r = s.collect(s.submit(hi - lo, 29, record_every=record_every, maxsteps=STEPS, ray_offset=lo,
                                   host_rays=(pos[lo:hi].copy(), dirs[lo:hi].copy(), wl[lo:hi].copy(), ["r"] * (hi - lo)), **kw))
            return {k: np.asarray(r.data[k]).copy() for k in TALLY_KEYS + (LOG_KEYS if record_every else ())}

        whole = submit(0, n, 1, max_events=ROWS)
        one = submit(alone, alone + 1, 1, max_events=ROWS)     # a launch of one ray: traced by the tail function
        k = int(whole["counts"][alone])
        assert int(one["counts"][0]) == k > 2
        for key in LOG_KEYS[1:]:
            assert np.array_equal(one[key][:k], whole[key][alone * ROWS:alone * ROWS + k], equal_nan=True), key
        parts = [submit(0, alone, 0), submit(alone, alone + 1, 0), submit(alone + 1, n, 0)]
        for key in TALLY_KEYS:
            assert np.array_equal(sum(p[key] for p in parts), whole[key]), key
        assert whole["rec_distinct"].min() > 0


# -- 7, 8, 9. beside a mesh, as the root, off its origin -----------------------------------------------------------------
def test_a_mesh_beside_a_polyhedron():
    world = air()
    wedge = solid("wedge", refractive_index=1.5)
    Node(name="solid", parent=world, geometry=wedge)
    gem = Node(name="gem", parent=world, geometry=Mesh.icosphere(1, 0.8, material=Material(refractive_index=1.6)))
    gem.location = (0.0, 12.0, 0.0)   # (beyond the reach of the families' rays before they meet the wedge)
    scene = Scene(world)
    assert compile_scene(scene).has_polyhedron and compile_scene(scene).n_mesh_faces > 0
    assert check_first_events(scene, wedge, [C.rays("wedge", f) for f in ("outside", "inside", "edges")]) > 500
    lit = guide_scene(mesh=True)
    from pvtrace_amd.engine.emit import emit_bundle

    pos, dirs, wl, _ = emit_bundle(lit, 4096, seed=2)
    pos[::2] = (2.5, 0.0, -4.0)   # (every other ray from below the gem)
    a, variant = trace(lit, pos, dirs, wl, seed=5, record_every=0, maxsteps=STEPS)
    b, _ = trace(lit, pos, dirs, wl, seed=5, record_every=1, max_events=ROWS, maxsteps=STEPS)
    assert variant == "rough"
    for k in TALLY_KEYS:
        assert np.array_equal(a[k], b[k]), k
    gem_id = list(compile_scene(lit).node_names).index("gem")
    assert np.any(b["hit"] == gem_id) and a["rec_distinct"].min() > 0


def test_a_polyhedron_as_the_root():
    room = Polyhedron.regular_prism(6, 10.0, 8.0, material=Material(refractive_index=1.0))
    world = Node(name="world", geometry=room, recorders=[Recorder("exit", event="exit")])
    Node(name="block", parent=world, geometry=Box((1.0, 1.0, 1.0), material=Material(refractive_index=1.5, components=[dye()])),
         recorders=[Recorder("in", event="entering"), Recorder("out", event="escaping")])
    scene = Scene(world)
    rng = np.random.default_rng(12)
    n = 2048
    pos = np.column_stack((rng.uniform(-0.6, 0.6, n), rng.uniform(-0.6, 0.6, n), np.full(n, -3.0)))
    dirs = C._unit(np.column_stack((rng.normal(0.0, 0.2, n), rng.normal(0.0, 0.2, n), np.ones(n))))
    hist, variant = trace(scene, pos, dirs, 480.0, seed=5, max_events=ROWS, maxsteps=STEPS)
    tally, _ = trace(scene, pos, dirs, 480.0, seed=5, record_every=0, maxsteps=STEPS)
    assert variant == "rough"
    for k in TALLY_KEYS:
        assert np.array_equal(hist[k], tally[k]), k
    last = np.arange(n) * ROWS + hist["counts"] - 1
    exits = last[hist["kind"][last] == EXIT]
    assert len(exits) > 0.9 * n and int(hist["rec_distinct"][0]) == len(exits)
    assert np.all(hist["hit"][exits] == 0)
    residual = np.abs(hist["position"][exits] @ room.planes[:, :3].T - room.planes[:, 3]).min(axis=1)
    assert residual.max() < 1e-12      # every ray leaves the scene ON a face of the root
    missed = np.flatnonzero(hist["counts"] == 2)    # GENERATE, EXIT: straight out, at the host class's distance
    assert len(missed) > 50
    for i in missed[:50]:
        (t,) = room._ray_distances(pos[i], dirs[i])
        assert np.array_equal(hist["position"][i * ROWS + 1], pos[i] + dirs[i] * t)


def test_a_polyhedron_that_does_not_contain_its_nodes_origin():
    shift = np.array([3.0, -2.0, 1.5])
    rows = C.shape("pyramid").planes.copy()
    rows[:, 3] += rows[:, :3] @ shift
    for pose in sorted(C.POSES):
        world = air()
        away = Polyhedron(rows, material=Material(refractive_index=1.5))
        assert not away.contains((0.0, 0.0, 0.0)) and away.contains(shift) and away.bounding_radius > 4.0
        posed(Node(name="solid", parent=world, geometry=away), C.POSES[pose])
        sets = [(o + shift, d) for o, d in (C.rays("pyramid", f) for f in ("outside", "inside", "vertices"))]
        assert check_first_events(Scene(world), away, sets) > 500


# -- 10. one face mirrored, another a cell -------------------------------------------------------------------------------------
def test_a_side_face_mirror_reflects_there_only_and_a_detected_recorder_counts_its_rows():
    world = air()
    plate = solid("hexagon", refractive_index=1.0)
    mirror_face, cell_face = 1, 4
    plate.material.surface = Surface(CoatedSurfaceDelegate([
        Coating(plate.facet_normal(mirror_face), reflectivity=1.0),
        Coating(plate.facet_normal(cell_face), reflectivity=0.0, absorptivity=1.0, transmission="matched")]))
    Node(name="solid", parent=world, geometry=plate,
         recorders=[Recorder("cell", event="detected", facet=plate.facet_normal(cell_face)), Recorder("any", event="detected")])
    scene = Scene(world)
    o = np.vstack([C.rays("hexagon", f)[0] for f in ("outside", "inside", "edges")])
    d = np.vstack([C.rays("hexagon", f)[1] for f in ("outside", "inside", "edges")])
    data, variant = trace(scene, o, d, max_events=8)
    assert variant == "rough"
    row1 = np.arange(len(o)) * 8 + 1
    kind, normal = data["kind"][row1], data["normal"][row1]
    on_solid = data["hit"][row1] == 1
    face = np.full(len(o), -1)
    for k in range(8):
        face[on_solid & np.all(normal == np.array(plate.facet_normal(k)), axis=1)] = k
    assert np.all(face[on_solid] >= 0)          # every logged normal is a stored row, bit for bit
    for k in range(8):
        assert np.sum(face == k) > 20, k
    assert np.all(kind[face == mirror_face] == REFLECT)
    assert np.all(kind[face == cell_face] == DETECT)
    others = on_solid & (face != mirror_face) & (face != cell_face)
    assert np.all(kind[others] == TRANSMIT)     # an n = 1 surface in an n = 1 world anywhere else: none is reflected
    detect_rows = data["kind"] == DETECT
    assert np.all(np.all(data["normal"][detect_rows] == np.array(plate.facet_normal(cell_face)), axis=1))
    assert int(data["rec_distinct"][0]) == int(data["rec_distinct"][1]) == int(np.sum(detect_rows)) > 50


# -- 11. shards, and the host-buffer entry -------------------------------------------------------------------------------------
def test_two_shards_on_one_gpu_equal_one_launch_and_the_host_buffer_entry_refuses():
    scene = guide_scene()
    n = 4096
    sharded = simulate(scene, n, seed=4, record_every=0, emission="device", emit_seed=8, devices=[0, 0])
    whole = simulate(scene, n, seed=4, record_every=0, emission="device", emit_seed=8)
    for k in TALLY_KEYS:
        assert np.array_equal(np.asarray(sharded.data[k]), np.asarray(whole.data[k])), k
    assert np.asarray(whole.data["rec_distinct"]).min() > 0
    from pvtrace_amd.engine.emit import emit_bundle

    pos, dirs, wl, _ = emit_bundle(scene, 16, seed=6)
    with pytest.raises(UnsupportedSceneError, match="convex polyhedron"):
        _kernel.trace_bundle(compile_scene(scene), pos, dirs, wl, 4, 100, 16, 0, 1, 1)


# -- 12. the entries ---------------------------------------------------------------------------------------------------------
def _create(compiled, entry, mutate=None, drop_polyhedra=False):
    """Call a creation entry with the scene's own structs -> (return code, message, whether a scene came back)."""
    lib = native.load_library()
    st, keep = native.scene_tables_struct(compiled)
    count = dict(native.CREATION_ENTRIES, **dict([native.NEWEST_ENTRY]))[entry]
    made = [native.marshal(t, compiled) for t in native.EXTENSION_TABLES[:count]]
    if mutate is not None:
        mutate(made[-1][1], made[-1][0], keep)
    if drop_polyhedra:
        made[-1] = (None, {})
    handle = ctypes.c_void_p()
    rc = getattr(lib, entry)(ctypes.byref(st), *[None if m is None else ctypes.byref(m) for m, _ in made], 0, ctypes.byref(handle))
    message = (lib.pvt_last_error() or b"").decode() if rc != 0 else ""
    came_back = bool(handle.value)
    if rc == 0:
        lib.pvt_scene_destroy(handle)
    del keep
    return rc, message, came_back


def test_older_entries_refuse_the_type_and_malformed_tables_are_refused_each_with_its_own_message(monkeypatch):
    assert native.NEWEST_ENTRY[0] not in native.CREATION_ENTRIES and len(native.CREATION_ENTRIES) == 11
    fresh = lambda: compile_scene(guide_scene())     # noqa: E731  (the structs point INTO the lowered tables)
    for entry in native.CREATION_ENTRIES:
        assert _create(fresh(), entry) == (-1, "unknown geometry type", False), entry
    assert _create(fresh(), native.NEWEST_ENTRY[0]) == (0, "", True)
    assert native.load_library().pvt_abi_version() == 13

    def put(field, index, value):
        def mutate(keep, struct, scene_keep):
            keep[field].reshape(-1)[index] = value
        return mutate

    def radius(value):
        def mutate(keep, struct, scene_keep):
            scene_keep["geom_params"].reshape(-1, 4)[1, 0] = value
        return mutate

    def other_node_count(keep, struct, scene_keep):
        struct.n_nodes = 1

    cases = [
        (put("node_plane_count", 1, 3), "a node needs 4 to 64 planes"),
        (put("node_plane_count", 1, 65), "a node needs 4 to 64 planes"),
        (put("node_plane_start", 1, 1), "plane range outside the pool"),
        (put("node_plane_start", 1, -1), "plane range outside the pool"),
        (put("planes", 7, math.nan), "plane rows must be finite"),
        (put("planes", 4, math.inf), "plane rows must be finite"),
        (put("planes", 8, 0.5), "unit vector within 1e-12"),
        (put("planes", 0, -0.5 * (1.0 + 1e-9)), "unit vector within 1e-12"),
        (radius(0.0), "bounding radius must be finite and > 0"),
        (radius(math.nan), "bounding radius must be finite and > 0"),
        (radius(math.inf), "bounding radius must be finite and > 0"),
        (other_node_count, "need one run of planes per node"),
    ]
    for mutate, text in cases:
        rc, message, came_back = _create(fresh(), native.NEWEST_ENTRY[0], mutate)
        assert rc == -1 and text in message and not came_back, (text, rc, message)
    assert len({text for _, text in cases}) == 6
    rc, message, came_back = _create(fresh(), native.NEWEST_ENTRY[0], drop_polyhedra=True)
    assert (rc, message, came_back) == (-1, "polyhedron node without polyhedron tables", False)
    # a scene without the shape: the new entry, handed NULL for the struct, builds what pvt_scene_create_aligned builds
    plain = guide_scene()
    plain.root.children[0].geometry = Box((1.6, 1.6, 0.4), material=plain.root.children[0].geometry.material)
    assert not compile_scene(plain).has_polyhedron
    assert native.marshal(native.PvtPolyhedronTables, compile_scene(plain)) == (None, {})
    from pvtrace_amd.engine.emit import emit_bundle

    pos, dirs, wl, _ = emit_bundle(plain, 2048, seed=6)
    new, _ = trace(plain, pos, dirs, wl, seed=4, max_events=32, maxsteps=STEPS)
    from pvtrace_amd.engine import api

    api.release_resident_scenes()      # (or the scene just made would be handed out again)
    lib, reached = native.load_library(), []
    real = lib.pvt_scene_create_aligned
    monkeypatch.setattr(lib, "pvt_scene_create_aligned", lambda *a: reached.append(len(a)) or real(*a))
    monkeypatch.setattr(native, "NEWEST_ENTRY", ("pvt_scene_create_aligned", 9))
    old, _ = trace(plain, pos, dirs, wl, seed=4, max_events=32, maxsteps=STEPS)
    api.release_resident_scenes()
    assert reached == [12]
    for k in TALLY_KEYS + LOG_KEYS:
        assert np.array_equal(new[k], old[k], equal_nan=True), k
    assert new["rec_distinct"][[0, 2, 3, 4]].min() > 0      # (no face of the box has the hexagon's side normal)


# -- 13. the example -------------------------------------------------------------------------------------------------------------
def test_the_hexagonal_lsc_example_runs():
    spec = importlib.util.spec_from_file_location("hexagonal_lsc", os.path.join(ROOT, "examples", "hexagonal_lsc.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    rows = module.main(photons=20_000)
    assert rows["square"]["edges"] == 4 and rows["hexagon"]["edges"] == 6
    assert rows["square"]["area"] == pytest.approx(25.0, rel=1e-12) and rows["hexagon"]["area"] == pytest.approx(25.0, rel=1e-12)
    for row in rows.values():
        assert 0.2 < row["collected"] < 0.9 and min(row["per_edge"]) > 100
        assert row["entered"] > 15_000
    assert abs(rows["square"]["collected"] - rows["hexagon"]["collected"]) < 0.1
