"""Truncated cones (`pvtrace_amd.Frustum`, PVT_GEOM_FRUSTUM) on the GPU.  The oracle does not know the shape; the engine is
held to the host class bit for bit (itself held to an exact rational reference, tests/test_frustum.py), to the cylinder
it becomes with equal radii, to the host tracer's geometry step by step, to two closed-form laws, and to itself across
launch shapes.

1. The first surface event of every ray of tests/frustum_cases.py's families -- logged position and normal -- is what
   the host class gives, `np.array_equal`, in the node's own frame and through a rotated and translated node (the host
   applies the node's matrices in the kernel's operation order).  Ambiguous rays (tests/frustum_cases.py) are set aside,
   at most 2 % of a family.
2. `Frustum(L, r, r)` traces 20 000 photons exactly as `Cylinder(L, r)`: full event logs and tallies, the one on the
   extension family's kernels, the other on the plain family's.
3. Host-tracer parity.  The host tracer draws from numpy's generator and the engine from its per-ray stream, so the two
   cannot take the same random decisions and whole histories cannot be compared row for row.  What is compared is every
   STEP of every engine history: from the logged ray before it, the host tracer's own interface search
   (`photon_tracer._interface_ahead`: `Scene.intersections` over the host classes) must name the node the engine hit and
   the container it was in, its distance must carry the ray to the engine's next position, and the host normal there must
   be the logged one (directions after a reflection or refraction are checked only indirectly: the logged ray of one row
   is the start ray of the next step's search, so a wrong direction shows as a wrong next node, position or normal; the
   search is the tracer's own `_interface_ahead`, private but the one function `follow` steps with) -- positions and normals within 1e-12 absolute, the tolerance tests/test_gpu_coating_tables.py uses
   for engine-against-host-tracer rows (the engine accumulates positions in the root's frame, the host tracer converts
   frames per step, so bit equality is not demanded there either); an absorption must lie before that interface.
4. The solid-angle partition and the mean chord of tests/test_frustum.py at 20 000 rays, from recorders and from the log,
   within 4 standard errors; observed on an MI355X: z = +0.15 (top cap), +0.21 (bottom cap), -0.28 (side); 5155 chords,
   z = +0.37.
5. Launch shapes: tally against history launches, device against host emission, more than 64 recorders, a mesh beside a
   truncated cone, a 3 x 3 array with and without PVT_NO_GRID, the host-buffer entry, two shards on one GPU; the
   `pvt_scene_create*` entries from before the shape refuse it as they did.
6. A mirror coating on the top cap reflects every ray that reaches that cap and none that reaches the side.
"""
import functools
import math

import numpy as np
import pytest
import torch

from pvtrace_amd import (
    Absorber, Box, CoatedSurfaceDelegate, Coating, Cylinder, Frustum, Light, Luminophore, Material, Mesh, Node, Ray, Scene,
    Sphere, Surface, cone,
)
from pvtrace_amd.algorithm import photon_tracer
from pvtrace_amd.data import lumogen_f_red_305
from pvtrace_amd.engine import Recorder, Session, _kernel, compile_scene, native, simulate
from pvtrace_amd.engine.emit import emit_bundle
from tests import frustum_cases as C
from tests.test_frustum import taper_array

pytestmark = pytest.mark.gpu

GENERATE, REFLECT, TRANSMIT, ABSORB, EXIT = 0, 1, 2, 3, 7
TALLY_KEYS = ("rec_distinct", "rec_crossings", "rec_bins")
LOG_KEYS = ("counts", "kind", "hit", "container", "adjacent", "position", "direction", "normal", "wavelength", "travelled",
            "duration")
X = np.arange(400, 800)


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


def check_first_events(scene, shape, families, node_name="taper"):
    """Every family's rays, given in the node's frame, sent through `scene` in its world: the first surface event on the
    node against the host class.  -> rays judged."""
    compiled = compile_scene(scene)
    node = list(compiled.node_names).index(node_name)
    l2w, w2l = compiled.local_to_world[node], compiled.world_to_local[node]
    frustum = Frustum(*C.SHAPES[shape])
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
    position, normal = data["position"][row1], data["normal"][row1]
    judged = 0
    for f, family in enumerate(families):
        ambiguous = 0
        for i in range(f * C.N_RAYS, (f + 1) * C.N_RAYS):
            ol, dl = C.to_local(w2l, pos[i], dirs[i])   # the node's frame as the kernel reaches it
            if C.exact_crossings(C.SHAPES[shape], ol, dl)[1]:
                ambiguous += 1
                continue
            ts = frustum._ray_distances(ol, dl)
            if not ts:
                assert hit[i] != node, (shape, family, i)
                continue
            t = min(ts)
            assert hit[i] == node and kind[i] in (REFLECT, TRANSMIT), (shape, family, i, kind[i], hit[i])
            want = pos[i] + dirs[i] * t
            assert np.array_equal(position[i], want), (shape, family, i, position[i], want)
            n_local = frustum.normal(C.to_local(w2l, want, dirs[i])[0])
            assert np.array_equal(normal[i], C.rotate(l2w[:3, :3], n_local)), (shape, family, i, normal[i], n_local)
            judged += 1
        assert ambiguous <= C.MAX_AMBIGUOUS * C.N_RAYS, (shape, family, ambiguous)
    return judged


@pytest.mark.parametrize("pose", sorted(C.POSES))
@pytest.mark.parametrize("shape", sorted(C.SHAPES))
def test_first_surface_event_is_the_host_class_bit_for_bit(shape, pose):
    world = air()
    posed(Node(name="taper", parent=world, geometry=Frustum(*C.SHAPES[shape], material=Material(refractive_index=1.5))),
          C.POSES[pose])
    assert check_first_events(Scene(world), shape, C.families_of(shape)) > 1000


# -- 2. cylinder anchor ------------------------------------------------------------------------------------------------------
def rod_scene(make):
    """tests/scenes.py nested_cylinders reduced to its inner shape: a rotated PMMA rod with a dye, a 30-degree cone below it."""
    world = air(10.0)
    rod = Node(name="A", parent=world, geometry=make(material=Material(refractive_index=1.5, components=[dye()])),
               recorders=[Recorder("A-escaping", event="escaping"), Recorder("A-entering", event="entering"),
                          Recorder("A-top", event="escaping", facet=(0.0, 0.0, 1.0)), Recorder("A-lost", event="lost")])
    rod.translate((0, 0, 2))
    rod.rotate(np.pi * 0.2, (0, 1, 0))
    world.recorders = [Recorder("exit", event="exit")]
    light = Node(name="Light", parent=world, light=Light(direction=functools.partial(cone, np.radians(30)), name="Light"))
    light.translate((0, 0, -1))
    return Scene(world)


def test_equal_radii_trace_as_the_cylinder_event_for_event():
    cylinder = rod_scene(functools.partial(Cylinder, 2.0, 0.4))
    frustum = rod_scene(functools.partial(Frustum, 2.0, 0.4, 0.4))
    n = 20_000
    pos, dirs, wl, _ = emit_bundle(cylinder, n, seed=5)
    a, va = trace(cylinder, pos, dirs, wl, seed=11, max_events=48, maxsteps=200)
    b, vb = trace(frustum, pos, dirs, wl, seed=11, max_events=48, maxsteps=200)
    assert va != "rough" and vb == "rough"
    for k in TALLY_KEYS + LOG_KEYS:
        assert np.array_equal(a[k], b[k]), k
    assert np.median(a["counts"]) < 48 and np.any(a["kind"] == ABSORB) and np.any(a["kind"] == REFLECT)   # (trapped light fills a log)
    assert a["rec_distinct"][:3].min() > 0   # (exit, A-escaping, A-entering)


# -- 3. the host tracer's geometry, step by step -------------------------------------------------------------------------
def nested_scene():
    world = Node(name="world", geometry=Box((40.0, 40.0, 40.0), material=Material(refractive_index=1.0)))
    block = Node(name="block", parent=world, geometry=Box((4.0, 4.0, 5.0), material=Material(refractive_index=1.2)))
    taper = Node(name="taper", parent=block,
                 geometry=Frustum(3.0, 1.2, 0.5, material=Material(refractive_index=1.5, components=[dye()])))
    taper.rotate(0.3, (1.0, 1.0, 0.0))
    bead = Node(name="bead", parent=taper, geometry=Sphere(0.25, material=Material(refractive_index=1.8)))
    bead.location = (0.1, 0.0, -0.3)
    return Scene(world)


def test_every_step_of_an_engine_history_is_a_step_of_the_host_tracers_geometry():
    scene = nested_scene()
    nodes = {n.name: n for n in [scene.root] + list(scene.root.children) + list(scene.root.children[0].children)
             + list(scene.root.children[0].children[0].children)}
    rng = np.random.default_rng(8)
    n, me = 512, 64
    pos = np.column_stack((rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n), np.full(n, -8.0)))
    dirs = C._unit(np.column_stack((rng.normal(0.0, 0.15, n), rng.normal(0.0, 0.15, n), np.ones(n))))
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
    assert nodes.keys() >= seen >= {"block", "taper", "bead"}
    assert steps > 2000 and surface_steps > 1500 and absorptions > 100, (steps, surface_steps, absorptions)


# -- 4. the two laws -----------------------------------------------------------------------------------------------------------
N_LAW = 20_000


def z_binomial(k, n, p):
    return (k - n * p) / math.sqrt(n * p * (1.0 - p))


def test_solid_angle_partition_from_recorders_and_from_the_log():
    scene = C.law_scene(recorders=True)
    pos, dirs = C.point_source_rays(N_LAW)
    data, variant = trace(scene, pos, dirs, max_events=4)
    assert variant == "rough"
    names = [r.name for r in compile_scene(scene).recorder_specs]
    tally = {name: int(data["rec_distinct"][i]) for i, name in enumerate(names)}
    assert tally["all"] == N_LAW
    where = C.which_surface(data["position"][np.arange(N_LAW) * 4 + 1])
    from_log = [int(np.sum(where == j)) for j in range(3)]
    from_tally = [tally["top"], tally["bottom"], tally["all"] - tally["top"] - tally["bottom"]]
    assert from_log == from_tally
    for name, k, p in zip(("top", "bottom", "side"), from_tally, C.partition_probabilities()):
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
    assert len(chords) > 4000 and abs(z) <= 4.0, z
    names = [r.name for r in compile_scene(scene).recorder_specs]
    assert int(data["rec_distinct"][names.index("all")]) == len(chords)   # (every chord ends in one escape)


# -- 5. launch shapes --------------------------------------------------------------------------------------------------------
STEPS, ROWS = 50, 2 * 50 + 8   # a step writes at most two rows; GENERATE and the closing row come on top


def guide_scene(extra_recorders=0, mesh=False):
    """A dyed PMMA taper under a lamp, in air; optionally with many recorders, or beside a mesh."""
    world = air(20.0)
    recorders = [Recorder("top", event="escaping", facet=(0.0, 0.0, 1.0)), Recorder("bottom", event="escaping", facet=(0.0, 0.0, -1.0)),
                 Recorder("escaping", event="escaping"), Recorder("entering", event="entering"), Recorder("lost", event="lost")]
    recorders += [Recorder(f"more-{i}", event="escaping", facet=(0.0, 0.0, 1.0 if i % 2 else -1.0)) for i in range(extra_recorders)]
    taper = Node(name="taper", parent=world, recorders=recorders,
                 geometry=Frustum(2.0, 1.0, 0.4, material=Material(refractive_index=1.5, components=[dye(), Absorber(0.05, name="host")])))
    taper.location = (0.0, 0.2, 0.0)   # (unrotated: a recorder's facet is matched in the root's frame)
    if mesh:
        gem = Node(name="gem", parent=world, geometry=Mesh.icosphere(1, 0.6, material=Material(refractive_index=1.6)))
        gem.location = (2.5, 0.0, 0.0)
    light = Node(name="Light", parent=world, light=Light(direction=functools.partial(cone, np.radians(25)), name="Light"))
    light.location = (0.3, 0.0, -4.0)
    return Scene(world)


def test_tally_history_device_emission_and_wide_recorder_launches_agree():
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
    wide, variant = trace(guide_scene(extra_recorders=70), *rays, seed=13, record_every=0, maxsteps=STEPS)   # (> 64 recorders: the wide seen-mask kernels)
    assert variant == "rough"
    assert np.array_equal(wide["rec_distinct"][:5], device["rec_distinct"])
    assert np.array_equal(wide["rec_distinct"][5:7], device["rec_distinct"][[1, 0]])


def test_a_mesh_beside_a_truncated_cone():
    world = air()
    Node(name="taper", parent=world, geometry=Frustum(*C.SHAPES["taper"], material=Material(refractive_index=1.5)))
    gem = Node(name="gem", parent=world, geometry=Mesh.icosphere(1, 0.8, material=Material(refractive_index=1.6)))
    gem.location = (0.0, 12.0, 0.0)   # (beyond the reach of the families' rays before they meet the taper)
    scene = Scene(world)
    assert compile_scene(scene).has_frustum and compile_scene(scene).n_mesh_faces > 0
    assert check_first_events(scene, "taper", ["outside", "inside", "slant"]) > 500
    lit = guide_scene(mesh=True)
    pos, dirs, wl, _ = emit_bundle(lit, 4096, seed=2)
    pos[::2] = (2.5, 0.0, -4.0)   # (every other ray from below the gem)
    a, variant = trace(lit, pos, dirs, wl, seed=5, record_every=0, maxsteps=STEPS)
    b, _ = trace(lit, pos, dirs, wl, seed=5, record_every=1, max_events=ROWS, maxsteps=STEPS)
    assert variant == "rough"
    for k in TALLY_KEYS:
        assert np.array_equal(a[k], b[k]), k
    gem_id = list(compile_scene(lit).node_names).index("gem")
    assert np.any(b["hit"] == gem_id) and a["rec_distinct"].min() > 0


def test_an_array_of_tapers_with_and_without_the_grid_switch(monkeypatch):
    scene = taper_array()
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
    assert np.array_equal(out[0], out[1]) and out[0].sum() > 0


def test_the_host_buffer_entry_and_two_shards_on_one_gpu():
    scene = guide_scene()
    compiled = compile_scene(scene)
    n = 4096
    pos, dirs, wl, _ = emit_bundle(scene, n, seed=6)
    want, _ = trace(scene, pos, dirs, wl, seed=4, max_events=32, maxsteps=1000)
    args = (pos, dirs, wl, 4, 1000, 32, 0, 1, 1)
    for kw in ({}, {"devices": [0, 0]}):
        got = _kernel.trace_bundle(compiled, *args, **kw)
        for k in TALLY_KEYS + ("counts", "kind", "position", "direction", "normal"):
            assert np.array_equal(np.asarray(got[k]), want[k]), (k, kw)
    sharded = simulate(scene, n, seed=4, record_every=0, emission="device", emit_seed=8, devices=[0, 0])
    whole = simulate(scene, n, seed=4, record_every=0, emission="device", emit_seed=8)
    for k in TALLY_KEYS:
        assert np.array_equal(np.asarray(sharded.data[k]), np.asarray(whole.data[k])), k


def test_the_entries_from_before_the_shape_refuse_it_as_they_did():
    """Geometry type 4 was "unknown geometry type" to every `pvt_scene_create*` entry; it still is to all of them but
    `pvt_scene_create_origin`, the one the Python layer calls (each entry knows a last geometry type, as it knows a last
    recorder selector and histogram property).  No scene comes back."""
    import ctypes as C_

    lib = native.load_library()
    st, keep = native.scene_tables_struct(compile_scene(guide_scene()))
    handle = C_.c_void_p()
    rc = lib.pvt_scene_create(C_.byref(st), 0, C_.byref(handle))
    assert (rc, lib.pvt_last_error().decode()) == (-1, "unknown geometry type") and not handle.value
    del keep


# -- 6. caps and side ------------------------------------------------------------------------------------------------------
def test_a_cap_mirror_reflects_at_the_cap_and_nowhere_else():
    world = air()
    mirror = Surface(CoatedSurfaceDelegate([Coating((0.0, 0.0, 1.0), reflectivity=1.0)]))
    Node(name="taper", parent=world, geometry=Frustum(*C.SHAPES["taper"], material=Material(refractive_index=1.0, surface=mirror)))
    scene = Scene(world)
    o = np.vstack([C.rays("taper", f)[0] for f in ("outside", "inside", "plane")])
    d = np.vstack([C.rays("taper", f)[1] for f in ("outside", "inside", "plane")])
    data, variant = trace(scene, o, d, max_events=4)
    assert variant == "rough"
    row1 = np.arange(len(o)) * 4 + 1
    kind, normal = data["kind"][row1], data["normal"][row1]
    on_taper = data["hit"][row1] == 1
    top = on_taper & (normal[:, 2] == 1.0) & (normal[:, 0] == 0.0) & (normal[:, 1] == 0.0)
    assert top.sum() > 30 and (on_taper & ~top).sum() > 300
    assert np.all(kind[top] == REFLECT)                 # the mirror: every ray that reaches the cap
    assert np.all(kind[on_taper & ~top] == TRANSMIT)    # an n = 1 surface in an n = 1 world anywhere else: none is reflected
