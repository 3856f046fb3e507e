"""Volume maps (`VolumeMap`) on the GPU.  The CPU referee knows no maps; the referee here is the event log: one launch
with `record_every=1` gives both the kernel's maps and every ray's history, and `map_histories` bins those histories on
the host by the same contract (include/pvtrace_hip.h, PvtMapTables).  The comparison is exact, slot for slot, `outside`
included: the contract fixes the order of every operation and the build has FMA contraction off.  Then the maps are held
to themselves (tally launches, carried launches, streams, a ray alone), to the recorders (conservation, the `lost`
recorder's crossings) and to the Beer-Lambert law."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from pvtrace_amd import (
    Absorber, Box, ConcentrationGrid, FresnelSurfaceDelegate, Luminophore, Material, Node, Reactor, Scatterer, Scene,
    Surface, VolumeMap,
)
from pvtrace_amd.engine import Recorder, Session, compile_scene, map_histories, native, simulate, simulate_stream, trace_stream
from pvtrace_amd.engine.api import maps_from_slots
from pvtrace_amd.engine.emit import emit_bundle
from pvtrace_amd.material import NullSurfaceDelegate
from tests import broken_tables as BT
from tests import laws as L
from tests import scenes
from tests.test_volume_maps import beer_lambert_probabilities, beer_lambert_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KILL = 9
SLAB_LO, SLAB_HI = (-2.5, -2.5, -0.5), (2.5, 2.5, 0.5)
HIST_KEYS = ("counts", "kind", "hit", "container", "component", "position", "direction", "wavelength", "duration")
TALLY_KEYS = ("rec_distinct", "rec_crossings", "rec_bins")   # (the integers: exact)
ALL_EVENTS = ("absorbed", "emitted", "scattered", "lost", "reacted")


def node(scene, name):
    return next(n for n in scene.root.preorder() if n.name == name)


def all_kinds(prefix, shape, lo, hi, **kw):
    return [VolumeMap(f"{prefix}{event}", shape, lo, hi, event=event, **kw) for event in ALL_EVENTS]


def same_maps(a, b):
    assert sorted(a) == sorted(b)
    for name in a:
        assert np.array_equal(a[name].counts, b[name].counts), name
        assert a[name].outside == b[name].outside, name


def pencil(start, direction, wavelength, n):
    return (np.tile(np.asarray(start, float), (n, 1)), np.tile(np.asarray(direction, float), (n, 1)),
            np.full(n, float(wavelength)))


def submit(session, rays, seed, **kw):
    pos, dirs, wl = rays
    return session.collect(session.submit(len(wl), seed, host_rays=(pos, dirs, wl, ["r"] * len(wl)), **kw))


def block(components, surface=None, angle=None, axis=None, location=None, size=(2.0, 2.0, 2.0), index=1.0):
    world = Node(name="world", geometry=Box((40.0, 40.0, 40.0), material=Material(refractive_index=1.0)))
    body = Node(name="block", parent=world, geometry=Box(size, material=Material(
        refractive_index=index, surface=Surface(NullSurfaceDelegate() if surface is None else surface),
        components=components)))
    if angle is not None:
        body.rotate(angle, axis)
    if location is not None:
        body.translate(location)
    return Scene(world), body


# -- 5. the kernel's maps against the event log, exactly ------------------------------------------------------------------
def lumogen_slab():
    scene = scenes.lsc_equivalent(recorders=False)
    wl = (400.0, 800.0, 16)
    node(scene, "LSC").volume_maps = [
        VolumeMap("absorbed", (8, 8, 4), SLAB_LO, SLAB_HI, wavelength=wl),
        VolumeMap("emitted", (8, 8, 4), SLAB_LO, SLAB_HI, event="emitted", wavelength=wl),
        VolumeMap("lost", (8, 8, 4), SLAB_LO, SLAB_HI, event="lost", wavelength=(500.0, 600.0, 5)),
    ]
    return scene, None


def rotated_roi():
    x = np.linspace(400.0, 800.0, 41)
    lum = Luminophore(np.column_stack([x, 1.5 * np.exp(-((x - 520.0) / 80.0) ** 2)]),
                      emission=np.column_stack([x, np.exp(-((x - 560.0) / 50.0) ** 2)]), quantum_yield=0.9, name="lum")
    scene, body = block([lum], angle=0.7, axis=(0.3, -1.0, 0.6), location=(1.5, -0.5, 0.25))
    body.volume_maps = all_kinds("roi-", (5, 4, 3), (-0.6, -0.5, -1.0), (0.4, 0.7, 0.1))   # smaller than the node
    R = L.rotation(0.7, (0.3, -1.0, 0.6))
    d = R @ np.array([0.1, 0.05, 1.0]) / np.linalg.norm([0.1, 0.05, 1.0])
    start = np.array([1.5, -0.5, 0.25]) + R @ np.array([0.05, 0.1, 0.0]) - 6.0 * d
    return scene, pencil(start, d, 500.0, 8192)


def two_components():
    scene = scenes.lsc_equivalent()
    slab = node(scene, "LSC")
    slab.volume_maps = [VolumeMap("dye", (6, 5, 2), SLAB_LO, SLAB_HI, component="Lumogen F Red 305"),
                        VolumeMap("background", (6, 5, 2), SLAB_LO, SLAB_HI, component="Background"),
                        VolumeMap("dye-emitted", (3, 3, 1), SLAB_LO, SLAB_HI, event="emitted", component="Lumogen F Red 305"),
                        VolumeMap("background-lost", (3, 3, 1), SLAB_LO, SLAB_HI, event="lost", component="Background"),
                        VolumeMap("dye-lost", (3, 3, 1), SLAB_LO, SLAB_HI, event="lost", component="Lumogen F Red 305")]
    return scene, None


def reactor():
    scene, body = block([Reactor(1.2, name="cat"), Absorber(0.4, name="ink")])
    body.volume_maps = all_kinds("", (3, 3, 7), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)) + [
        VolumeMap("cat-reacted", (1, 1, 4), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), event="reacted", component="cat")]
    return scene, pencil((0.2, -0.3, -5.0), (0.0, 0.0, 1.0), 555.0, 8192)


def scatterer():
    scene, body = block([Scatterer(2.0, quantum_yield=0.9, name="fog")])
    body.volume_maps = all_kinds("", (4, 4, 4), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), wavelength=(500.0, 600.0, 2))
    return scene, pencil((0.2, -0.3, -5.0), (0.0, 0.0, 1.0), 555.0, 8192)


def tiles():
    scene = scenes.tiles6()
    tiled = [n for n in scene.root.preorder() if n.geometry is not None and n is not scene.root]
    assert len(tiled) >= 8
    c = compile_scene(scene)
    near = sorted(tiled, key=lambda n: float(np.hypot(*c.local_to_world[c.nodes.index(n)][:2, 3])))[:2]   # under the lamp
    for k, n in enumerate(near):
        size = np.asarray(n.geometry._size, float)
        n.volume_maps = [VolumeMap(f"tile{k}-absorbed", (4, 4, 2), tuple(-0.5 * size), tuple(0.5 * size)),
                         VolumeMap(f"tile{k}-emitted", (2, 2, 1), tuple(-0.5 * size), tuple(0.5 * size), event="emitted")]
    return scene, None


def mesh():
    scene = scenes.mesh_lsc()
    slab = node(scene, "LSC")
    slab.recorders = [r for r in slab.recorders if r.name not in ALL_EVENTS]   # (the maps take the plain names)
    slab.volume_maps = all_kinds("", (5, 5, 2), SLAB_LO, SLAB_HI)
    return scene, None


def field_and_rough():
    ix, iy, iz = np.indices((3, 2, 4))
    grid = ConcentrationGrid(0.2 + ((ix + 2 * iy + iz) % 3), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    x = np.linspace(400.0, 800.0, 41)
    lum = Luminophore(np.column_stack([x, 1.5 * np.exp(-((x - 520.0) / 80.0) ** 2)]),
                      emission=np.column_stack([x, np.exp(-((x - 560.0) / 50.0) ** 2)]), quantum_yield=0.95,
                      concentration=grid, name="lum")
    scene, body = block([lum], surface=FresnelSurfaceDelegate(roughness=0.3), angle=0.5, axis=(1.0, 1.0, 0.0), index=1.5)
    body.volume_maps = [VolumeMap.like(grid, "dose", wavelength=(400.0, 800.0, 8)),
                        VolumeMap.like(grid, "glow", event="emitted"), VolumeMap.like(grid, "heat", event="lost")]
    R = L.rotation(0.5, (1.0, 1.0, 0.0))
    return scene, pencil(R @ np.array([0.2, -0.1, -4.0]), R @ np.array([0.0, 0.0, 1.0]), 480.0, 8192)


def device_emission():
    scene = scenes.lsc_equivalent(recorders=False)
    node(scene, "LSC").volume_maps = all_kinds("", (4, 4, 2), SLAB_LO, SLAB_HI)
    return scene, "device"


EXACT_SCENES = {"lumogen_slab": lumogen_slab, "rotated_roi": rotated_roi, "two_components": two_components,
                "reactor": reactor, "scatterer": scatterer, "node_grid": tiles, "mesh": mesh,
                "field_and_rough": field_and_rough, "device_emission": device_emission}


def history_launch(scene, rays, n=8192, seed=7, max_events=512):
    """ONE launch that keeps every ray's history -> (result, the same rays and seed tallied only)."""
    if isinstance(rays, str):   # device emission
        with Session(scene, emission="device") as s:
            hist = s.collect(s.submit(n, seed, record_every=1, max_events=max_events, emit_seed=31))
            tally = s.collect(s.submit(n, seed, record_every=0, emit_seed=31))
    else:
        if rays is None:
            pos, dirs, wl, _ = emit_bundle(scene, n, seed=3)
            rays = (pos, dirs, wl)
        with Session(scene, emission="host") as s:
            hist = submit(s, rays, seed, record_every=1, max_events=max_events)
            tally = submit(s, rays, seed, record_every=0)
    # no history was cut: neither by max_events nor by maxsteps
    assert int(np.asarray(hist.data["counts"]).max()) < max_events
    return hist, tally


@pytest.mark.parametrize("name", sorted(EXACT_SCENES))
def test_kernel_maps_equal_the_event_log_slot_for_slot(name):
    scene, rays = EXACT_SCENES[name]()
    hist, tally = history_launch(scene, rays)
    assert not any(int(k.value) == KILL for k in hist.event_counts())
    kernel = hist.volume_maps
    referee = map_histories(scene, hist.histories())
    assert sum(m.total for m in kernel.values()) > 0, "the scene absorbed nothing"
    same_maps(kernel, referee)
    same_maps(kernel, tally.volume_maps)        # 6. a tally-only launch of the same rays and seed
    if name == "rotated_roi":
        assert kernel["roi-absorbed"].outside > 0 and kernel["roi-absorbed"].counts.sum() > 0
    if name == "two_components":
        assert kernel["dye"].total > 0 and kernel["background"].total > 0 and kernel["dye-lost"].total == 0
        assert kernel["dye-emitted"].total == kernel["dye"].total      # quantum yield 1
        assert kernel["background-lost"].total == kernel["background"].total
    if name == "reactor":
        assert kernel["reacted"].total > 0 and kernel["cat-reacted"].total == kernel["reacted"].total
    if name == "scatterer":
        assert kernel["scattered"].total > 0 and kernel["lost"].total > 0 and kernel["emitted"].total == 0
    if name == "node_grid":
        assert compile_scene(scene).n_maps == 4 and all(kernel[f"tile{k}-absorbed"].total > 0 for k in (0, 1))
    # 7. conservation per node, in integers
    by_node = {}
    c = compile_scene(scene)
    for i, n in enumerate(c.node_names):
        specs = c.map_specs[c.node_map_start[i]: c.node_map_start[i] + c.node_map_count[i]]
        plain = {s.event: kernel[s.name].total for s in specs if s.component is None}
        if set(plain) == set(ALL_EVENTS):
            by_node[n] = plain
    for n, t in by_node.items():
        assert t["absorbed"] == t["emitted"] + t["scattered"] + t["lost"] + t["reacted"], (n, t)


# -- 6. the launch does not matter ----------------------------------------------------------------------------------------
def conservation_scene(shape=(8, 8, 4)):
    scene = scenes.lsc_equivalent()
    slab = node(scene, "LSC")
    slab.volume_maps = all_kinds("", shape, SLAB_LO, SLAB_HI)
    slab.recorders = [r for r in slab.recorders if r.name not in ALL_EVENTS] + [Recorder("lost-crossings", event="lost")]
    return scene


def test_carried_launches_streams_and_a_ray_alone_give_the_same_maps():
    scene = conservation_scene()
    n, seed, emit_seed = 1_000_000, 13, 21
    whole = simulate(scene, n, seed=seed, record_every=0, emission="device", emit_seed=emit_seed)
    maps = whole.volume_maps
    assert maps["absorbed"].total > n // 2
    # carried launches: three bundles on a pipeline whose launches hand their live photons on
    compiled, data, _ = trace_stream(scene, n, n // 3 + 1, seed, emit_seed=emit_seed, depth=1)
    same_maps(maps, maps_from_slots(compiled, data["map_bins"]))
    compiled, data, _ = trace_stream(scene, n, n // 3 + 1, seed, emit_seed=emit_seed, depth=2)
    same_maps(maps, maps_from_slots(compiled, data["map_bins"]))
    # a stream of bundles, one map set per bundle (tally sets of grouped launches), summed
    total, bundles = None, 0
    for result, _ in simulate_stream(scene, n, bundle=50_000, seed=seed, record_every=0, emission="device",
                                     emit_seed=emit_seed):
        part = np.asarray(result.data["map_bins"]).astype(np.int64)
        total = part.copy() if total is None else total + part
        bundles += 1
    assert bundles == 20
    same_maps(maps, maps_from_slots(whole.compiled, total))
    # a ray alone (a launch of one photon finishes in the tail function) and the rest around it
    with Session(scene, emission="device") as s:
        for i in (0, 123_457, n - 1):
            parts = [s.collect(s.submit(b - a, seed, record_every=0, emit_seed=emit_seed, ray_offset=a))
                     for a, b in ((0, i), (i, i + 1), (i + 1, n)) if b > a]
            total = sum(np.asarray(p.data["map_bins"]).astype(np.int64) for p in parts)
            same_maps(maps, maps_from_slots(whole.compiled, total))


# -- 7. conservation, and the tie to the recorders -------------------------------------------------------------------------
def assert_conserved(result):
    m = result.volume_maps
    assert m["absorbed"].total == m["emitted"].total + m["scattered"].total + m["lost"].total + m["reacted"].total
    assert m["absorbed"].total > 0 and m["lost"].total > 0 and m["emitted"].total > 0
    assert m["lost"].total == result.recorders["lost-crossings"].crossings
    assert all(v.outside == 0 for v in m.values())      # the maps cover the slab


def test_conservation_and_the_lost_recorder():
    result = simulate(conservation_scene(), 1_000_000, seed=5, record_every=0, emission="device", emit_seed=6)
    assert_conserved(result)


# -- 8. existing behaviour --------------------------------------------------------------------------------------------------
def test_a_map_changes_neither_recorders_nor_histories():
    plain, mapped = scenes.lsc_equivalent(), scenes.lsc_equivalent()
    node(mapped, "LSC").volume_maps = all_kinds("map-", (8, 8, 4), SLAB_LO, SLAB_HI)
    pos, dirs, wl, _ = emit_bundle(plain, 200_000, seed=3)
    out = []
    for scene in (plain, mapped):
        with Session(scene, emission="host") as s:
            h = submit(s, (pos[:20_000], dirs[:20_000], wl[:20_000]), 7, record_every=1, max_events=64)
            t = submit(s, (pos, dirs, wl), 7, record_every=0)
            out.append(({k: np.asarray(h.data[k]).copy() for k in HIST_KEYS + TALLY_KEYS},
                        {k: np.asarray(t.data[k]).copy() for k in TALLY_KEYS + ("rec_sums",)}))
    assert "map_bins" not in simulate(plain, 1000, seed=1, record_every=0).data
    for k in HIST_KEYS + TALLY_KEYS:
        assert np.array_equal(out[0][0][k], out[1][0][k]), k
    for k in TALLY_KEYS:
        assert np.array_equal(out[0][1][k], out[1][1][k]), k
    # (the moment sums are floating-point atomics: the same addends in whatever order the waves arrive, run to run)
    assert np.allclose(out[0][1]["rec_sums"], out[1][1]["rec_sums"], rtol=1e-12, atol=0)


# -- 9. a map too large for any LDS -------------------------------------------------------------------------------------------
def test_a_million_slot_map_traces_and_conserves():
    scene = conservation_scene(shape=(128, 128, 64))
    assert compile_scene(scene).map_slots == 5 * (128 * 128 * 64 + 1)
    result = simulate(scene, 1_000_000, seed=5, record_every=0, emission="device", emit_seed=6)
    assert_conserved(result)
    assert result.volume_maps["absorbed"].counts.shape == (128, 128, 64)
    small = simulate(conservation_scene(), 1_000_000, seed=5, record_every=0, emission="device", emit_seed=6)
    fine = result.volume_maps["absorbed"].counts.reshape(8, 16, 8, 16, 4, 16).sum(axis=(1, 3, 5))
    assert np.array_equal(fine, small.volume_maps["absorbed"].counts)       # the same photons, coarser cells


# -- 10. Beer-Lambert -----------------------------------------------------------------------------------------------------------
def test_lost_map_follows_beer_lambert_at_a_million_photons():
    alpha, cells, n = 1.0, 8, 1_000_000
    scene = beer_lambert_scene(alpha, cells)
    with Session(scene, emission="host") as s:
        result = submit(s, pencil((0.1, -0.2, -5.0), (0.0, 0.0, 1.0), 555.0, n), 17, record_every=0)
    lost = result.volume_maps["lost"]
    assert lost.outside == 0
    counts = np.append(lost.counts[0, 0], n - lost.total)
    L.assert_chi2(counts, beer_lambert_probabilities(alpha, cells), "GPU lost map, Beer-Lambert")


# -- 11. the packer ---------------------------------------------------------------------------------------------------------------
def test_the_packer_refuses_each_malformed_table_with_its_own_message():
    compiled = compile_scene(BT.map_scene())
    lib = native.load_library()
    st, keep = native.scene_tables_struct(compiled)

    def attempt(n_nodes=2, **change):
        mt, held = BT.map_tables(n_nodes, **change)
        handle = C.c_void_p()
        rc = lib.pvt_scene_create_maps(C.byref(st), None, None, None, None, C.byref(mt), 0, C.byref(handle))
        if rc == 0:
            slots = lib.pvt_scene_map_slots(handle)
            lib.pvt_scene_destroy(handle)
            return slots
        assert not handle.value
        return lib.pvt_last_error().decode()

    assert attempt() == 22
    bad = BT.MAP_BREAKS   # (the cases: tests/broken_tables.py)
    messages = {}
    for what, change in bad.items():
        msg = attempt(**change)
        assert isinstance(msg, str) and "map tables" in msg, (what, msg)
        messages[what] = msg
    assert len(set(messages.values())) == len(messages), messages
    handle = C.c_void_p()   # no maps: exactly pvt_scene_create_field
    assert lib.pvt_scene_create_maps(C.byref(st), None, None, None, None, None, 0, C.byref(handle)) == 0
    assert lib.pvt_scene_map_slots(handle) == 0
    lib.pvt_scene_destroy(handle)


# -- 12. the example -----------------------------------------------------------------------------------------------------------------
def test_photobleach_example_absorbs_less_where_it_bleached():
    spec = importlib.util.spec_from_file_location("photobleach", os.path.join(ROOT, "examples", "photobleach.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    out = module.main(photons=200_000)
    worst = out["worst"]
    assert worst.any()
    assert int(out["dose_after"].counts[worst].sum()) < int(out["dose_before"].counts[worst].sum())
    assert out["dose_after"].total < out["dose_before"].total
    assert out["edge_before"] > 0 and out["edge_after"] > 0
