"""Volume maps (`VolumeMap`: per-voxel integer tallies of a node's volume events) on the host: the constructor's and the
flattener's refusals, the lowered tables restated by hand, the ctypes struct against the C header, `map_histories` on
hand-written histories (every slot stated here), and the host tracer's `lost` map held to the Beer-Lambert law.
No GPU needed."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from pvtrace_amd import (
    Absorber, Box, ConcentrationGrid, Event, Luminophore, Material, Node, Ray, Reactor, Scene, Surface, VolumeMap,
    VolumeMapResult,
)
from pvtrace_amd.algorithm import photon_tracer
from pvtrace_amd.engine import Recorder, map_histories, native
from pvtrace_amd.engine.compiler import UnsupportedSceneError, compile_scene
from pvtrace_amd.engine.recorder import MAX_MAP_SLOTS
from pvtrace_amd.material import NullSurfaceDelegate
from tests import laws as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO, HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)


def two_blocks():
    """World, block `a` at (3, 0, 0) with two components, block `b` at (-3, 0, 0) turned a quarter about z."""
    x = np.linspace(400.0, 800.0, 5)
    world = Node(name="world", geometry=Box((40.0, 40.0, 40.0), material=Material(refractive_index=1.0)))
    a = Node(name="a", parent=world, geometry=Box((2.0, 2.0, 2.0), material=Material(
        refractive_index=1.0, surface=Surface(NullSurfaceDelegate()),
        components=[Luminophore(1.0, x=x, name="dye"), Absorber(0.5, name="bg")])))
    a.translate((3.0, 0.0, 0.0))
    b = Node(name="b", parent=world, geometry=Box((2.0, 2.0, 2.0), material=Material(
        refractive_index=1.0, surface=Surface(NullSurfaceDelegate()), components=[Reactor(1.0, name="cat")])))
    b.rotate(np.pi / 2, (0.0, 0.0, 1.0))
    b.translate((-3.0, 0.0, 0.0))
    return Scene(world), world, a, b


# -- 1. the constructor -------------------------------------------------------------------------------------------------
def test_constructor_keeps_what_it_is_given():
    m = VolumeMap("m", (2, 3, 4), (-1, -1, 0), (1, 2, 2), event="emitted", component="dye", wavelength=(400, 800, 16))
    assert (m.name, m.shape, m.lower, m.upper) == ("m", (2, 3, 4), (-1.0, -1.0, 0.0), (1.0, 2.0, 2.0))
    assert (m.event, m.component, m.wavelength_bins) == ("emitted", "dye", 16)
    assert m.cell_widths == (1.0, 1.0, 0.5) and m.size == 2 * 3 * 4 * 16 + 1
    plain = VolumeMap("p", (1, 1, 1), LO, HI)
    assert plain.event == "absorbed" and plain.component is None and plain.wavelength is None and plain.size == 2


def test_like_copies_the_lattice_of_a_grid():
    grid = ConcentrationGrid(np.ones((3, 2, 5)), (-2.0, -1.0, 0.0), (2.5, 1.0, 0.75))
    m = VolumeMap.like(grid, "m", event="lost", component="bg")
    assert m.shape == (3, 2, 5) and m.lower == (-2.0, -1.0, 0.0) and m.upper == (2.5, 1.0, 0.75)
    assert m.event == "lost" and m.component == "bg"
    assert np.array_equal(m.cell_widths, grid.h)


@pytest.mark.parametrize("what, kwargs, message", [
    ("event", dict(shape=(1, 1, 1), lower=LO, upper=HI, event="killed"), "Unknown volume-map event"),
    ("zero shape", dict(shape=(2, 0, 2), lower=LO, upper=HI), "shape must be >= 1"),
    ("2-d shape", dict(shape=(2, 2), lower=LO, upper=HI), "three integers"),
    ("fractional shape", dict(shape=(2, 2.5, 2), lower=LO, upper=HI), "three integers"),
    ("inverted", dict(shape=(1, 1, 1), lower=(0, 2, 0), upper=(1, 1, 1)), "lower < upper"),
    ("equal", dict(shape=(1, 1, 1), lower=(0, 0, 1), upper=(1, 1, 1)), "lower < upper"),
    ("infinite", dict(shape=(1, 1, 1), lower=(0, 0, -np.inf), upper=(1, 1, 1)), "must be finite"),
    ("nan", dict(shape=(1, 1, 1), lower=(0, 0, 0), upper=(1, 1, np.nan)), "must be finite"),
    ("wavelength range", dict(shape=(1, 1, 1), lower=LO, upper=HI, wavelength=(800, 400, 4)), "stop > start"),
    ("wavelength bins", dict(shape=(1, 1, 1), lower=LO, upper=HI, wavelength=(400, 800, 0)), "at least one bin"),
])
def test_constructor_refusals(what, kwargs, message):
    with pytest.raises(ValueError, match=message):
        VolumeMap("m", **kwargs)


def test_bounds_are_required():
    with pytest.raises(TypeError):
        VolumeMap("m", (1, 1, 1))


# -- 2. the flattener ---------------------------------------------------------------------------------------------------
def test_flattener_refusals_each_with_its_own_message():
    def refused(attach):
        scene, world, a, b = two_blocks()
        attach(world, a, b)
        with pytest.raises(UnsupportedSceneError) as err:
            compile_scene(scene)
        return str(err.value)

    def on_empty_node(world, a, b):
        Node(name="frame", parent=world).volume_maps = [VolumeMap("m", (1, 1, 1), LO, HI)]

    def twice(world, a, b):
        a.volume_maps = [VolumeMap("m", (1, 1, 1), LO, HI)]
        b.volume_maps = [VolumeMap("m", (1, 1, 1), LO, HI, event="reacted")]

    def as_a_recorder(world, a, b):
        a.recorders = [Recorder("m", event="lost")]
        b.volume_maps = [VolumeMap("m", (1, 1, 1), LO, HI)]

    def too_large(world, a, b):
        a.volume_maps = [VolumeMap("big", (1024, 1024, 32), LO, HI), VolumeMap("more", (1024, 1024, 32), LO, HI)]

    def not_a_map(world, a, b):
        a.volume_maps = [Recorder("r", event="lost")]

    def mutated_event(world, a, b):
        m = VolumeMap("m", (1, 1, 1), LO, HI)
        m.event = "entering"
        a.volume_maps = [m]

    messages = {
        "root": refused(lambda w, a, b: setattr(w, "volume_maps", [VolumeMap("m", (1, 1, 1), LO, HI)])),
        "no geometry": refused(on_empty_node),
        "component": refused(lambda w, a, b: setattr(a, "volume_maps", [VolumeMap("m", (1, 1, 1), LO, HI, component="cat")])),
        "duplicate": refused(twice),
        "recorder name": refused(as_a_recorder),
        "slots": refused(too_large),
        "type": refused(not_a_map),
        "event": refused(mutated_event),
    }
    assert "root cannot carry a volume map" in messages["root"]
    assert "has no geometry" in messages["no geometry"]
    assert "unknown component 'cat'" in messages["component"] and "dye" in messages["component"]
    assert "must be unique" in messages["duplicate"]
    assert "recorder has the same name" in messages["recorder name"]
    assert str(MAX_MAP_SLOTS) in messages["slots"] and MAX_MAP_SLOTS == 2 ** 26
    assert "must be VolumeMap objects" in messages["type"]
    assert "unknown event 'entering'" in messages["event"]
    assert len(set(messages.values())) == len(messages)


def test_a_scene_without_maps_lowers_to_the_tables_it_had():
    scene, world, a, b = two_blocks()
    c = compile_scene(scene)
    assert not c.has_maps and c.n_maps == 0 and c.map_slots == 0
    plain = c.tables()
    assert set(plain) == set(c.TABLE_FIELDS) | {"root_id", "total_bins"}
    assert not any("map" in name for name in c.TABLE_FIELDS)
    assert native.map_tables_struct(c)[0] is None
    assert a.volume_maps == [] and world.volume_maps == []
    # maps add tables of their own and change none of the others; total_bins keeps its meaning
    a.recorders = [Recorder("lost", event="lost")]
    before = compile_scene(scene).tables()
    a.volume_maps = [VolumeMap("m", (2, 2, 2), LO, HI)]
    after = compile_scene(scene).tables()
    assert set(after) - set(before) == set(c.MAP_TABLE_FIELDS) | {"map_slots"}
    for key, value in before.items():
        assert np.array_equal(np.asarray(value), np.asarray(after[key])), key


def test_lowered_tables_match_hand_written_expectations():
    scene, world, a, b = two_blocks()
    a.volume_maps = [VolumeMap("a-abs", (2, 2, 2), LO, HI),
                     VolumeMap("a-dye-emitted", (4, 1, 2), (-1.0, 0.0, -0.5), (1.0, 0.5, 0.5), event="emitted",
                               component="bg", wavelength=(400.0, 800.0, 4))]
    b.volume_maps = [VolumeMap("b-reacted", (1, 1, 3), (-1.0, -1.0, -1.0), (1.0, 1.0, 0.5), event="reacted")]
    c = compile_scene(scene)
    assert c.has_maps and c.n_maps == 3 and c.map_names == ["a-abs", "a-dye-emitted", "b-reacted"]
    assert c.node_names == ["world", "a", "b"] and c.component_names == ["dye", "bg", "cat"]
    assert np.array_equal(c.node_map_start, [0, 0, 2]) and np.array_equal(c.node_map_count, [0, 2, 1])
    assert np.array_equal(c.map_kind, [3, 6, 8])            # ABSORB, EMIT, REACT
    assert np.array_equal(c.map_component, [-1, 1, -1])
    assert np.array_equal(c.map_shape, [[2, 2, 2], [4, 1, 2], [1, 1, 3]])
    assert np.array_equal(c.map_lower, [[-1.0, -1.0, -1.0], [-1.0, 0.0, -0.5], [-1.0, -1.0, -1.0]])
    assert np.array_equal(c.map_h, [[1.0, 1.0, 1.0], [0.5, 0.5, 0.5], [2.0, 2.0, 0.5]])
    assert np.array_equal(c.map_nw, [0, 4, 0])
    assert np.array_equal(c.map_wl_start, [0.0, 400.0, 0.0]) and np.array_equal(c.map_wl_stop, [1.0, 800.0, 1.0])
    assert np.array_equal(c.map_offset, [0, 9, 42]) and c.map_offset.dtype == np.int64   # 8 + 1, 4 * 1 * 2 * 4 + 1, 3 + 1
    assert c.map_slots == 46 and c.total_bins == 0
    st, keep = native.map_tables_struct(c)
    assert (st.n_nodes, st.n_maps, st.map_slots) == (3, 3, 46)
    assert [st.map_offset[i] for i in range(3)] == [0, 9, 42] and st.map_h[8] == 0.5


def test_ctypes_struct_matches_the_header(tmp_path):
    header = os.path.join(ROOT, "include", "pvtrace_hip.h")
    fields = [name for name, _ in native.PvtMapTables._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"', "int main(void){",
             'printf("size %zu\\n", sizeof(PvtMapTables));', 'printf("limit %lld\\n", (long long)PVT_MAX_MAP_SLOTS);']
    lines += [f'printf("{f} %zu\\n", offsetof(PvtMapTables, {f}));' for f in fields]
    lines.append("return 0;}")
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).strip().splitlines())
    assert int(out.pop("size")) == C.sizeof(native.PvtMapTables)
    assert int(out.pop("limit")) == MAX_MAP_SLOTS
    for f in fields:
        assert getattr(native.PvtMapTables, f).offset == int(out[f]), f


def test_the_host_buffer_entry_refuses_maps(built):
    from pvtrace_amd.engine import _kernel

    scene, world, a, b = two_blocks()
    a.volume_maps = [VolumeMap("m", (1, 1, 1), LO, HI)]
    with pytest.raises(UnsupportedSceneError, match="volume maps"):
        _kernel.trace_bundle(compile_scene(scene), np.zeros((1, 3)), np.array([[0.0, 0.0, 1.0]]), np.array([555.0]),
                             0, 10, 4, 0, 1, 1)


# -- 3. map_histories on hand-written histories ---------------------------------------------------------------------------
def ev(kind, position, wavelength, container, component):
    ray = Ray(position=tuple(position), direction=(0.0, 0.0, 1.0), wavelength=wavelength)
    return ray, kind, {"container": container, "component": component}


def test_map_histories_bins_by_the_contract():
    scene, world, a, b = two_blocks()
    a.volume_maps = [
        VolumeMap("abs", (2, 2, 2), LO, HI),
        VolumeMap("abs-bg", (2, 2, 2), LO, HI, component="bg"),
        VolumeMap("emitted-wl", (1, 1, 1), LO, HI, event="emitted", wavelength=(400.0, 800.0, 4)),
        VolumeMap("lost-roi", (1, 1, 2), (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), event="lost"),
    ]
    b.volume_maps = [VolumeMap("reacted", (2, 1, 1), LO, HI, event="reacted")]
    A = lambda x, y, z: (x + 3.0, y, z)                    # a's frame -> world: a translation, exact here
    Bw = lambda x, y, z: (-y - 3.0, x, z)                  # b's frame -> world: a quarter turn about z, then (-3, 0, 0)
    histories = [
        [ev(Event.GENERATE, (0, 0, -5), 555.0, "world", None),
         ev(Event.ABSORB, A(-0.5, -0.5, -0.5), 555.0, "a", "dye"),          # abs cell (0,0,0) = slot 0
         ev(Event.EMIT, A(-0.5, -0.5, -0.5), 400.0, "a", "dye"),            # wavelength = start: bin 0
         ev(Event.ABSORB, A(0.0, 0.0, 0.0), 400.0, "a", "bg"),              # on three faces: cell (1,1,1) = slot 7
         ev(Event.NONRADIATIVE, A(0.0, 0.0, 0.0), 400.0, "a", "bg")],       # roi: z = 0 is the face -> cell (0,0,1)
        [ev(Event.ABSORB, A(1.0, 0.0, 0.0), 500.0, "a", "dye"),             # on `upper`: outside
         ev(Event.EMIT, A(1.0, 0.0, 0.0), 800.0, "a", "dye"),               # wavelength = stop: outside
         ev(Event.ABSORB, A(-1.0, -1.0, -1.0), 800.0, "a", "dye"),          # on `lower`: cell (0,0,0) = slot 0
         ev(Event.EMIT, A(-1.0, -1.0, -1.0), 799.9, "a", "dye"),            # last bin 3
         ev(Event.ABSORB, A(0.5, -0.5, 0.5), 799.9, "a", "bg"),             # cell (1,0,1) = slot 5
         ev(Event.NONRADIATIVE, A(0.5, -0.5, 0.5), 799.9, "a", "bg")],      # roi: z = 0.5 is `upper` -> outside
        [ev(Event.ABSORB, A(0.25, 0.25, -0.25), 600.0, "a", "dye"),         # cell (1,1,0) = slot 6
         ev(Event.EMIT, A(0.25, 0.25, -0.25), 650.0, "a", "dye"),           # (650 - 400) / 400 * 4 = 2.5: bin 2
         ev(Event.ABSORB, A(0.25, 0.25, -0.25), 650.0, "world", None),      # another container: not counted
         ev(Event.ABSORB, Bw(0.5, 0.5, 0.0), 650.0, "b", "cat"),
         ev(Event.REACT, Bw(0.5, 0.5, 0.0), 650.0, "b", "cat")],            # b cell (1,0,0) = slot 1
        [ev(Event.ABSORB, Bw(-0.5, 0.9, 0.9), 555.0, "b", "cat"),
         ev(Event.REACT, Bw(-0.5, 0.9, 0.9), 555.0, "b", "cat"),            # b cell (0,0,0) = slot 0
         ev(Event.ABSORB, Bw(-0.5, 0.0, 1.5), 555.0, "b", "cat"),
         ev(Event.REACT, Bw(-0.5, 0.0, 1.5), 555.0, "b", "cat")],           # z beyond the lattice: outside
    ]
    maps = map_histories(scene, histories)
    assert sorted(maps) == ["abs", "abs-bg", "emitted-wl", "lost-roi", "reacted"]
    assert all(isinstance(m, VolumeMapResult) for m in maps.values())
    expect = np.zeros((2, 2, 2), np.int64)
    expect[0, 0, 0], expect[1, 1, 1], expect[1, 0, 1], expect[1, 1, 0] = 2, 1, 1, 1
    assert np.array_equal(maps["abs"].counts, expect) and maps["abs"].outside == 1 and maps["abs"].total == 6
    assert maps["abs"].counts.dtype == np.int64 and maps["abs"].counts.ravel()[[0, 5, 6, 7]].tolist() == [2, 1, 1, 1]
    bg = np.zeros((2, 2, 2), np.int64)
    bg[1, 1, 1], bg[1, 0, 1] = 1, 1
    assert np.array_equal(maps["abs-bg"].counts, bg) and maps["abs-bg"].outside == 0
    assert maps["emitted-wl"].counts.shape == (1, 1, 1, 4)
    assert maps["emitted-wl"].counts.ravel().tolist() == [1, 0, 1, 1] and maps["emitted-wl"].outside == 1
    assert maps["lost-roi"].counts.ravel().tolist() == [0, 1] and maps["lost-roi"].outside == 1
    assert maps["reacted"].counts.ravel().tolist() == [1, 1] and maps["reacted"].outside == 1
    r = maps["lost-roi"]
    assert (r.shape, r.lower, r.upper, r.cell_volume) == ((1, 1, 2), (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), 0.5)
    # the compiled scene serves as well, and no history gives zeros
    empty = map_histories(compile_scene(scene), [])
    assert all(m.total == 0 for m in empty.values()) and map_histories(two_blocks()[0], histories) == {}


# -- 4. the host tracer against Beer-Lambert ------------------------------------------------------------------------------
def beer_lambert_scene(alpha, cells):
    world = Node(name="world", geometry=Box((40.0, 40.0, 40.0), material=Material(refractive_index=1.0)))
    slab = Node(name="slab", parent=world, geometry=Box((2.0, 2.0, 2.0), material=Material(
        refractive_index=1.0, surface=Surface(NullSurfaceDelegate()), components=[Absorber(alpha, name="ink")])))
    slab.volume_maps = [VolumeMap("lost", (1, 1, cells), LO, HI, event="lost")]
    return Scene(world)


def beer_lambert_probabilities(alpha, cells, thickness=2.0):
    """p_k = exp(-alpha z_k) - exp(-alpha z_{k+1}) per cell along the pencil, then the transmitted remainder."""
    z = np.linspace(0.0, thickness, cells + 1)
    edges = np.exp(-alpha * z)
    return np.append(edges[:-1] - edges[1:], edges[-1])


def test_host_tracer_lost_map_follows_beer_lambert():
    alpha, cells = 1.0, 8
    probs = beer_lambert_probabilities(alpha, cells)
    n = math.ceil(L.CHI2_MIN_EXPECTED / probs.min())     # every cell's expected count reaches the chi-square's minimum
    scene = beer_lambert_scene(alpha, cells)
    np.random.seed(12)
    ray = Ray(position=(0.1, -0.2, -5.0), direction=(0.0, 0.0, 1.0), wavelength=555.0)
    histories = [list(photon_tracer.step_forward(scene, ray, backend="host")) for _ in range(n)]
    lost = map_histories(scene, histories)["lost"]
    assert lost.outside == 0 and lost.counts.shape == (1, 1, cells)
    counts = np.append(lost.counts[0, 0], n - lost.total)
    assert counts[-1] == sum(1 for h in histories if h[-1][1] == Event.EXIT)
    L.assert_chi2(counts, probs, "host lost map, Beer-Lambert")
