"""Photon event counters (`Histogram("emissions" | "scatterings" | "reflections", ...)` and the capture columns of the
same names) without a GPU: the vocabulary and what the flattener lowers, the host path (`engine.tally`) on a hand-written
history with known answers, and the host tracer held to two closed forms -- the geometric law of re-emission in an opaque
luminescent ball and the bounce count of a guided pencil, found by unfolding its path."""
import json
import math
import os

import numpy as np
import pytest

from pvtrace_amd import Box, Luminophore, Material, Node, Scene, Sphere
from pvtrace_amd.algorithm import photon_tracer
from pvtrace_amd.engine import (
    CapturedRays, Heatmap, Histogram, Recorder, capture_histories, compile_scene, tally_histories,
)
from pvtrace_amd.engine import recorder as R
from pvtrace_amd.engine.compiler import UnsupportedSceneError
from pvtrace_amd.light import Event, Ray
from tests import laws as L
from tests import scenes

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
COUNTERS = ("emissions", "scatterings", "reflections")

# -- the two closed-form scenes, shared with tests/test_gpu_history_counters.py ------------------------------------------
QUANTUM_YIELD = 0.7
EMISSION_BINS = 16
PENCIL_ANGLE = math.radians(60.0)
GUIDE_SIZE = (10.0, 1.0, 1.0)
PENCIL_START = (-4.0, 0.0, 0.0)
REFLECTION_BINS = 64


def opaque_ball():
    """A ball of radius 1 whose luminophore (yield 0.7) absorbs 10^3 per cm at every wavelength it can emit: a photon
    born at the centre never reaches the surface (exp(-1000)), so it is re-emitted k times with probability q^k (1 - q)
    and then lost.  `lost` bins the emissions it arrives with -> (scene, the ray's start, direction, wavelength)."""
    x = np.linspace(300.0, 900.0, 61)
    dye = Luminophore(np.column_stack((x, np.full_like(x, 1e3))),
                      emission=np.column_stack((x, np.exp(-((x - 600.0) / 40.0) ** 2))), quantum_yield=QUANTUM_YIELD,
                      name="dye")
    world = Node(name="world", geometry=Sphere(radius=10.0, material=Material(refractive_index=1.0)))
    ball = Node(name="ball", parent=world,
                geometry=Sphere(radius=1.0, material=Material(refractive_index=1.5, components=[dye])))
    ball.recorders = [Recorder("lost", event="lost", histograms=[Histogram("emissions", 0, EMISSION_BINS, EMISSION_BINS)]),
                      Recorder("out", event="escaping")]
    return Scene(world), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 500.0


def geometric_law(counts, rays, what):
    """P(k) = q^k (1 - q) on the `emissions` bins, the photons with 16 or more emissions as one more category."""
    q = QUANTUM_YIELD
    probs = [q ** k * (1.0 - q) for k in range(EMISSION_BINS)] + [q ** EMISSION_BINS]
    counts = [int(c) for c in counts]
    L.assert_multinomial(counts + [int(rays) - sum(counts)], probs, what)


def guide():
    """A lossless n = 1.5 bar, 10 x 1 x 1, and a pencil inside it in the xz plane at 60 degrees from z: beyond the critical
    angle (41.8 degrees) at the top and bottom faces, at 30 degrees -- inside the escape cone -- at the +x facet.  `right`
    bins the reflections of what escapes through that facet -> (scene, start, direction, wavelength)."""
    world = Node(name="world", geometry=Box((100.0, 100.0, 100.0), material=Material(refractive_index=1.0)))
    bar = Node(name="bar", parent=world, geometry=Box(GUIDE_SIZE, material=Material(refractive_index=1.5)))
    bar.recorders = [Recorder("right", event="escaping", facet=(1, 0, 0),
                              histograms=[Histogram("reflections", 0, REFLECTION_BINS, REFLECTION_BINS)]),
                     Recorder("any", event="escaping")]
    return Scene(world), PENCIL_START, (math.sin(PENCIL_ANGLE), 0.0, math.cos(PENCIL_ANGLE)), 555.0


def unfolded_bounces():
    """Reflections of the pencil before it FIRST reaches the +x facet: unfold the bar along z -- the straight line from the
    start climbs dz = dx / tan(60 degrees) while it runs dx to the facet, and crosses one image of a face per bar depth."""
    length, _, depth = GUIDE_SIZE
    dx = length / 2.0 - PENCIL_START[0]
    climb = PENCIL_START[2] + depth / 2.0 + dx / math.tan(PENCIL_ANGLE)
    assert abs(climb / depth - round(climb / depth)) > 0.05     # (the pencil does not end in an edge of the bar)
    return int(math.floor(climb / depth))


def host_history(scene, ray):
    return list(photon_tracer.step_forward(scene, ray, backend="host"))


# -- the vocabulary and the flattener --------------------------------------------------------------------------------------
def test_the_references_properties_are_untouched_and_the_counters_lower_to_7_8_9():
    with open(os.path.join(GOLD, "recorder_ids.json")) as fp:
        assert R.PROPERTIES == json.load(fp)["PROPERTIES"] and len(R.PROPERTIES) == 7
    assert R.EXTENSION_PROPERTIES == {"emissions": 7, "scatterings": 8, "reflections": 9}
    assert R.ALL_PROPERTIES == {**R.PROPERTIES, **R.EXTENSION_PROPERTIES}
    scene = scenes.lsc_equivalent(recorders=False)
    slab = next(n for n in scene.root.preorder() if n.name == "LSC")
    slab.recorders = [Recorder("lost", event="lost", histograms=[
        Histogram("emissions", 0, 16, 16), Histogram("scatterings", 0, 4, 4), Histogram("reflections", 0, 8, 8),
        Heatmap("emissions", "reflections", (0, 4, 4), (0, 8, 8)), Heatmap("reflections", "wavelength", (0, 8, 8), (400, 800, 4))])]
    compiled = compile_scene(scene)
    assert list(compiled.hist_prop_a) == [7, 8, 9, 7, 9] and list(compiled.hist_prop_b) == [-1, -1, -1, 9, 0]
    assert compiled.has_counter_histograms and compiled.total_bins == 16 + 4 + 8 + 32 + 32
    assert not compile_scene(scenes.lsc_equivalent()).has_counter_histograms
    header = open(os.path.join(os.path.dirname(GOLD), "..", "include", "pvtrace_hip.h")).read()
    for name, code in R.EXTENSION_PROPERTIES.items():
        assert f"#define PVT_PROPX_{name.upper()} {code}" in header
    for name, code in R.PROPERTIES.items():
        assert f"PVT_PROP_{name.upper()} = {code}" in header
    with pytest.raises(ValueError, match="Unknown property"):
        Histogram("absorptions", 0, 4, 4)


def test_the_host_buffer_entry_refuses_a_counter_histogram():
    from pvtrace_amd.engine import _kernel

    scene, *_ = opaque_ball()
    with pytest.raises(UnsupportedSceneError, match="photon event counter"):
        _kernel._host_buffer_scene(compile_scene(scene))


# -- a hand-written history ------------------------------------------------------------------------------------------------
def hand_written():
    """GENERATE, TRANSMIT in, ABSORB, EMIT, REFLECT, REFLECT, ABSORB, EMIT, TRANSMIT out: a photon enters a slab, is
    re-emitted, bounces twice off the outside of a core inside the slab, is re-emitted again and leaves."""
    world = Node(name="world", geometry=Box((100.0, 100.0, 100.0), material=Material(refractive_index=1.0)))
    slab = Node(name="slab", parent=world, geometry=Box((10.0, 10.0, 2.0), material=Material(refractive_index=1.5)))
    core = Node(name="core", parent=slab, geometry=Box((1.0, 1.0, 0.5), material=Material(refractive_index=1.7)))
    hists = lambda: [Histogram(name, 0, 4, 4) for name in COUNTERS] + [Heatmap("emissions", "reflections", (0, 4, 4), (0, 4, 4))]
    slab.recorders = [Recorder("escaping", event="escaping", histograms=hists(), capture=8),
                      Recorder("entering", event="entering", histograms=hists(), capture=8)]
    core.recorders = [Recorder("reflected", event="reflected", histograms=hists(), capture=8)]
    up, down = (0.0, 0.0, 1.0), (0.0, 0.0, -1.0)
    ray = lambda z, d, wl=555.0, src="lamp": Ray((3.0, 0.0, z), d, wl, travelled=5.0 - z, duration=1e-9, source=src)
    into = {"hit": "slab", "container": "world", "adjacent": "slab", "normal": up}
    off_core = {"hit": "core", "container": "slab", "adjacent": "core", "normal": up}
    out = {"hit": "slab", "container": "slab", "adjacent": "world", "normal": up}
    history = [
        (ray(5.0, down), Event.GENERATE, {}), (ray(1.0, down), Event.TRANSMIT, into),
        (ray(0.8, down), Event.ABSORB, {"container": "slab", "component": "dye"}),
        (ray(0.8, down, 600.0, "dye"), Event.EMIT, {"container": "slab", "component": "dye"}),
        (ray(0.25, up, 600.0, "dye"), Event.REFLECT, off_core), (ray(0.25, up, 600.0, "dye"), Event.REFLECT, off_core),
        (ray(0.9, up, 600.0, "dye"), Event.ABSORB, {"container": "slab", "component": "dye"}),
        (ray(0.9, up, 650.0, "dye"), Event.EMIT, {"container": "slab", "component": "dye"}),
        (ray(1.0, up, 650.0, "dye"), Event.TRANSMIT, out),
    ]
    return Scene(world), history


def test_a_hand_written_history_has_the_known_answers():
    scene, history = hand_written()
    tallies = tally_histories(scene, [history])
    want = {"escaping": (2, 0, 2), "entering": (0, 0, 0), "reflected": (1, 0, 0)}
    assert tallies["reflected"].crossings == 2 and tallies["reflected"].rays == 1
    for name, values in want.items():
        rec = tallies[name]
        assert rec.rays == 1
        for k, value in enumerate(values):                      # the 1-D histograms: one ray, in the bin of the value
            assert list(rec._bins[k]) == [1 if b == value else 0 for b in range(4)], (name, COUNTERS[k])
        joint = rec._bins[3].reshape(4, 4)
        assert joint[values[0], values[2]] == 1 and joint.sum() == 1, name
    captures = capture_histories(scene, [history], ray_offset=40)
    for name, values in want.items():
        rows = captures[name]
        assert isinstance(rows, CapturedRays) and len(rows) == 1 and rows.index[0] == 40
        assert (int(rows.emissions[0]), int(rows.scatterings[0]), int(rows.reflections[0])) == values, name
        assert all(getattr(rows, c).dtype == np.int32 for c in COUNTERS)
    assert R.CAPTURE_COLUMNS[-3:] == COUNTERS and list(captures["escaping"].columns())[-3:] == list(COUNTERS)
    # a SCATTER row counts as a scattering, nothing else does
    scattered = history[:4] + [(history[3][0], Event.SCATTER, {"container": "slab", "component": "fog"})] + history[4:]
    rows = capture_histories(scene, [scattered])["escaping"]
    assert (int(rows.emissions[0]), int(rows.scatterings[0]), int(rows.reflections[0])) == (2, 1, 2)


def test_captured_rays_keep_the_counters_through_rows_merges_and_old_dicts():
    columns = {"index": [5, 3], "position": np.zeros((2, 3)), "direction": np.ones((2, 3)), "wavelength": [1.0, 2.0],
               "pathlength": [0.0, 0.0], "duration": [0.0, 0.0], "source": [-1, 2]}
    old = CapturedRays("r", 4, 2, columns)                     # a dict from before the counters: zeros
    assert all(np.array_equal(getattr(old, c), np.zeros(2, np.int32)) and getattr(old, c).dtype == np.int32 for c in COUNTERS)
    new = CapturedRays("r", 4, 2, {**columns, "emissions": [7, 1], "scatterings": [0, 2], "reflections": [9, 3]})
    assert list(new.index) == [3, 5] and list(new.emissions) == [1, 7] and list(new.reflections) == [3, 9]   # sorted with the rest
    merged = CapturedRays.merged([new, CapturedRays("r", 4, 1, {k: np.asarray(v)[:1] for k, v in {**columns, "index": [1], "emissions": [4]}.items()})])
    assert list(merged.index) == [1, 3, 5] and list(merged.emissions) == [4, 1, 7] and list(merged.scatterings) == [0, 2, 0]
    rows = np.zeros((2, 12), dtype=np.uint64)                  # device rows: word 11 = emissions | scatterings << 20 | reflections << 40
    rows[:, 0] = 8, 9
    rows[0, 11] = 3 | (5 << 20) | (1048575 << 40)
    rows[1, 11] = 1048575 | (0 << 20) | (2 << 40)
    got = CapturedRays.from_rows("r", 4, 2, rows)
    assert list(got.emissions) == [3, 1048575] and list(got.scatterings) == [5, 0] and list(got.reflections) == [1048575, 2]
    header = open(os.path.join(os.path.dirname(GOLD), "..", "include", "pvtrace_hip.h")).read()
    assert "emissions | scatterings << 20 | reflections << 40" in header and R.COUNTER_BITS == 20


# -- the host tracer against closed forms ----------------------------------------------------------------------------------
def test_host_tracer_emissions_of_an_opaque_luminescent_ball_are_geometric():
    scene, start, direction, wl = opaque_ball()
    np.random.seed(17)
    n = 3000
    histories = [host_history(scene, Ray(start, direction, wl, source="lamp")) for _ in range(n)]
    tallies = tally_histories(scene, histories)
    assert tallies["out"].rays == 0 and tallies["lost"].rays == n      # none escapes, every photon is lost in the end
    geometric_law(tallies["lost"]._bins[0], n, "host tracer, emissions of lost photons")
    # the histories themselves say the same: EMIT rows before the NONRADIATIVE row
    direct = np.bincount([sum(1 for _, e, _ in h if e == Event.EMIT) for h in histories], minlength=EMISSION_BINS)[:EMISSION_BINS]
    assert np.array_equal(direct, tallies["lost"]._bins[0])


def test_host_tracer_guided_pencil_escapes_after_the_unfolded_number_of_bounces():
    scene, start, direction, wl = guide()
    bounces = unfolded_bounces()
    assert bounces == 5
    np.random.seed(23)
    histories = [host_history(scene, Ray(start, direction, wl, source="lamp")) for _ in range(400)]
    tallies = tally_histories(scene, histories)
    bins = tallies["right"]._bins[0]
    assert tallies["right"].rays > 300                                   # (Fresnel at 30 degrees inside glass: most leave at once)
    assert int(np.flatnonzero(bins)[0]) == bounces and bins[bounces] > 300
    assert tallies["any"].rays == 400                                    # lossless: every photon leaves the bar


def test_the_spec_readers_recorders_section_takes_the_counter_names():
    from pvtrace_amd.engine.instrument import recorders_from_spec

    scene, *_ = opaque_ball()
    ball = next(n for n in scene.root.preorder() if n.name == "ball")
    ball.recorders = []
    recorders_from_spec({"lost": {"node": "ball", "event": "lost", "histograms": {
        "emissions": [0, 16, 16], "position": ["emissions", "reflections", [0, 4, 4], [0, 8, 8]]}}}, {"ball": ball})
    compiled = compile_scene(scene)
    assert list(compiled.hist_prop_a) == [7, 7] and list(compiled.hist_prop_b) == [-1, 9]
