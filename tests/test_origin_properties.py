"""Launch origin as histogram properties (`Histogram("origin_wavelength" | "origin_x" | "origin_y" | "origin_z", ...)`)
without a GPU: the vocabulary and what the flattener lowers, the host path (`engine.tally`) on a hand-written history with
known answers, and the host tracer held to the Beer-Lambert law per LAUNCH wavelength."""
import json
import math
import os

import numpy as np
import pytest

from pvtrace_amd import Absorber, Box, Material, Node, Scene
from pvtrace_amd.algorithm import photon_tracer
from pvtrace_amd.engine import Heatmap, Histogram, Recorder, compile_scene, tally_histories
from pvtrace_amd.engine import recorder as R
from pvtrace_amd.engine.compiler import UnsupportedSceneError
from pvtrace_amd.light import Event, Ray
from tests import laws as L
from tests import scenes

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ORIGINS = ("origin_wavelength", "origin_x", "origin_y", "origin_z")

# -- the Beer-Lambert scene, shared with tests/test_gpu_origin_properties.py ---------------------------------------------
BL_WAVELENGTHS = np.arange(420.0, 720.0, 40.0)             # the 8 launch wavelengths: 420, 460, ..., 700 nm
BL_ALPHAS = np.array([0.05, 0.2, 0.5, 1.0, 1.5, 2.5, 4.0, 0.0])   # per cm at those wavelengths
BL_DEPTH = 0.8
BL_HISTOGRAM = ("origin_wavelength", 400.0, 720.0, 8)      # bin k holds launch wavelength k alone


def beer_lambert_slab():
    """An absorber slab of thickness d, index-matched (n = 1: no reflection, no refraction) in a world of n = 1, with alpha
    tabulated AT the 8 launch wavelengths: a ray launched at wavelength k at normal incidence leaves the scene with
    probability exp(-alpha_k d) and is lost otherwise.  `exit` on the root bins the launch wavelength."""
    assert len(BL_WAVELENGTHS) == len(BL_ALPHAS) == 8
    world = Node(name="world", geometry=Box((20.0, 20.0, 20.0), material=Material(refractive_index=1.0)))
    slab = Node(name="slab", parent=world, geometry=Box((4.0, 4.0, BL_DEPTH), material=Material(
        refractive_index=1.0, components=[Absorber(np.column_stack((BL_WAVELENGTHS, BL_ALPHAS)), name="dye")])))
    slab.recorders = [Recorder("lost", event="lost", histograms=[Histogram(*BL_HISTOGRAM)])]
    world.recorders = [Recorder("exit", event="exit", histograms=[Histogram(*BL_HISTOGRAM)])]
    return Scene(world)


def beer_lambert_rays(n):
    """n rays, n / 8 per launch wavelength, interleaved, straight down onto the slab from points spread over its face."""
    assert n % 8 == 0
    k = np.arange(n)
    pos = np.column_stack((-1.5 + 3.0 * ((k * 0.6180339887498949) % 1.0), -1.5 + 3.0 * ((k * 0.7548776662466927) % 1.0),
                           np.full(n, 3.0)))
    return pos, np.tile((0.0, 0.0, -1.0), (n, 1)), BL_WAVELENGTHS[k % 8]


def beer_lambert_law(exit_bins, lost_bins, n, what):
    """Bin k of `exit` within 5 sigma (binomial) of (n / 8) exp(-alpha_k d); what did not leave was lost, wavelength by
    wavelength."""
    per = n // 8
    for k, alpha in enumerate(BL_ALPHAS):
        print(what, BL_WAVELENGTHS[k], int(exit_bins[k]), per * math.exp(-alpha * BL_DEPTH))
        L.assert_binomial(int(exit_bins[k]), per, math.exp(-alpha * BL_DEPTH), (what, float(BL_WAVELENGTHS[k])))
        assert int(exit_bins[k]) + int(lost_bins[k]) == per, (what, k)


# -- the vocabulary and the flattener --------------------------------------------------------------------------------------
def test_the_older_vocabularies_are_untouched_and_the_origins_lower_to_10_to_13():
    with open(os.path.join(GOLD, "recorder_ids.json")) as fp:
        assert R.PROPERTIES == json.load(fp)["PROPERTIES"] and len(R.PROPERTIES) == 7
    assert R.EXTENSION_PROPERTIES == {"emissions": 7, "scatterings": 8, "reflections": 9}
    assert R.ALL_PROPERTIES == {**R.PROPERTIES, **R.EXTENSION_PROPERTIES}
    assert R.ORIGIN_PROPERTIES == {"origin_wavelength": 10, "origin_x": 11, "origin_y": 12, "origin_z": 13}
    assert R.HISTOGRAM_PROPERTIES == {**R.ALL_PROPERTIES, **R.ORIGIN_PROPERTIES} and len(R.HISTOGRAM_PROPERTIES) == 14
    scene = scenes.lsc_equivalent(recorders=False)
    slab = next(n for n in scene.root.preorder() if n.name == "LSC")
    slab.recorders = [Recorder("lost", event="lost", histograms=[
        Histogram("origin_wavelength", 400, 800, 40), Histogram("origin_x", -3, 3, 6), Histogram("origin_y", -3, 3, 6),
        Histogram("origin_z", 0, 8, 4), Heatmap("origin_x", "origin_y", (-3, 3, 8), (-3, 3, 8)),
        Heatmap("wavelength", "origin_wavelength", (400, 800, 4), (400, 800, 4))])]
    compiled = compile_scene(scene)
    assert list(compiled.hist_prop_a) == [10, 11, 12, 13, 11, 0] and list(compiled.hist_prop_b) == [-1, -1, -1, -1, 12, 10]
    assert compiled.total_bins == 40 + 6 + 6 + 4 + 64 + 16
    # an origin is no event counter: the scene does not count
    assert not compiled.has_counter_histograms and compiled.origin_mask == 0b1111
    slab.recorders = [Recorder("lost", event="lost", histograms=[Heatmap("origin_y", "emissions", (-3, 3, 8), (0, 4, 4))])]
    mixed = compile_scene(scene)
    assert mixed.has_counter_histograms and mixed.origin_mask == 0b0100
    plain = compile_scene(scenes.lsc_equivalent())
    assert not plain.has_counter_histograms and plain.origin_mask == 0
    header = open(os.path.join(os.path.dirname(GOLD), "..", "include", "pvtrace_hip.h")).read()
    for name, code in R.ORIGIN_PROPERTIES.items():
        assert f"#define PVT_PROPX_{name.upper()} {code}" in header
    assert "pvt_scene_create_origin(" in header
    with pytest.raises(ValueError, match="Unknown property"):
        Histogram("origin_direction", 0, 4, 4)
    with pytest.raises(ValueError, match="Unknown property"):
        Heatmap("origin_x", "origin", (0, 1, 1), (0, 1, 1))


def test_the_host_buffer_entry_refuses_an_origin_histogram():
    from pvtrace_amd.engine import _kernel

    with pytest.raises(UnsupportedSceneError, match="launch-origin property"):
        _kernel._host_buffer_scene(compile_scene(beer_lambert_slab()))


# -- a hand-written history ------------------------------------------------------------------------------------------------
def hand_written():
    """GENERATE at 450 nm and (3, 0, 5), TRANSMIT in, ABSORB, EMIT at 600 nm, REFLECT, TRANSMIT out at (1, 2, 1): a photon
    enters a slab, is re-emitted at another wavelength, wanders and leaves at another point."""
    world = Node(name="world", geometry=Box((100.0, 100.0, 100.0), material=Material(refractive_index=1.0)))
    slab = Node(name="slab", parent=world, geometry=Box((10.0, 10.0, 2.0), material=Material(refractive_index=1.5)))
    hists = lambda: [Histogram("origin_wavelength", 400, 700, 6), Histogram("wavelength", 400, 700, 6),
                     Histogram("origin_x", 0, 4, 4), Histogram("x", 0, 4, 4), Histogram("origin_y", -2, 2, 4),
                     Histogram("y", -2, 4, 6), Histogram("origin_z", 0, 8, 8), Histogram("z", 0, 8, 8),
                     Heatmap("origin_wavelength", "wavelength", (400, 700, 6), (400, 700, 6)),
                     Heatmap("origin_x", "emissions", (0, 4, 4), (0, 4, 4))]
    slab.recorders = [Recorder("escaping", event="escaping", histograms=hists()),
                      Recorder("entering", event="entering", histograms=hists())]
    up, down = (0.0, 0.0, 1.0), (0.0, 0.0, -1.0)
    ray = lambda p, d, wl, src="lamp": Ray(p, d, wl, travelled=1.0, duration=1e-9, source=src)
    into = {"hit": "slab", "container": "world", "adjacent": "slab", "normal": up}
    inside = {"hit": "slab", "container": "slab", "adjacent": "world", "normal": down}
    out = {"hit": "slab", "container": "slab", "adjacent": "world", "normal": up}
    dye = {"container": "slab", "component": "dye"}
    history = [
        (ray((3.0, 0.0, 5.0), down, 450.0), Event.GENERATE, {}), (ray((3.0, 0.0, 1.0), down, 450.0), Event.TRANSMIT, into),
        (ray((3.0, 0.0, 0.5), down, 450.0), Event.ABSORB, dye), (ray((3.0, 0.0, 0.5), down, 600.0, "dye"), Event.EMIT, dye),
        (ray((2.0, 1.0, -1.0), up, 600.0, "dye"), Event.REFLECT, inside),
        (ray((1.0, 2.0, 1.0), up, 600.0, "dye"), Event.TRANSMIT, out),
    ]
    return Scene(world), history


def one_hot(bins, at):
    return [1 if b == at else 0 for b in range(bins)]


def test_a_hand_written_history_bins_the_launch_values_beside_the_events_values():
    scene, history = hand_written()
    tallies = tally_histories(scene, [history])
    esc, ent = tallies["escaping"], tallies["entering"]
    assert esc.rays == ent.rays == 1
    # escaping: launched at 450 nm (bin 1) from (3, 0, 5); the event is at 600 nm (bin 4) and (1, 2, 1)
    assert list(esc._bins[0]) == one_hot(6, 1) and list(esc._bins[1]) == one_hot(6, 4)
    assert list(esc._bins[2]) == one_hot(4, 3) and list(esc._bins[3]) == one_hot(4, 1)
    assert list(esc._bins[4]) == one_hot(4, 2) and list(esc._bins[5]) == one_hot(6, 4)
    assert list(esc._bins[6]) == one_hot(8, 5) and list(esc._bins[7]) == one_hot(8, 1)
    joint = esc._bins[8].reshape(6, 6)
    assert joint[1, 4] == 1 and joint.sum() == 1
    joint = esc._bins[9].reshape(4, 4)
    assert joint[3, 1] == 1 and joint.sum() == 1                    # launched at x = 3, arrives after one emission
    # entering: the event's wavelength IS the launch wavelength there, and x, y too; z is not
    assert list(ent._bins[0]) == list(ent._bins[1]) == one_hot(6, 1)
    assert list(ent._bins[2]) == list(ent._bins[3]) == one_hot(4, 3)
    assert list(ent._bins[6]) == one_hot(8, 5) and list(ent._bins[7]) == one_hot(8, 1)
    # an origin outside a histogram's range is binned nowhere, as any other property
    scene.root.children[0].recorders = [Recorder("escaping", event="escaping", histograms=[Histogram("origin_x", 0, 3, 3)])]
    assert tally_histories(scene, [history])["escaping"]._bins[0].sum() == 0


# -- the host tracer against the Beer-Lambert law, per launch wavelength ---------------------------------------------------
def test_host_tracer_transmission_per_launch_wavelength_is_beer_lamberts():
    scene = beer_lambert_slab()
    n = 2400
    pos, dirs, wl = beer_lambert_rays(n)
    np.random.seed(41)
    histories = [list(photon_tracer.step_forward(scene, Ray(tuple(pos[j]), tuple(dirs[j]), float(wl[j]), source="lamp"),
                                                 backend="host")) for j in range(n)]    # (what `follow(backend="host")` runs)
    tallies = tally_histories(scene, histories)
    assert tallies["exit"].rays + tallies["lost"].rays == n
    beer_lambert_law(tallies["exit"]._bins[0], tallies["lost"]._bins[0], n, "host tracer")
    assert tallies["exit"]._bins[0][7] == n // 8                    # alpha = 0 at 700 nm: every such ray leaves


def test_the_spec_readers_recorders_section_takes_the_origin_names():
    from pvtrace_amd.engine.instrument import recorders_from_spec

    scene = beer_lambert_slab()
    slab = next(n for n in scene.root.preorder() if n.name == "slab")
    slab.recorders, scene.root.recorders = [], []
    recorders_from_spec({"lost": {"node": "slab", "event": "lost", "histograms": {
        "origin_wavelength": [400, 720, 8], "position": ["origin_x", "origin_y", [-2, 2, 8], [-2, 2, 8]]}}}, {"slab": slab})
    compiled = compile_scene(scene)
    assert list(compiled.hist_prop_a) == [10, 11] and list(compiled.hist_prop_b) == [-1, 12]
    assert compiled.origin_mask == 0b0111
