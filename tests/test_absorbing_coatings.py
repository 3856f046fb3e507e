"""Absorbing coatings (`Coating(..., absorptivity=...)`) and `detected` recorders without a GPU: what the constructor and
the flattener refuse, what a scene lowers to, and the host tracer held to the rule's closed forms -- the three-way split,
tables, total internal reflection, clipping where R + A > 1 -- and to the DETECT row's contract."""
import hashlib
import json
import math
import os

import numpy as np
import pytest

from pvtrace_amd import AbsorptivityTable, Coating, Event, Ray, ReflectivityTable, photon_tracer
from pvtrace_amd.engine import Recorder, capture_histories, compile_scene, tally_histories
from pvtrace_amd.engine import recorder as recorder_module
from pvtrace_amd.engine.compiler import CompiledScene
from tests import absorbing_scenes as S
from tests import scenes
from tests.util import GOLD

TOP = S.TOP


# -- 1. refusals -------------------------------------------------------------------------------------------------------------------
def test_constructor_refuses_bad_absorptivities_each_with_its_message():
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"absorptivity must be in \[0, 1\], an AbsorptivityTable or None"):
            Coating(TOP, absorptivity=bad)
    with pytest.raises(ValueError, match=r"reflectivity \+ absorptivity must not exceed 1: R = 0.7, A = 0.4$"):
        Coating(TOP, reflectivity=0.7, absorptivity=0.4)
    Coating(TOP, reflectivity=0.6, absorptivity=0.4)   # (exactly 1 is allowed)
    # table + number: the table's own vertices decide
    r_table = ReflectivityTable([500.0, 600.0], [[0.1, 0.3], [0.5, 0.7]], angle=[0.0, 90.0])
    with pytest.raises(ValueError, match=r"must not exceed 1: R = 0.7, A = 0.4 at 600 nm, 90 degrees"):
        Coating(TOP, reflectivity=r_table, absorptivity=0.4)
    Coating(TOP, reflectivity=r_table, absorptivity=0.3)
    # table + table: each is fine at its own vertices (R peaks where A is low and the other way round); the sum exceeds
    # one only at (550 nm, 45 degrees), a vertex of the union grid that is a vertex of neither table alone
    r_tab = ReflectivityTable([500.0, 550.0, 600.0], [[0.1, 0.9, 0.1], [0.1, 0.9, 0.1]], angle=[0.0, 90.0])
    a_tab = AbsorptivityTable([500.0, 600.0], [[0.05, 0.05], [0.3, 0.3], [0.05, 0.05]], angle=[0.0, 45.0, 90.0])
    assert 550.0 not in a_tab.wavelength and 45.0 not in r_tab.angle
    for wl in r_tab.wavelength:
        for ang in r_tab.angle:
            assert r_tab.at(wl, ang) + a_tab.at(wl, ang) <= 1.0
    for wl in a_tab.wavelength:
        for ang in a_tab.angle:
            assert r_tab.at(wl, ang) + a_tab.at(wl, ang) <= 1.0
    with pytest.raises(ValueError, match=r"must not exceed 1: R = 0.9, A = 0.3 at 550 nm, 45 degrees"):
        Coating(TOP, reflectivity=r_tab, absorptivity=a_tab)
    # a malformed table is the table class's own refusal: the alias IS the class
    assert AbsorptivityTable is ReflectivityTable
    with pytest.raises(ValueError, match=r"values must be finite and in \[0, 1\]"):
        AbsorptivityTable([500.0, 600.0], [0.2, 1.2])
    with pytest.raises(ValueError, match="wavelength must be finite and strictly increasing"):
        AbsorptivityTable([600.0, 500.0], [0.2, 0.3])


def test_flattener_refuses_an_absorptivity_set_out_of_range_after_construction():
    from pvtrace_amd.engine.compiler import UnsupportedSceneError

    coating = Coating(TOP, absorptivity=0.5)
    coating.absorptivity = 1.5
    with pytest.raises(UnsupportedSceneError, match=r"absorptivity must be in \[0, 1\], got 1.5"):
        compile_scene(S.coated_box([coating]))


def test_recorder_vocabulary_keeps_the_reference_dict_and_gains_an_extension():
    assert recorder_module.EXTENSION_EVENTS == {"detected": 7}
    assert "detected" not in recorder_module.EVENTS and len(recorder_module.EVENTS) == 7
    assert Recorder("d", event="detected").event == "detected"
    with pytest.raises(ValueError) as err:
        Recorder("r", event="vanished")
    golden = json.load(open(os.path.join(GOLD, "recorder_ids.json")))
    assert str(err.value) == golden["refused"]["recorder_unknown_event"]
    header = open(os.path.join(os.path.dirname(GOLD), "..", "include", "pvtrace_hip.h")).read()
    assert "#define PVT_RECX_DETECTED 7" in header and "PVT_EV_DETECT = 10" in header
    assert Event.DETECT.value == 10


# -- 2. lowering -------------------------------------------------------------------------------------------------------------------
PLAIN_SCENES = ("hello_world", "lsc_equivalent", "nested_cylinders", "coated_slab", "fresnel_box", "bench_slab", "kitchen_sink",
                "touching_boxes", "trapped_light", "lambertian_sheet", "hist_slab", "hist_lamp", "mesh_lsc", "mesh_gem",
                "l_prism", "lambertian_fog", "hello_world_recorded", "tiles6")


def tables_digest(tables):
    """sha256 over every table of a lowered scene, in key order: name, dtype, shape, bytes."""
    h = hashlib.sha256()
    for key in sorted(tables):
        a = np.ascontiguousarray(tables[key])
        h.update(key.encode()); h.update(a.dtype.str.encode()); h.update(repr(a.shape).encode()); h.update(a.tobytes())
    return h.hexdigest()


def test_scenes_without_an_absorbing_coating_lower_to_the_tables_they_had():
    """tests/golden/lowering_digests.json holds, per scene of tests/scenes.py, the keys of `tables()` and the digest of
    their bytes as the flattener gave them before coatings could absorb."""
    golden = json.load(open(os.path.join(GOLD, "lowering_digests.json")))
    assert sorted(golden) == sorted(PLAIN_SCENES)
    for name in PLAIN_SCENES:
        compiled = compile_scene(getattr(scenes, name)())
        tables = compiled.tables()
        assert not compiled.has_absorbing_coatings
        assert sorted(tables) == golden[name]["keys"], name                 # no new key, none lost
        assert not set(tables) & set(CompiledScene.ABSORB_TABLE_FIELDS), name
        assert tables_digest(tables) == golden[name]["sha256"], name        # byte for byte


def test_absorptivity_none_lowers_as_no_absorptivity_and_a_value_adds_its_tables():
    def lowered(**kw):
        mirror = Coating(TOP, reflectivity=0.9, region=((0.0, None), None, None), **kw)
        return compile_scene(S.coated_box([mirror, Coating((1, 0, 0), reflectivity=ReflectivityTable([500.0, 600.0], [0.2, 0.4]))]))

    bare, none = lowered().tables(), lowered(absorptivity=None).tables()
    assert sorted(bare) == sorted(none) and tables_digest(bare) == tables_digest(none)
    table = S.step_table()
    scene = S.coated_box([Coating(TOP, reflectivity=0.3, absorptivity=0.5), Coating((1, 0, 0), absorptivity=table),
                          Coating((0, 1, 0), reflectivity=0.2), Coating((-1, 0, 0), absorptivity=table)])
    compiled = compile_scene(scene)
    tables = compiled.tables()
    assert compiled.has_absorbing_coatings and set(CompiledScene.ABSORB_TABLE_FIELDS) <= set(tables)
    assert set(tables) - set(CompiledScene.ABSORB_TABLE_FIELDS) == set(bare)
    assert tables["coat_absorptivity"].tolist() == [0.5, 0.0, 0.0, 0.0] and tables["coat_absorptivity"].dtype == np.float64
    assert tables["coat_abs_table"].tolist() == [-1, 0, -1, 0] and tables["coat_abs_table"].dtype == np.int32   # (pooled once)
    assert tables["atab_nw"].tolist() == [2] and tables["atab_na"].tolist() == [2]
    assert tables["atab_wl_start"].tolist() == tables["atab_angle_start"].tolist() == tables["atab_value_start"].tolist() == [0]
    assert tables["atab_wavelength"].tolist() == [500.0, 600.0] and tables["atab_angle"].tolist() == [20.0, 60.0]
    assert tables["atab_value"].tolist() == [0.2, 0.6, 0.4, 0.8]
    # the reflectivity side is what it was
    assert tables["coat_reflectivity"].tolist() == [0.3, -1.0, 0.2, -1.0] and tables["coat_table"].tolist() == [-1, -1, -1, -1]
    # absorptivity=0.0 is an absorptivity: it lowers (to zeros), so that the library can prove it changes nothing
    zero = compile_scene(S.coated_box([Coating(TOP, reflectivity=0.3, absorptivity=0.0)])).tables()
    assert zero["coat_absorptivity"].tolist() == [0.0] and zero["coat_abs_table"].tolist() == [-1]


def test_host_buffer_entry_refuses_an_absorbing_scene():
    from pvtrace_amd.engine import _kernel
    from pvtrace_amd.engine.compiler import UnsupportedSceneError

    compiled = compile_scene(S.coated_box([Coating(TOP, absorptivity=0.5)]))
    rays = np.zeros((1, 3)), np.array([[0.0, 0.0, 1.0]]), np.array([555.0])
    with pytest.raises(UnsupportedSceneError, match="absorbing coatings"):
        _kernel.trace_bundle(compiled, *rays, 1, 10, 16, 0, 1, 0)


# -- 3-6. the host tracer against the rule -----------------------------------------------------------------------------------------
def outcomes(scene, start, direction, wavelength, n, seed):
    """Counts of the first surface event of `n` rays of one pencil, traced on the host objects."""
    np.random.seed(seed)
    counts = {Event.REFLECT: 0, Event.TRANSMIT: 0, Event.DETECT: 0}
    ray = Ray(start, direction, wavelength)
    for _ in range(n):
        history = photon_tracer.follow(scene, ray, maxsteps=1, backend="host")
        counts[history[1][1]] += 1
        assert history[-1][1] in (Event.DETECT, Event.KILL) and (history[1][1] != Event.DETECT or len(history) == 2)
    return counts


def test_three_way_split_is_multinomial():
    n = 20_000
    scene = S.coated_box([Coating(TOP, reflectivity=0.3, absorptivity=0.5)], recorders=False)   # n = 1 both sides: Fresnel R = 0
    got = outcomes(scene, *S.pencil_from_above(), 555.0, n, seed=101)
    print("three-way", got)
    assert sum(got.values()) == n
    assert S.five_sigma(got[Event.REFLECT], n, 0.3) and S.five_sigma(got[Event.DETECT], n, 0.5)
    assert S.five_sigma(got[Event.TRANSMIT], n, 0.2)


def test_table_absorptivity_holds_in_each_cell_and_at_its_nodes():
    table = S.step_table()
    # nodes and an interior point, by hand: 0.2 + 0.5 (0.6 - 0.2) = 0.4 and 0.4 + 0.5 (0.8 - 0.4) = 0.6 at 550 nm, their
    # mean 0.5 at 40 degrees
    assert [table.at(500.0, 20.0), table.at(600.0, 20.0), table.at(500.0, 60.0), table.at(600.0, 60.0)] == [0.2, 0.6, 0.4, 0.8]
    assert table.at(550.0, 20.0) == pytest.approx(0.4, abs=1e-15) and table.at(550.0, 40.0) == pytest.approx(0.5, abs=1e-15)
    assert table.at(300.0, 0.0) == 0.2 and table.at(900.0, 90.0) == 0.8          # clamped, like a reflectivity table
    scene = S.coated_box([Coating(TOP, absorptivity=table)], recorders=False)      # reflectivity None, n = 1: R = 0
    n = 5000
    for k, ((wl, angle), a) in enumerate(S.STEP_CELLS.items()):
        got = outcomes(scene, *S.pencil_from_above(math.radians(angle)), wl, n, seed=200 + k)
        print("cell", wl, angle, got)
        assert got[Event.REFLECT] == 0
        assert S.five_sigma(got[Event.DETECT], n, a) and S.five_sigma(got[Event.TRANSMIT], n, 1.0 - a)


def test_total_internal_reflection_beats_absorption_unless_matched():
    n = 500
    theta = math.radians(60.0)      # beyond asin(1 / 1.5) = 41.8 degrees
    fresnel = S.coated_box([Coating(TOP, reflectivity=0.0, absorptivity=1.0)], n_box=1.5, recorders=False)
    got = outcomes(fresnel, *S.pencil_from_inside(theta), 555.0, n, seed=301)
    assert got == {Event.REFLECT: n, Event.TRANSMIT: 0, Event.DETECT: 0}
    matched = S.coated_box([Coating(TOP, reflectivity=0.0, absorptivity=1.0, transmission="matched")], n_box=1.5, recorders=False)
    got = outcomes(matched, *S.pencil_from_inside(theta), 555.0, n, seed=302)
    assert got == {Event.REFLECT: 0, Event.TRANSMIT: 0, Event.DETECT: n}


def test_absorption_is_clipped_where_r_plus_a_exceeds_one():
    n = 20_000
    theta = math.radians(80.0)
    r = S.fresnel_r(theta, 1.0, 1.5)
    assert 0.38 < r < 0.39     # (Hecht: 0.3878 for air -> glass at 80 degrees)
    scene = S.coated_box([Coating(TOP, absorptivity=1.0)], n_box=1.5, recorders=False)   # reflectivity None: Fresnel
    got = outcomes(scene, *S.pencil_from_above(theta), 555.0, n, seed=401)
    print("clipping", got, "R =", r)
    assert S.five_sigma(got[Event.REFLECT], n, r)
    assert got[Event.DETECT] == n - got[Event.REFLECT] and got[Event.TRANSMIT] == 0


def test_absorptivity_zero_draws_nothing_more_than_no_absorptivity():
    """The same seeded sequence gives the same histories, event for event and number for number."""
    def run(absorptivity):
        scene = S.s1_slab(absorptivity=absorptivity)
        np.random.seed(9)
        rays = list(scene.emit(60))
        np.random.seed(10)
        return [list(photon_tracer.step_forward(scene, ray, backend="host")) for ray in rays]

    none, zero, table = run(None), run(0.0), run("zero")
    assert none == zero == table
    assert any(e == Event.REFLECT for h in none for _, e, _ in h) and len(none) == 60


# -- 7. the DETECT row and its recorder --------------------------------------------------------------------------------------------
def test_detect_row_ends_the_history_and_the_recorder_counts_its_face_only():
    theta = math.radians(35.0)
    coatings = [Coating(TOP, reflectivity=0.0, absorptivity=0.6, transmission="matched"),
                Coating((0, 0, -1), reflectivity=0.0, absorptivity=1.0, transmission="matched")]
    scene = S.coated_box(coatings, recorders=False)
    box = next(n for n in scene.root.preorder() if n.name == "box")
    box.recorders = [Recorder("top", event="detected", facet=TOP, capture=1000,
                              histograms=[S.Histogram("angle", 0.0, math.pi / 2, 9)]),
                     Recorder("bottom", event="detected", facet=(0, 0, -1)), Recorder("any", event="detected")]
    start, direction = S.pencil_from_above(theta, at=(0.5, -0.25))
    np.random.seed(77)
    n = 400
    histories = [list(photon_tracer.step_forward(scene, Ray(start, direction, 600.0), backend="host")) for _ in range(n)]
    on_top = [h for h in histories if len(h) == 2]
    through = [h for h in histories if len(h) == 3]
    assert len(on_top) + len(through) == n and S.five_sigma(len(on_top), n, 0.6)
    for h in on_top:
        ray, event, meta = h[-1]
        assert event == Event.DETECT and meta["hit"] == "box" and meta["container"] == "world" and meta["adjacent"] == "box"
        assert ray.position == pytest.approx((0.5, -0.25, 1.0), abs=1e-12) and tuple(ray.direction) == tuple(direction)
        assert tuple(meta["normal"]) == TOP and ray.travelled == pytest.approx(1.0) and ray.wavelength == 600.0
    for h in through:     # transmitted unrefracted, then absorbed by the bottom face from INSIDE
        assert [e for _, e, _ in h] == [Event.GENERATE, Event.TRANSMIT, Event.DETECT]
        ray, _, meta = h[-1]
        assert meta["hit"] == meta["container"] == "box" and meta["adjacent"] == "world" and ray.position[2] == pytest.approx(-1.0)
        assert tuple(ray.direction) == pytest.approx(direction)
    tallies = tally_histories(scene, histories)
    assert tallies["top"].rays == tallies["top"].crossings == len(on_top)
    assert tallies["bottom"].rays == tallies["bottom"].crossings == len(through)
    assert tallies["any"].rays == tallies["any"].crossings == n
    bins = np.asarray(tallies["top"].histogram(0)[1])
    assert bins[int(theta / (math.pi / 2) * 9)] == len(on_top) == bins.sum()      # 35 degrees: the middle of bin 3 of 9
    captured = capture_histories(scene, histories)["top"]
    assert len(captured) == len(on_top) and np.allclose(captured.position[:, 2], 1.0, rtol=0, atol=1e-12)
    assert np.array_equal(captured.direction, np.tile(direction, (len(on_top), 1)))
    # follow() drops the metadata and keeps the event
    np.random.seed(78)
    assert photon_tracer.follow(scene, Ray(start, direction, 600.0), backend="host")[-1][1] == Event.DETECT
