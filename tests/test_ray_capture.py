"""Ray capture (`Recorder(..., capture=rows)`) without a GPU: the constructor's and the flattener's refusals, the lowered
tables, the ctypes structs against the C header, and `capture_histories` -- the host path and the GPU tests' referee --
held to `tally_histories` and to the histories themselves, on host-traced rays and on a committed event log."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pvtrace_amd.algorithm import photon_tracer
from pvtrace_amd.engine import CapturedRays, Recorder, capture_histories, compile_scene, native, tally_histories
from pvtrace_amd.engine.api import EngineResult
from pvtrace_amd.engine.compiler import UnsupportedSceneError
from pvtrace_amd.engine.recorder import MAX_CAPTURE_ROWS
from tests import scenes
from tests.util import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def node(scene, name):
    return next(n for n in scene.root.preorder() if n.name == name)


def captured_lsc(capacity=1 << 16, **only):
    """The headline slab, every recorder of it captured (`only`: per-name capacities instead)."""
    scene = scenes.lsc_equivalent()
    for rec in node(scene, "LSC").recorders:
        rec.capture = only.get(rec.name) if only else capacity
    return scene


# -- the constructor ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [0, -1, 2.5, "10", True, 1.0])
def test_recorder_refuses_a_capacity_that_is_no_positive_integer(bad):
    with pytest.raises(ValueError, match="capture must be a positive"):
        Recorder("edge", event="escaping", capture=bad)


def test_recorder_takes_a_capacity_and_defaults_to_none():
    assert Recorder("edge").capture is None
    assert Recorder("edge", capture=5).capture == 5
    assert Recorder("edge", capture=np.int64(7)).capture == 7 and type(Recorder("edge", capture=np.int64(7)).capture) is int


# -- the flattener ------------------------------------------------------------------------------------------------------
def test_a_scene_without_captures_lowers_to_exactly_todays_tables():
    compiled = compile_scene(scenes.lsc_equivalent())
    assert not compiled.has_captures and compiled.capture_rows == 0
    tables = compiled.tables()
    assert not [k for k in tables if "capture" in k]
    assert sorted(tables) == sorted(compiled.TABLE_FIELDS + ("root_id", "total_bins"))
    assert native.capture_tables_struct(compiled) == (None, {})
    captured = compile_scene(captured_lsc())
    assert sorted(set(captured.tables()) - set(tables)) == ["capture_rows", "rec_capture_capacity", "rec_capture_start"]
    for name, value in tables.items():
        assert np.array_equal(value, captured.tables()[name]), name


def test_capacities_and_starts_are_lowered_in_recorder_order():
    scene = captured_lsc(top=10, left=3, lost=1000)
    compiled = compile_scene(scene)
    want = np.array([{"top": 10, "left": 3, "lost": 1000}.get(n, 0) for n in compiled.recorder_names], dtype=np.int64)
    assert compiled.rec_capture_capacity.dtype == np.int64 and np.array_equal(compiled.rec_capture_capacity, want)
    assert np.array_equal(compiled.rec_capture_start, np.concatenate([[0], np.cumsum(want)[:-1]]))
    assert compiled.capture_rows == 1013 and compiled.has_captures
    st, keep = native.capture_tables_struct(compiled)
    assert st.n_recorders == len(want) and st.capture_rows == 1013
    assert [st.rec_capture_capacity[r] for r in range(len(want))] == list(want)


def test_the_flattener_refuses_too_many_rows_and_a_mutated_capacity():
    scene = captured_lsc(top=MAX_CAPTURE_ROWS, left=1)
    with pytest.raises(UnsupportedSceneError, match="more than 16777216 rows"):
        compile_scene(scene)
    assert compile_scene(captured_lsc(top=MAX_CAPTURE_ROWS)).capture_rows == 1 << 24
    scene = captured_lsc(top=5)
    node(scene, "LSC").recorders[0].capture = -3
    with pytest.raises(UnsupportedSceneError, match="capture must be a positive integer"):
        compile_scene(scene)
    node(scene, "LSC").recorders[0].capture = np.int64(6)    # what the constructor takes, the flattener takes
    compiled = compile_scene(scene)
    assert compiled.capture_rows == 6 and int(compiled.rec_capture_capacity.max()) == 6


def test_the_host_buffer_entry_refuses_captured_scenes():
    from pvtrace_amd.engine import _kernel

    with pytest.raises(UnsupportedSceneError, match="captured recorders"):
        _kernel._host_buffer_scene(compile_scene(captured_lsc()))


def test_the_structs_and_the_limit_match_the_header():
    header = open(os.path.join(ROOT, "include", "pvtrace_hip.h")).read()
    assert "#define PVT_MAX_CAPTURE_ROWS (1LL << 24)" in header and MAX_CAPTURE_ROWS == 1 << 24
    assert f"#define PVT_CAPTURE_ROW_WORDS {native.CAPTURE_ROW_WORDS}" in header
    for struct in (native.PvtCaptureTables, native.PvtCaptures):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct.__name__, struct.__name__), header, re.S).group(1)
        fields = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
        assert fields == [name for name, _ in struct._fields_]
    assert C.sizeof(native.PvtCaptureTables) == 32 and C.sizeof(native.PvtCaptures) == 16
    for symbol in ("pvt_scene_create_capture", "pvt_scene_capture_rows", "pvt_trace_device_capture"):
        assert symbol in header and symbol in native.ABI_SYMBOLS


# -- capture_histories ----------------------------------------------------------------------------------------------------
def host_history(scene, ray):
    """What `follow(scene, ray, backend="host")` walks, metadata kept: `follow` itself returns (ray, event) pairs."""
    return list(photon_tracer.step_forward(scene, ray, backend="host"))


def first_matches(scene, histories, name):
    """Per ray, the history event at which a one-recorder tally first counts it: found by tallying the history's prefixes."""
    out = {}
    for j, history in enumerate(histories):
        for k in range(len(history)):
            if tally_histories(scene, [history[:k + 1]])[name].rays == 1:
                out[j] = history[k][0]
                break
    return out


def check_against_the_histories(scene, histories, offset=0):
    captures = capture_histories(scene, histories, ray_offset=offset)
    tallies = tally_histories(scene, histories)
    compiled = compile_scene(scene)
    assert sorted(captures) == sorted(r.name for r in compiled.recorder_specs if r.capture)
    for name, got in captures.items():
        assert isinstance(got, CapturedRays)
        assert len(got) + got.dropped == got.matched == tallies[name].rays, name
        assert np.all(np.diff(got.index) > 0)       # one row per ray, ascending
        rays = first_matches(scene, histories, name)
        kept = sorted(rays)[:got.capacity]           # the capacity in ray order
        assert list(got.index - offset) == kept, name
        for row, j in enumerate(kept):
            ray = rays[j]
            assert tuple(got.position[row]) == tuple(ray.position) and tuple(got.direction[row]) == tuple(ray.direction)
            assert (got.wavelength[row], got.pathlength[row], got.duration[row]) == (ray.wavelength, ray.travelled, ray.duration)
            want = compiled.component_names.index(ray.source) if ray.source in compiled.component_names else -1
            assert got.source[row] == want
    return captures, tallies


def test_capture_histories_on_host_traced_rays():
    scene = captured_lsc(top=1 << 10, bottom=1 << 10, left=4, lost=1 << 10, entering=1 << 10, reflected=3)
    node(scene, "LSC").recorders.append(Recorder("glow-top", event="escaping", facet=(0, 0, 1), source="components", capture=99))
    np.random.seed(11)
    histories = [host_history(scene, ray) for ray in scene.emit(300)]
    captures, tallies = check_against_the_histories(scene, histories, offset=1000)
    assert tallies["entering"].rays > 200 and len(captures["entering"]) == tallies["entering"].rays
    assert captures["reflected"].dropped > 0 and len(captures["reflected"]) == 3
    assert len(captures["glow-top"]) > 0 and np.all(captures["glow-top"].source >= 0)
    assert np.all(captures["entering"].source == -1)


def test_capture_histories_on_a_committed_event_log():
    g = load_golden("trace_lsc_equivalent.npz")
    scene = captured_lsc()
    data = {k[4:]: g[k] for k in g.files if k.startswith("ref_")}
    result = EngineResult(compile_scene(scene), data, ["Light"] * len(g["in_wl"]), int(g["par_max_events"]), 1, 0.0)
    histories = list(result.histories())
    captures, tallies = check_against_the_histories(scene, histories)
    for r, name in enumerate(result.compiled.recorder_names):
        assert captures[name].matched == int(g["ref_rec_distinct"][r]), name     # the reference kernel's own `rays`
    assert captures["entering"].matched > 200 and captures["top"].matched > 0


def test_merged_captures_concatenate_and_sort():
    scene = captured_lsc(entering=1 << 10)
    np.random.seed(3)
    histories = [host_history(scene, ray) for ray in scene.emit(40)]
    whole = capture_histories(scene, histories)["entering"]
    parts = [capture_histories(scene, histories[25:], ray_offset=25)["entering"], capture_histories(scene, histories[:25])["entering"]]
    merged = CapturedRays.merged(parts)
    assert merged.matched == whole.matched and merged.capacity == whole.capacity
    for name, column in whole.columns().items():
        assert np.array_equal(column, merged.columns()[name]), name
