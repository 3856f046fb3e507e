"""Ray capture (`Recorder(..., capture=rows)`) on the GPU.  The referee is the event log: one launch with `record_every=1`
gives both the kernel's captured rows and every ray's history, and `capture_histories` picks each ray's first match out of
those histories on the host.  Every column is compared bit for bit.  Then the captures are held to themselves (tally
launches, carried launches, streams, shards, a ray alone), to the recorders' `rays`, and to the overflow contract."""
import ctypes as C
import importlib.util
import os
import warnings

import numpy as np
import pytest

from pvtrace_amd import VolumeMap
from pvtrace_amd.engine import (
    Recorder, Session, capture_histories, compile_scene, native, simulate, simulate_stream, trace_stream,
)
from pvtrace_amd.engine.emit import emit_bundle
from pvtrace_amd.engine.recorder import CAPTURE_COLUMNS
from tests import scenes
from tests.capture_scenes import history_launch, node, rough_fielded_block, submit

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 1 << 20
EDGES = {"right": (1, 0, 0), "left": (-1, 0, 0), "far": (0, 1, 0), "near": (0, -1, 0)}
TALLY_KEYS = ("rec_distinct", "rec_crossings", "rec_bins")
HIST_KEYS = ("counts", "kind", "hit", "container", "component", "source", "position", "direction", "wavelength",
             "travelled", "duration")


def same_captures(a, b, names=None):
    assert sorted(a) == sorted(b)
    for name in (names or a):
        assert len(a[name]) == len(b[name]) and a[name].matched == b[name].matched, (name, a[name], b[name])
        for column in CAPTURE_COLUMNS:   # (bit for bit: the doubles compared as integers, so -0.0 and NaN payloads count)
            x, y = getattr(a[name], column), getattr(b[name], column)
            assert x.dtype == y.dtype and np.array_equal(np.ascontiguousarray(x).view(np.int64 if x.dtype.itemsize == 8 else np.int32),
                                                         np.ascontiguousarray(y).view(np.int64 if y.dtype.itemsize == 8 else np.int32)), (name, column)


def edge_slab(capacity=BIG):
    """The Lumogen slab: one facet recorder per edge that hears luminescence only, `lost`, and `exit` on the root."""
    scene = scenes.lsc_equivalent(recorders=False)
    slab = node(scene, "LSC")
    slab.recorders = [Recorder(f"edge-{label}", event="escaping", facet=normal, source="components", capture=capacity)
                      for label, normal in EDGES.items()]
    slab.recorders += [Recorder("lost", event="lost", capture=capacity), Recorder("entering", event="entering")]
    scene.root.recorders = [Recorder("exit", event="exit", capture=capacity)]
    return scene


def slab():
    return edge_slab(), None


def node_grid():
    scene = scenes.tiles6()       # 82 recorders: the four-word first-crossing mask, the node grid's walk
    captured = 0
    for n in scene.root.preorder():
        for rec in getattr(n, "recorders", []):
            if rec.name in GRID_CAPTURED:
                rec.capture = 1 << 14
                captured += 1
    assert captured == len(GRID_CAPTURED) == 37
    return scene, None


def mesh():
    scene = scenes.mesh_lsc()
    for rec in node(scene, "LSC").recorders:
        if rec.name in ("top", "bottom", "right", "lost", "entering", "reflected"):
            rec.capture = BIG
    return scene, None


def rough_field_map():
    scene, rays = rough_fielded_block()
    body = node(scene, "block")
    body.recorders = [Recorder("in", event="entering", capture=BIG), Recorder("out", event="escaping", capture=BIG),
                      Recorder("glow-out", event="escaping", source="lum", capture=BIG),
                      Recorder("lost-rays", event="lost", capture=BIG), Recorder("bounce", event="reflected", capture=BIG)]
    assert len(body.volume_maps) == 3
    return scene, rays


def device_emission():
    return edge_slab(), "device"


# the recorders of the tile array to which the referee alone (the CPU oracle on these rays and this seed) gives a few
# hundred rows each: every tile's `escaping` (316 ... 456 rows) and the middle tile's `entering` (615), by their names
GRID_CAPTURED = frozenset({f"escaping-{row}-{col}" for row in range(6) for col in range(6)} | {"entering"})
EXACT_SCENES = {"slab": slab, "node_grid": node_grid, "mesh": mesh, "rough_field_map": rough_field_map,
                "device_emission": device_emission}
N_RAYS = 16384


# -- 1-3. the kernel's rows against the event log, exactly ---------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(EXACT_SCENES))
def test_captured_rows_equal_the_first_matches_of_the_event_log(name):
    scene, rays = EXACT_SCENES[name]()
    hist, tally = history_launch(scene, rays, n=N_RAYS if rays is None or isinstance(rays, str) else 8192)
    kernel = hist.captures
    referee = capture_histories(scene, hist.histories())
    compiled = compile_scene(scene)
    assert sorted(kernel) == sorted(r.name for r in compiled.recorder_specs if r.capture) and kernel
    for rec_name, rows in referee.items():
        print(name, rec_name, len(rows))
        assert len(rows) >= 200, (name, rec_name, len(rows))    # the referee alone: no empty or near-empty recorder
    same_captures(kernel, referee)
    for rec_name, rows in kernel.items():                          # 2. the rays behind the `rays` count, all of them
        assert rows.matched == hist.recorders[rec_name].rays == len(rows) and rows.dropped == 0, rec_name
        assert np.all(np.diff(rows.index) > 0) and rows.index[0] >= 0 and rows.index[-1] < hist.num_rays
    same_captures(kernel, tally.captures)                          # 3. a tally-only launch of the same rays and seed
    for rec_name, rows in tally.captures.items():
        assert rows.matched == tally.recorders[rec_name].rays
    if name in ("slab", "device_emission"):
        assert all(np.all(kernel[f"edge-{e}"].source >= 0) for e in EDGES) and np.all(kernel["exit"].index >= 0)
        assert np.allclose(np.abs(kernel["edge-right"].position[:, 0]), 2.5) and np.all(kernel["edge-left"].direction[:, 0] < 0)
    assert native_variant(scene) == "rough"


def native_variant(scene):
    with Session(scene, emission="host") as s:
        rays = (np.tile((0.1, 0.2, 3.0), (64, 1)), np.tile((0.0, 0.0, -1.0), (64, 1)), np.full(64, 555.0))
        submit(s, rays, 1, record_every=0)
        return s.dscene.launch_info()["variant"]


def test_a_scene_without_captures_runs_the_variant_it_ran_before():
    assert native_variant(scenes.lsc_equivalent()) in ("lean", "w4")
    assert native_variant(scenes.tiles6()) == "grid"
    assert simulate(scenes.lsc_equivalent(), 1000, seed=1, record_every=0).captures == {}


# -- 4-6. the launch does not matter -----------------------------------------------------------------------------------------
def test_carried_launches_streams_shards_and_a_ray_alone_give_the_same_rows():
    scene = edge_slab()
    n, seed, emit_seed = 1_000_000, 13, 21
    whole = simulate(scene, n, seed=seed, record_every=0, emission="device", emit_seed=emit_seed).captures
    assert all(len(rows) > 10_000 and rows.dropped == 0 for rows in whole.values())
    # carried launches: three bundles on a pipeline whose launches hand their live photons on
    for depth in (1, 2):
        compiled, data, _ = trace_stream(scene, n, n // 3 + 1, seed, emit_seed=emit_seed, depth=depth)
        same_captures(whole, data["captures"])   # (`BundlePipeline.captures_host` of the job's pipeline)
        for r, rec_name in enumerate(compiled.recorder_names):
            if rec_name in whole:
                assert whole[rec_name].matched == int(data["rec_distinct"][r])
    # a stream of 20 bundles, one set of captures per bundle (tally sets of grouped launches), global indices
    parts = []
    for result, traced in simulate_stream(scene, n, bundle=50_000, seed=seed, record_every=0, emission="device",
                                          emit_seed=emit_seed):
        for rows in result.captures.values():
            assert len(rows) == 0 or (rows.index[0] >= traced - result.num_rays and rows.index[-1] < traced)
        parts.append(result.captures)
    assert len(parts) == 20
    from pvtrace_amd.engine.api import merge_captures

    same_captures(whole, merge_captures(parts))
    # 5. two shards on one device
    same_captures(whole, simulate(scene, n, seed=seed, record_every=0, emission="device", emit_seed=emit_seed,
                                  devices=[0, 0]).captures)
    # 6. a ray alone (a launch of one photon finishes in the tail function) and the rest around it
    with Session(scene, emission="device") as s:
        for i in (0, int(whole["edge-left"].index[7]), int(whole["lost"].index[-1]), n - 1):
            pieces = [s.collect(s.submit(b - a, seed, record_every=0, emit_seed=emit_seed, ray_offset=a)).captures
                      for a, b in ((0, i), (i, i + 1), (i + 1, n)) if b > a]
            same_captures(whole, merge_captures(pieces))


def test_a_host_emitted_stream_reports_global_indices():
    scene = edge_slab()
    n = 200_000
    parts = []
    for result, traced in simulate_stream(scene, n, bundle=50_000, seed=5, record_every=0, emission="host", emit_seed=9):
        parts.append(result.captures)
        assert all(len(rows) > 0 and rows.index[0] >= traced - result.num_rays and rows.index[-1] < traced
                   for rows in result.captures.values())
    assert len(parts) == 4


# -- 7. existing behaviour ---------------------------------------------------------------------------------------------------
def test_capture_changes_neither_tallies_nor_maps_nor_histories():
    def build(capacity):
        scene = edge_slab(capacity)
        node(scene, "LSC").volume_maps = [VolumeMap("dose", (8, 8, 4), (-2.5, -2.5, -0.5), (2.5, 2.5, 0.5))]
        return scene

    plain, captured = build(None), build(BIG)
    assert not compile_scene(plain).has_captures
    pos, dirs, wl, _ = emit_bundle(plain, 200_000, seed=3)
    out = []
    for scene in (plain, captured):
        with Session(scene, emission="host") as s:
            h = submit(s, (pos[:20_000], dirs[:20_000], wl[:20_000]), 7, record_every=1, max_events=64)
            t = submit(s, (pos, dirs, wl), 7, record_every=0)
            out.append(({k: np.asarray(h.data[k]).copy() for k in HIST_KEYS + TALLY_KEYS + ("map_bins",)},
                        {k: np.asarray(t.data[k]).copy() for k in TALLY_KEYS + ("map_bins", "rec_sums")}))
    for k in HIST_KEYS + TALLY_KEYS + ("map_bins",):
        assert np.array_equal(out[0][0][k], out[1][0][k]), k
    for k in TALLY_KEYS + ("map_bins",):
        assert np.array_equal(out[0][1][k], out[1][1][k]), k
    # (the moment sums are floating-point atomics: the same addends in whatever order the waves arrive, run to run)
    assert np.allclose(out[0][1]["rec_sums"], out[1][1]["rec_sums"], rtol=1e-12, atol=0)


# -- 8. overflow -----------------------------------------------------------------------------------------------------------------
def test_overflow_keeps_capacity_rows_all_of_them_rows_of_the_full_capture():
    n, seed, emit_seed, capacity = 200_000, 3, 4, 1000
    full = simulate(edge_slab(), n, seed=seed, record_every=0, emission="device", emit_seed=emit_seed)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        short = simulate(edge_slab(capacity), n, seed=seed, record_every=0, emission="device", emit_seed=emit_seed)
    messages = [str(w.message) for w in caught if "capture capacity" in str(w.message)]
    assert len(messages) == len(short.captures) and len(set(messages)) == len(messages)     # once per recorder
    for name, rows in short.captures.items():
        whole = full.captures[name]
        rays = short.recorders[name].rays
        assert rays == whole.matched == rows.matched > capacity
        assert len(rows) == capacity == rows.capacity and rows.dropped == rays - capacity
        assert len(np.unique(rows.index)) == capacity
        at = np.searchsorted(whole.index, rows.index)
        assert np.array_equal(whole.index[at], rows.index)
        for column in CAPTURE_COLUMNS:
            assert np.array_equal(getattr(whole, column)[at], getattr(rows, column)), (name, column)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        simulate(edge_slab(), 10_000, seed=seed, record_every=0, emission="device", emit_seed=emit_seed)   # no overflow: silent


# -- the packer --------------------------------------------------------------------------------------------------------------------
def test_the_packer_refuses_each_malformed_capture_table_with_its_own_message():
    compiled = compile_scene(edge_slab())
    lib = native.load_library()
    st, keep = native.scene_tables_struct(compiled)
    R = len(compiled.recorder_names)

    def attempt(n_recorders=R, **change):
        tabs = {"rec_capture_capacity": np.arange(R, dtype=np.int64), "capture_rows": R * (R - 1) // 2}
        tabs["rec_capture_start"] = np.concatenate([[0], np.cumsum(tabs["rec_capture_capacity"])[:-1]]).astype(np.int64)
        tabs.update(change)
        ct = native.PvtCaptureTables()
        ct.n_recorders, ct.capture_rows = n_recorders, int(tabs.pop("capture_rows"))
        held = {k: np.ascontiguousarray(v, dtype=np.int64) for k, v in tabs.items() if v is not None}
        for key, value in held.items():
            setattr(ct, key, native.np_ptr(value))
        handle = C.c_void_p()
        rc = lib.pvt_scene_create_capture(C.byref(st), None, None, None, None, None, C.byref(ct), 0, C.byref(handle))
        if rc == 0:
            rows = lib.pvt_scene_capture_rows(handle)
            lib.pvt_scene_destroy(handle)
            return rows
        assert not handle.value
        return lib.pvt_last_error().decode()

    assert attempt() == R * (R - 1) // 2
    big = np.zeros(R, dtype=np.int64)
    big[:2] = 1 << 23, (1 << 23) + 1
    bad = {
        "recorders": dict(n_recorders=R + 1),
        "missing": dict(rec_capture_start=None),
        "negative": dict(rec_capture_capacity=np.array([-1] + [0] * (R - 1)), rec_capture_start=np.zeros(R), capture_rows=-1),
        "start": dict(rec_capture_start=np.ones(R)),
        "total": dict(capture_rows=R * (R - 1) // 2 + 1),
        "limit": dict(rec_capture_capacity=big, rec_capture_start=np.concatenate([[0], np.cumsum(big)[:-1]]), capture_rows=int(big.sum())),
    }
    messages = {}
    for what, change in bad.items():
        msg = attempt(**change)
        assert isinstance(msg, str) and "capture tables" in msg, (what, msg)
        messages[what] = msg
    assert len(set(messages.values())) == len(messages), messages
    handle = C.c_void_p()   # no captures: exactly pvt_scene_create_maps
    assert lib.pvt_scene_create_capture(C.byref(st), None, None, None, None, None, None, 0, C.byref(handle)) == 0
    assert lib.pvt_scene_capture_rows(handle) == 0
    lib.pvt_scene_destroy(handle)


# -- 9. the example ----------------------------------------------------------------------------------------------------------------
def test_ray_chain_example_feeds_the_second_stage_with_the_captured_rays():
    spec = importlib.util.spec_from_file_location("ray_chain", os.path.join(ROOT, "examples", "ray_chain.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    out = module.main(photons=200_000)
    edge = out["captured"]
    assert len(edge) > 1000 and edge.dropped == 0
    pos, dirs, wl = out["second_stage_input"]
    assert np.array_equal(pos, edge.position) and np.array_equal(dirs, edge.direction) and np.array_equal(wl, edge.wavelength)
    assert 0 < out["cell"] <= len(edge) and out["cell"] + out["missed"] <= len(edge)
