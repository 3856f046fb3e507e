"""Absorbing coatings (`Coating(..., absorptivity=...)`) and `detected` recorders on the GPU.  The reference has no such
coating, so the feature is held by (a) the rule's closed forms, (b) the host tracer, (c) the kernel's own event log refereed
on the host (`tally_histories`, `capture_histories`, `map_histories`), and (d) itself: A = 0 against no absorptivity, and one
launch against the same rays launched every other way.  Layouts: (s1) a coated box in a world, (s2) a 37-node tile array
on the node grid with absorbing inner faces, (s3) a mesh beside a coated box (tests/absorbing_scenes.py)."""
import ctypes as C
import importlib.util
import math
import os

import numpy as np
import pytest

from pvtrace_amd import Coating, Event, Ray, VolumeMap, photon_tracer
from pvtrace_amd.engine import (
    Recorder, Session, _kernel, capture_histories, compile_scene, map_histories, native, simulate, simulate_stream,
    tally_histories, trace_stream,
)
from pvtrace_amd.engine.api import merge_captures
from pvtrace_amd.engine.compiler import UnsupportedSceneError
from pvtrace_amd.engine.emit import emit_bundle
from tests import absorbing_scenes as S
from tests.capture_scenes import history_launch, node, submit
from tests.test_gpu_coating_tables import two_sample_sigmas
from tests.test_gpu_ray_capture import same_captures

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 1 << 16
TALLY_KEYS = ("rec_distinct", "rec_crossings", "rec_bins")
HIST_KEYS = ("counts", "kind", "hit", "container", "adjacent", "component", "source", "position", "direction", "normal",
             "wavelength", "travelled", "duration")
SIZES = (1, 64, 20_000)     # the tail function alone; one wave; several workgroups with refill


def variant(session):
    return session.dscene.launch_info()["variant"]


def launches(scene, rays, seed=7, max_events=256):
    """The history launch and the tally launch of the same rays -> (columns, tallies, variant)."""
    with Session(scene, emission="host") as s:
        h = submit(s, rays, seed, record_every=1, max_events=max_events)
        t = submit(s, rays, seed, record_every=0)
        assert int(np.asarray(h.data["counts"]).max()) < max_events
        return ({k: np.asarray(h.data[k]).copy() for k in HIST_KEYS + TALLY_KEYS},
                {k: np.asarray(t.data[k]).copy() for k in TALLY_KEYS + ("rec_sums",)}, variant(s))


def rays_of(scene, n, seed=3):
    pos, dirs, wl, _ = emit_bundle(scene, n, seed=seed)
    return pos, dirs, wl


# -- 1. A = 0 is no absorptivity, bit for bit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("layout", sorted(S.LAYOUTS))
def test_zero_absorptivity_traces_bit_for_bit_as_none(layout, n):
    build = S.LAYOUTS[layout]
    rays = rays_of(build(absorptivity=None), n)
    none_h, none_t, none_v = launches(build(absorptivity=None), rays)
    for zero in (0.0, "zero"):     # the scalar (the library proves it changes nothing), tables of zeros (the extension variants)
        h, t, v = launches(build(absorptivity=zero), rays)
        for k in HIST_KEYS + TALLY_KEYS:
            assert np.array_equal(h[k], none_h[k], equal_nan=h[k].dtype.kind == "f"), (layout, zero, k)
        for k in TALLY_KEYS:
            assert np.array_equal(t[k], none_t[k]), (layout, zero, k)
        assert np.allclose(t["rec_sums"], none_t["rec_sums"], rtol=1e-12, atol=0)
        assert v == ("rough" if zero == "zero" else none_v), (layout, zero, v)
    # (s1: `none` above is the launch the plain variants trace; a mesh scene runs the mesh family, the tiles the grid's)
    assert none_v == {"s1": "w4", "s2": "grid", "s3": "mesh"}[layout]
    assert not np.any(none_h["kind"] == Event.DETECT.value)
    if n > 1000:
        assert np.sum(none_h["kind"] == Event.REFLECT.value) > 100


# -- 2. the kernel against the host referee on its own histories ----------------------------------------------------------------------
@pytest.mark.parametrize("layout", sorted(S.LAYOUTS))
def test_kernel_tallies_captures_and_maps_equal_the_referee_on_the_event_log(layout):
    scene = S.LAYOUTS[layout](capture=BIG)
    mapped = node(scene, {"s1": "LSC", "s2": "tile-2-3", "s3": "LSC"}[layout])
    mapped.volume_maps = [VolumeMap("dose", (4, 4, 2), (-2.5, -2.5, -0.5), (2.5, 2.5, 0.5))]
    hist, tally = history_launch(scene, None, n=8192)
    histories = list(hist.histories())
    referee = tally_histories(scene, histories)
    detected = 0
    for name, rec in hist.recorders.items():
        want = referee[name]
        assert (rec.rays, rec.crossings) == (want.rays, want.crossings) == (tally.recorders[name].rays, tally.recorders[name].crossings), name
        for i in range(len(rec.spec.histograms)):
            assert np.array_equal(rec._bins[i], want._bins[i]) and np.array_equal(rec._bins[i], tally.recorders[name]._bins[i]), (name, i)
        assert np.allclose(rec._moments, want._moments, rtol=1e-9), name
        if rec.spec.event == "detected":
            assert rec.rays == rec.crossings     # a photon is detected once
            detected += rec.rays
    print(layout, "detected", detected, {k: v.rays for k, v in hist.recorders.items() if v.rays})
    assert detected > 200
    ends = [h[-1][1] for h in histories]
    assert sum(e == Event.DETECT for e in ends) == sum(e == Event.DETECT for h in histories for _, e, _ in h) > 200   # terminal
    captured = capture_histories(scene, histories)
    assert captured and all(scene_rec.event == "detected" for scene_rec in compile_scene(scene).recorder_specs if scene_rec.capture)
    same_captures(hist.captures, captured)
    same_captures(hist.captures, tally.captures)
    assert sum(len(rows) for rows in captured.values()) > 200
    # the map is what the histories say, and what the same scene without the coatings' absorptivity... cannot say: the
    # photons differ; what must hold is the referee's count of THIS log
    kernel_maps, referee_maps = hist.volume_maps, map_histories(scene, histories)
    assert np.array_equal(kernel_maps["dose"].counts, referee_maps["dose"].counts) and kernel_maps["dose"].outside == referee_maps["dose"].outside
    assert np.array_equal(kernel_maps["dose"].counts, tally.volume_maps["dose"].counts) and kernel_maps["dose"].total > 0


def test_rays_that_meet_no_absorbing_face_keep_their_histories_and_their_map_counts():
    """The slab with and without absorbing edges, the same rays and seed, both on the extension variants (a volume map):
    a ray that never meets an edge draws what it drew, so its history is the same row for row -- with UF_CABS on and the
    absorptivity looked up at no point of it."""
    def build(absorptivity):
        scene = S.s1_slab(absorptivity=absorptivity, mirror=False)
        node(scene, "LSC").volume_maps = [VolumeMap("dose", (5, 5, 2), (-2.5, -2.5, -0.5), (2.5, 2.5, 0.5))]
        return scene

    n = 4096
    rays = rays_of(build(None), n)
    out = []
    for a in (None, "table"):
        with Session(build(a), emission="host") as s:
            out.append(list(submit(s, rays, 5, record_every=1, max_events=256).histories()))
            assert variant(s) == "rough"
    plain, coated = out

    def meets_an_edge(history):
        return any(m.get("normal") is not None and m["hit"] == "LSC" and abs(m["normal"][2]) < 0.5 for _, _, m in history)

    same = [j for j, h in enumerate(plain) if not meets_an_edge(h)]
    assert n // 4 < len(same) < n
    for j in same:
        assert plain[j] == coated[j], j
    assert any(e == Event.DETECT for h in coated for _, e, _ in h)


# -- 3. the laws -------------------------------------------------------------------------------------------------------------------------
N_LAW = 200_000


def pencil(start, direction, wavelength, n=N_LAW):
    return np.tile(start, (n, 1)), np.tile(direction, (n, 1)), np.full(n, float(wavelength))


def first_outcomes(scene, rays, seed):
    """(reflected, detected, entered or escaped) of a pencil's FIRST surface event, from recorders: maxsteps = 1."""
    with Session(scene, emission="host") as s:
        r = s.collect(s.submit(len(rays[2]), seed, host_rays=(*rays, ["r"] * len(rays[2])), record_every=0, maxsteps=1))
        assert variant(s) == "rough"
    rec = r.recorders
    return rec["reflected"].rays, rec["detected"].rays, rec["entering"].rays + rec["escaping"].rays, rec


def test_three_way_split_on_the_gpu():
    scene = S.coated_box([Coating(S.TOP, reflectivity=0.3, absorptivity=0.5)])
    reflected, detected, through, rec = first_outcomes(scene, pencil(*S.pencil_from_above(), 555.0), seed=11)
    print("three-way", reflected, detected, through)
    assert reflected + detected + through == N_LAW
    assert S.five_sigma(reflected, N_LAW, 0.3) and S.five_sigma(detected, N_LAW, 0.5) and S.five_sigma(through, N_LAW, 0.2)
    edges, bins = rec["detected"].histogram(0)
    assert bins[0] == detected        # normal incidence: angle 0


def test_table_cells_on_the_gpu_at_two_wavelengths():
    scene = S.coated_box([Coating(S.TOP, absorptivity=S.step_table())])
    for k, ((wl, angle), a) in enumerate(S.STEP_CELLS.items()):
        reflected, detected, through, _ = first_outcomes(scene, pencil(*S.pencil_from_above(math.radians(angle)), wl), seed=20 + k)
        print("cell", wl, angle, detected, through)
        assert reflected == 0 and detected + through == N_LAW
        assert S.five_sigma(detected, N_LAW, a) and S.five_sigma(through, N_LAW, 1.0 - a)
    # an interior point: bilinear, A(550 nm, 40 degrees) = 0.5
    reflected, detected, through, _ = first_outcomes(scene, pencil(*S.pencil_from_above(math.radians(40.0)), 550.0), seed=29)
    assert S.five_sigma(detected, N_LAW, 0.5) and detected + through == N_LAW


def test_total_internal_reflection_and_clipping_on_the_gpu():
    theta = math.radians(60.0)
    inside = pencil(*S.pencil_from_inside(theta), 555.0)
    # (a reflection off the INSIDE of the box fires no `reflected` recorder: that selector is owned by the far side)
    scene = S.coated_box([Coating(S.TOP, reflectivity=0.0, absorptivity=1.0)], n_box=1.5)
    reflected, detected, through, _ = first_outcomes(scene, inside, seed=31)
    assert (detected, through) == (0, 0)
    with Session(scene, emission="host") as s:
        r = s.collect(s.submit(1000, 31, host_rays=(*(a[:1000] for a in inside), ["r"] * 1000), record_every=1, maxsteps=1, max_events=8))
    assert all([e for _, e, _ in h] == [Event.GENERATE, Event.REFLECT, Event.KILL] for h in r.histories())
    scene = S.coated_box([Coating(S.TOP, reflectivity=0.0, absorptivity=1.0, transmission="matched")], n_box=1.5)
    reflected, detected, through, _ = first_outcomes(scene, inside, seed=32)
    assert (reflected, detected, through) == (0, N_LAW, 0)
    # clipping: Fresnel R at 80 degrees from air into glass, A = 1: the rest is detected, nothing transmitted
    theta = math.radians(80.0)
    r80 = S.fresnel_r(theta, 1.0, 1.5)
    scene = S.coated_box([Coating(S.TOP, absorptivity=1.0)], n_box=1.5)
    reflected, detected, through, _ = first_outcomes(scene, pencil(*S.pencil_from_above(theta), 555.0), seed=33)
    print("clipping", reflected, detected, through, r80)
    assert S.five_sigma(reflected, N_LAW, r80) and detected == N_LAW - reflected and through == 0


# -- 4. host == GPU ------------------------------------------------------------------------------------------------------------------------
def test_host_tracer_and_gpu_agree_on_the_shares_of_the_cell_slab():
    scene = S.s1_slab()
    names = [f"cell-{e}" for e in S.EDGES] + ["mirror", "exit", "lost"]
    n_gpu, n_host = 200_000, 3000
    gpu = simulate(scene, n_gpu, seed=5, record_every=0, emission="host").recorders
    p_gpu = np.array([gpu[k].rays for k in names], dtype=float) / n_gpu
    np.random.seed(12)
    histories = [list(photon_tracer.step_forward(scene, ray, backend="host")) for ray in scene.emit(n_host)]
    host = tally_histories(scene, histories)
    p_host = np.array([host[k].rays for k in names], dtype=float) / n_host
    z = two_sample_sigmas(p_gpu, n_gpu, p_host, n_host)
    print(dict(zip(names, zip(p_gpu.round(4), p_host.round(4), z.round(2)))))
    assert np.all(z < 5.0), dict(zip(names, z))
    assert abs(p_gpu.sum() - 1.0) < 1e-3 and p_gpu[:4].min() > 0.02 and p_gpu[4] > 0.005


# -- 5. every ray ends once ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", sorted(S.LAYOUTS))
def test_every_ray_ends_in_exactly_one_terminal_recorder(layout):
    scene = S.LAYOUTS[layout]()
    if layout == "s3":     # (`panel-any` hears what `panel-left` hears: one listener per terminal)
        panel = node(scene, "panel")
        panel.recorders = [r for r in panel.recorders if r.name != "panel-left"]
    n = 100_000
    r = simulate(scene, n, seed=3, record_every=0).recorders
    ends = {name: rec.rays for name, rec in r.items()
            if rec.spec.event in ("detected", "exit", "lost", "reacted", "killed")}
    print(layout, {k: v for k, v in ends.items() if v})
    assert sum(ends.values()) == n
    assert sum(v for k, v in ends.items() if r[k].spec.event == "detected") > n // 50


# -- 6. the launch does not matter -----------------------------------------------------------------------------------------------------------
def test_a_ray_alone_carried_launches_sets_emission_and_shards_give_the_same_tallies_and_rows():
    scene = S.s1_slab(capture=BIG)
    n, seed, emit_seed = 200_000, 13, 21
    whole = simulate(scene, n, seed=seed, record_every=0, emission="device", emit_seed=emit_seed)
    assert all(rows.dropped == 0 for rows in whole.captures.values()) and sum(len(r) for r in whole.captures.values()) > 10_000

    def same_tallies(data):
        for k in TALLY_KEYS:
            assert np.array_equal(np.asarray(data[k]), np.asarray(whole.data[k])), k

    for depth in (1, 2):     # carried launches
        compiled, data, _ = trace_stream(scene, n, n // 3 + 1, seed, emit_seed=emit_seed, depth=depth)
        same_captures(whole.captures, data["captures"])
        same_tallies(data)
    parts, totals = [], None     # a stream of tally sets
    for result, _ in simulate_stream(scene, n, bundle=25_000, seed=seed, record_every=0, emission="device", emit_seed=emit_seed):
        parts.append(result.captures)
        block = {k: np.asarray(result.data[k]).astype(np.int64) for k in TALLY_KEYS}
        totals = block if totals is None else {k: totals[k] + block[k] for k in TALLY_KEYS}
    same_captures(whole.captures, merge_captures(parts))
    same_tallies(totals)
    sharded = simulate(scene, n, seed=seed, record_every=0, emission="device", emit_seed=emit_seed, devices=[0, 0])
    same_captures(whole.captures, sharded.captures)
    same_tallies(sharded.data)
    with Session(scene, emission="device") as s:     # a ray alone (the tail function) and the rest around it
        for i in (0, int(whole.captures["cell-left"].index[5]), int(whole.captures["mirror"].index[-1]), n - 1):
            pieces = [s.collect(s.submit(b - a, seed, record_every=0, emit_seed=emit_seed, ray_offset=a))
                      for a, b in ((0, i), (i, i + 1), (i + 1, n)) if b > a]
            same_captures(whole.captures, merge_captures([p.captures for p in pieces]))
            same_tallies({k: sum(np.asarray(p.data[k]).astype(np.int64) for p in pieces) for k in TALLY_KEYS})


@pytest.mark.parametrize("tables", ["heads", "global"])
def test_absorptivity_tables_read_from_global_memory_give_the_same_result(tables, monkeypatch):
    scene = S.s1_slab(capture=BIG)
    rays = rays_of(scene, 20_000)
    want_h, want_t, _ = launches(scene, rays)
    with Session(scene, emission="host") as s:
        want_rows = submit(s, rays, 7, record_every=0).captures
    monkeypatch.setenv("PVT_TABLES", tables)
    got_h, got_t, v = launches(scene, rays)
    with Session(scene, emission="host") as s:
        got_rows = submit(s, rays, 7, record_every=0).captures
    monkeypatch.delenv("PVT_TABLES")
    assert v == "rough" and np.sum(want_h["kind"] == Event.DETECT.value) > 1000
    for k in HIST_KEYS + TALLY_KEYS:
        assert np.array_equal(got_h[k], want_h[k], equal_nan=got_h[k].dtype.kind == "f"), (tables, k)
    for k in TALLY_KEYS:
        assert np.array_equal(got_t[k], want_t[k]), (tables, k)
    same_captures(got_rows, want_rows)


# -- 7. the packer and the entries -------------------------------------------------------------------------------------------------------
def test_the_packer_refuses_each_malformed_absorb_table_with_its_own_message():
    scene = S.coated_box([Coating(S.TOP, reflectivity=0.3, absorptivity=0.5), Coating((1, 0, 0), absorptivity=S.step_table())])
    compiled = compile_scene(scene)
    lib = native.load_library()
    st, keep = native.scene_tables_struct(compiled)

    def attempt(change=None):
        # the struct points into the CompiledScene's own arrays, so each attempt pokes a scene compiled for it alone
        at, akeep = native.absorb_tables_struct(compile_scene(scene))
        if change is not None:
            change(at, akeep)
        handle = C.c_void_p()
        rc = lib.pvt_scene_create_absorb(C.byref(st), None, None, None, None, None, None, C.byref(at), 0, C.byref(handle))
        if rc == 0:
            lib.pvt_scene_destroy(handle)
            return None
        assert rc == -1 and not handle.value
        return lib.pvt_last_error().decode()

    def poke(name, index, value):
        def change(at, akeep):
            akeep[name][index] = value
        return change

    def count(at, akeep):
        at.n_coatings = 3

    assert attempt() is None
    messages = {"count": attempt(count), "nan": attempt(poke("coat_absorptivity", 0, float("nan"))),
                "range": attempt(poke("coat_absorptivity", 0, 1.5)), "descending": attempt(poke("wavelength", 1, 400.0)),
                "angle": attempt(poke("angle", 1, 10.0)), "value": attempt(poke("value", 2, 1.25)),
                "size": attempt(poke("table_nw", 0, 3)), "names": attempt(poke("coat_table", 1, 5))}
    assert all(isinstance(m, str) and "absorb tables" in m for m in messages.values()), messages
    assert len(set(messages.values())) == len(messages), messages
    assert "one absorptivity per coating" in messages["count"] and "finite" in messages["nan"] and "[0, 1]" in messages["range"]
    assert "strictly increasing" in messages["descending"]


def test_host_buffer_entry_refuses_and_a_null_struct_is_create_capture():
    absorbing = S.s1_slab()
    with pytest.raises(UnsupportedSceneError, match="absorbing coatings"):
        _kernel.trace_bundle(compile_scene(absorbing), *rays_of(absorbing, 16), 1, 100, 16, 0, 1, 0)
    # pvt_scene_create_absorb with a NULL struct (and with every A zero) builds the scene pvt_scene_create_capture builds
    # (without the `detected` recorders: pvt_scene_create_absorb alone knows their selector, the older entries refuse it)
    scene = S.s1_slab(absorptivity=None)
    slab = node(scene, "LSC")
    slab.recorders = [r for r in slab.recorders if r.event != "detected"]
    compiled = compile_scene(scene)
    lib = native.load_library()
    st, keep = native.scene_tables_struct(compiled)
    handle = C.c_void_p()
    st7, keep7 = native.scene_tables_struct(compile_scene(S.s1_slab(absorptivity=None)))
    assert lib.pvt_scene_create_capture(C.byref(st7), None, None, None, None, None, None, 0, C.byref(handle)) == -1
    assert lib.pvt_last_error().decode() == "recorder selector out of range" and not handle.value
    pos, dirs, wl = rays_of(scene, 4096)
    zeros = native.PvtCoatingAbsorbTables()
    zeros.n_coatings = compiled.n_coatings
    a0 = np.zeros(compiled.n_coatings)
    zeros.coat_absorptivity = native.np_ptr(a0)
    results = []
    for create, extra in ((lib.pvt_scene_create_capture, ()), (lib.pvt_scene_create_absorb, (None,)),
                          (lib.pvt_scene_create_absorb, (C.byref(zeros),))):
        handle = C.c_void_p()
        assert create(C.byref(st), None, None, None, None, None, None, *extra, 0, C.byref(handle)) == 0
        dscene = native.DeviceScene.__new__(native.DeviceScene)
        dscene.lib, dscene.compiled, dscene.device, dscene.handle, dscene.has_emitter = lib, compiled, 0, handle, False
        import torch

        dev = torch.device("cuda", 0)
        tallies = dscene.new_tallies()
        rays = tuple(torch.as_tensor(np.ascontiguousarray(a), device=dev) for a in (pos, dirs, wl))
        dscene.trace(rays, len(wl), 9, tallies)
        torch.cuda.synchronize(0)
        results.append(({k: np.asarray(v).copy() for k, v in tallies.host(0).items() if k in TALLY_KEYS}, dscene.launch_info()["variant"]))
        dscene.close()
    for got, v in results[1:]:
        assert v == results[0][1] == "w4"
        for k in TALLY_KEYS:
            assert np.array_equal(got[k], results[0][0][k]), k
    assert int(results[0][0]["rec_distinct"].sum()) > 0


# -- 8. the example ---------------------------------------------------------------------------------------------------------------------
def test_edge_cells_example_accounts_for_every_photon():
    spec = importlib.util.spec_from_file_location("edge_cells", os.path.join(ROOT, "examples", "edge_cells.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    out = module.main(photons=100_000)
    shares = out["shares"]
    assert abs(sum(shares.values()) - 1.0) < 1e-12 and shares["detected"] > 0.05 and shares["mirror"] > 0.0
    assert shares["escaped"] > 0.0 and out["photons"] == 100_000
