"""Launch origin as histogram properties on the GPU.  The referee is the kernel's own event log: one launch with
`record_every=1` gives both the kernel's recorders and every ray's history, and `tally_histories` bins the FIRST row's
wavelength and position at each ray's first match on the host.  Integers: every bin, `rays` and `crossings` is compared
exactly.  Then the origins are held to the launch arrays themselves (exact conservation over the terminal recorders), to
themselves (carried launches, streams, shards, a ray alone), to the scene without them (no side effect), to the
Beer-Lambert law per launch wavelength and to the refusals of the C ABI."""
import ctypes as C
import functools
import importlib.util
import math
import os

import numpy as np
import pytest

from pvtrace_amd import Distribution, Light, VolumeMap, cone
from pvtrace_amd.engine import (
    Heatmap, Histogram, Recorder, Session, compile_scene, native, simulate, simulate_stream, tally_histories, trace_stream,
)
from pvtrace_amd.engine.compiler import UnsupportedSceneError
from pvtrace_amd.engine.emit import emit_bundle
from pvtrace_amd.engine.tally import _Probe
from pvtrace_amd.light import RectangularMask, SpectrumWavelengthMask
from tests import scenes
from tests.capture_scenes import history_launch, node, submit
from tests.test_gpu_history_counters import (
    BIG, HIST_KEYS, N_RAYS, TALLY_KEYS, edge_slab, many_recorders, mesh, node_grid, rough_field_map_capture,
    same_captures, same_recorders, same_tallies, tallies_of,
)
from tests.test_origin_properties import beer_lambert_law, beer_lambert_rays, beer_lambert_slab

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WL_AXIS = (400.0, 800.0, 20)
XY_AXIS = (-20.0, 20.0, 40)


def origin_histograms():
    """A histogram of each origin, the issue's map, and the two heatmaps of the negative control: the launch value against
    the event's."""
    return [Histogram("origin_wavelength", 400, 800, 40), Histogram("origin_x", -20, 20, 160), Histogram("origin_y", -20, 20, 160),
            Histogram("origin_z", -6, 6, 24), Heatmap("origin_x", "origin_y", (-20, 20, 16), (-20, 20, 16)),
            Heatmap("origin_wavelength", "wavelength", WL_AXIS, WL_AXIS), Heatmap("origin_x", "x", XY_AXIS, XY_AXIS)]


def add_origins(scene, histograms=origin_histograms):
    """Every recorder of the scene gets the origin histograms behind its own."""
    for n in scene.root.preorder():
        for rec in getattr(n, "recorders", None) or []:
            rec.histograms = list(rec.histograms) + histograms()
    return scene


def spread_lamp(scene):
    """The scene's light becomes an area light with a spectrum: wavelengths over the dye's absorption band, positions over
    4 x 4 cm of the face, a narrow cone."""
    x = np.linspace(430.0, 630.0, 21)
    lamp = next(n for n in scene.root.preorder() if getattr(n, "light", None) is not None)
    lamp.light = Light(wavelength=SpectrumWavelengthMask(Distribution(x, 1.0 + 0.5 * np.sin(x / 30.0))),
                       position=RectangularMask(2.0, 2.0), direction=functools.partial(cone, np.radians(5.0)), name=lamp.light.name)
    return scene


def spread_rays(scene, rays, n, width=0.5):
    """Host rays of the scene's light (or the given ones) with the launch values spread: wavelengths over 440-640 nm, the
    starting points over a square of `width` centimetres around where they were."""
    if rays is None:
        pos, dirs, wl, _ = emit_bundle(scene, n, seed=3)
    else:
        pos, dirs, wl = (np.array(a[:n], dtype=np.float64, copy=True) for a in rays)
    k = np.arange(len(wl))
    pos = np.array(pos, dtype=np.float64, copy=True)
    pos[:, 0] += width * (((k * 0.6180339887498949) % 1.0) - 0.5)
    pos[:, 1] += width * (((k * 0.7548776662466927) % 1.0) - 0.5)
    return pos, np.asarray(dirs, dtype=np.float64), 440.0 + 200.0 * ((k * 0.5698402909980532) % 1.0)


def origin_only():
    """No counter, no capture: the scene reads two of the four origins and counts nothing."""
    scene = edge_slab(counters=False)
    return add_origins(scene, lambda: [Histogram("origin_wavelength", 400, 800, 40), Histogram("origin_y", -3, 3, 24),
                                       Heatmap("origin_wavelength", "wavelength", WL_AXIS, WL_AXIS),
                                       Heatmap("origin_y", "y", (-3, 3, 12), (-3, 3, 12))]), None


def slab():
    return add_origins(edge_slab()), None


def device_emission():
    return add_origins(spread_lamp(edge_slab(capture=BIG))), "device"


def with_origins(builder):
    def build():
        scene, rays = builder()
        return add_origins(scene), rays
    return build


EXACT_SCENES = {"slab": slab, "origin_only": origin_only, "node_grid": with_origins(node_grid), "mesh": with_origins(mesh),
                "many_recorders": with_origins(many_recorders),
                "rough_field_map_capture": with_origins(rough_field_map_capture), "device_emission": device_emission}


def off_diagonal(recorders, at, bins):
    """First matches whose launch value and event value fall into different bins of the same axis, over all recorders."""
    total = 0
    for rec in recorders.values():
        joint = np.asarray(rec._bins[len(rec._bins) + at]).reshape(bins, bins)
        total += int(joint.sum() - np.trace(joint))
    return total


# -- the kernel against its own log ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(EXACT_SCENES))
def test_the_kernels_origins_equal_its_own_event_log(name):
    scene, rays = EXACT_SCENES[name]()
    n = N_RAYS // 2 if name == "node_grid" else N_RAYS   # (82 probes per event on the host)
    if not isinstance(rays, str):
        # (a point light over a 5 x 5 cm face: spread over 4 x 4 cm of it; the tiles' light and the block's pencil: half a centimetre)
        rays = spread_rays(scene, rays, n, width=0.5 if name in ("node_grid", "rough_field_map_capture") else 4.0)
        assert len(np.unique(rays[2])) > n // 2 and len(np.unique(rays[0][:, 0])) > n // 2
    hist, tally = history_launch(scene, rays, n=n)
    histories = list(hist.histories())
    assert len({h[0][0].wavelength for h in histories}) > 100 and len({tuple(h[0][0].position) for h in histories}) > 100
    referee = tally_histories(scene, histories)
    same_recorders(hist.recorders, referee, (name, "history launch"))
    same_recorders(tally.recorders, referee, (name, "tally launch"))
    # the referee alone: a kernel that binned the photon's CURRENT wavelength / position would not pass -- some first matches
    # have another wavelength than the launch's (re-emission), and another x (y) than the launch's
    moved_wl, moved_x = off_diagonal(referee, -2, WL_AXIS[2]), off_diagonal(referee, -1, 12 if name == "origin_only" else XY_AXIS[2])
    matched = sum(int(rec._bins[-2].sum()) for rec in referee.values())
    print(name, "first matches binned", matched, "with another wavelength", moved_wl, "with another position", moved_x)
    assert moved_wl > 0 and moved_x > 0 and matched > moved_wl
    with Session(scene, emission="host") as s:
        dummy = (np.tile((0.1, 0.2, 3.0), (64, 1)), np.tile((0.0, 0.0, -1.0), (64, 1)), np.full(64, 555.0))
        submit(s, dummy, 1, record_every=0)
        assert s.dscene.launch_info()["variant"] == "rough"


# -- exact conservation ----------------------------------------------------------------------------------------------------------
TERMINAL = ("lost", "killed", "reacted", "detected")
CONS_WL = Histogram("origin_wavelength", 400.0, 700.0, 60)
CONS_XY = Heatmap("origin_x", "origin_y", (-2.5, 2.5, 10), (-2.5, 2.5, 10))


def test_the_terminal_recorders_origins_sum_to_the_launch_arrays_exactly():
    scene = spread_lamp(scenes.lsc_equivalent(recorders=False))
    fresh = lambda: [Histogram(CONS_WL.prop, CONS_WL.start, CONS_WL.stop, CONS_WL.bins),
                     Heatmap(CONS_XY.a.prop, CONS_XY.b.prop, (CONS_XY.a.start, CONS_XY.a.stop, CONS_XY.a.bins),
                             (CONS_XY.b.start, CONS_XY.b.stop, CONS_XY.b.bins))]
    names = []
    for n in scene.root.preorder():
        if n.geometry is None:
            continue
        n.recorders = [Recorder(f"{event}-{n.name}", event=event, histograms=fresh()) for event in TERMINAL]
        names += [rec.name for rec in n.recorders]
    scene.root.recorders = list(scene.root.recorders) + [Recorder("exit", event="exit", histograms=fresh())]
    names.append("exit")
    n = 200_000
    pos, dirs, wl, _ = emit_bundle(scene, n, seed=11)
    # the launch arrays alone, on the CPU: every value falls into a bin (the ranges cover the light), and not all into one
    iw = _Probe._bin_indices(wl, CONS_WL)
    ix, iy = _Probe._bin_indices(pos[:, 0], CONS_XY.a), _Probe._bin_indices(pos[:, 1], CONS_XY.b)
    assert iw.min() >= 0 and ix.min() >= 0 and iy.min() >= 0
    want_wl = np.bincount(iw, minlength=CONS_WL.bins)
    want_xy = np.bincount(ix * CONS_XY.b.bins + iy, minlength=CONS_XY.size)
    assert np.count_nonzero(want_wl) > 30 and np.count_nonzero(want_xy) > 60
    with Session(scene, emission="host") as s:
        result = submit(s, (pos, dirs, wl), 5, record_every=0)
    recs = [result.recorders[name] for name in names]
    assert sum(rec.rays for rec in recs) == n                      # every photon ends in exactly one of them
    assert result.recorders["exit"].rays > 0 and result.recorders["lost-LSC"].rays > 0
    assert np.array_equal(sum(np.asarray(rec._bins[0]) for rec in recs), want_wl)
    assert np.array_equal(sum(np.asarray(rec._bins[1]) for rec in recs), want_xy)


# -- the launch does not matter ------------------------------------------------------------------------------------------------
def test_carried_launches_streams_shards_and_a_ray_alone_give_the_same_origins():
    scene = add_origins(spread_lamp(edge_slab(capture=BIG)))          # counts too: the longest carry record and slot
    n, seed, emit_seed = 200_000, 13, 21
    result = simulate(scene, n, seed=seed, record_every=0, emission="device", emit_seed=emit_seed)
    whole, rows = tallies_of(result.data), result.captures
    deep = rows["edge-left"]
    assert all(r.dropped == 0 for r in rows.values()) and deep.emissions.max() >= 3
    left = result.recorders["edge-left"]
    assert np.count_nonzero(left._bins[-7]) > 10 and np.count_nonzero(left._bins[-6]) > 10 and off_diagonal({"edge-left": left}, -2, WL_AXIS[2]) > 0
    for depth in (1, 2):     # carried launches: three bundles on a pipeline whose launches hand their live photons on
        _, data, _ = trace_stream(scene, n, n // 3 + 1, seed, emit_seed=emit_seed, depth=depth)
        same_tallies(whole, tallies_of(data), ("carried", depth))
    total = None             # a stream of 8 bundles, one tally set per bundle
    for part, _ in simulate_stream(scene, n, bundle=25_000, seed=seed, record_every=0, emission="device", emit_seed=emit_seed):
        total = tallies_of(part.data) if total is None else {k: total[k] + np.asarray(part.data[k]) for k in TALLY_KEYS}
    same_tallies(whole, total, "stream of tally sets")
    sharded = simulate(scene, n, seed=seed, record_every=0, emission="device", emit_seed=emit_seed, devices=[0, 0])
    same_tallies(whole, tallies_of(sharded.data), "two shards")
    # a ray alone (a launch of one photon finishes in the tail function) and the rest around it: the first ray, one that is
    # re-emitted three times or more, the last
    again = int(deep.index[np.argmax(deep.emissions)])
    with Session(scene, emission="device") as s:
        for i in (0, again, n - 1):
            pieces = [s.collect(s.submit(b - a, seed, record_every=0, emit_seed=emit_seed, ray_offset=a))
                      for a, b in ((0, i), (i, i + 1), (i + 1, n)) if b > a]
            total = {k: sum(np.asarray(p.data[k]) for p in pieces) for k in TALLY_KEYS}
            same_tallies(whole, total, ("a ray alone", i))
    # the scene that reads origins alone (it counts nothing: the shorter record), carried
    scene = spread_lamp(origin_only()[0])
    whole = tallies_of(simulate(scene, n, seed=seed, record_every=0, emission="device", emit_seed=emit_seed).data)
    for depth in (1, 2):
        _, data, _ = trace_stream(scene, n, n // 3 + 1, seed, emit_seed=emit_seed, depth=depth)
        same_tallies(whole, tallies_of(data), ("origins alone, carried", depth))


# -- no side effect --------------------------------------------------------------------------------------------------------------
def test_origins_change_neither_histories_nor_other_tallies_nor_maps_nor_captures():
    def build(origins, counters, capture, volume_map):
        scene = edge_slab(counters=counters, capture=capture)
        if volume_map:
            node(scene, "LSC").volume_maps = [VolumeMap("dose", (8, 8, 4), (-2.5, -2.5, -0.5), (2.5, 2.5, 0.5))]
        return add_origins(scene) if origins else scene

    pos, dirs, wl = spread_rays(edge_slab(counters=False), None, 100_000, width=4.0)
    others = ((False, None, False), (True, None, True), (False, BIG, True), (True, BIG, False))
    for counters, capture, volume_map in others:
        out = {}
        for origins in (False, True):
            with Session(build(origins, counters, capture, volume_map), emission="host") as s:
                h = submit(s, (pos[:10_000], dirs[:10_000], wl[:10_000]), 7, record_every=1, max_events=64)
                t = submit(s, (pos, dirs, wl), 7, record_every=0)
                out[origins] = (h, t, s.dscene.launch_info()["variant"])
        (h0, t0, v0), (h1, t1, v1) = out[False], out[True]
        what = (counters, capture, volume_map)
        assert v1 == "rough" and (v0 == "rough" if counters or capture or volume_map else v0 in ("lean", "w4")), what
        for k in HIST_KEYS + (("map_bins",) if volume_map else ()):
            assert np.array_equal(np.asarray(h0.data[k]), np.asarray(h1.data[k])), (what, k)
        if volume_map:
            assert np.array_equal(np.asarray(t0.data["map_bins"]), np.asarray(t1.data["map_bins"])), what
        for a, b in ((h0, h1), (t0, t1)):
            for name, rec in a.recorders.items():          # every recorder's own counts and its own histograms
                other = b.recorders[name]
                assert (rec.rays, rec.crossings) == (other.rays, other.crossings), (what, name)
                for i, bins in enumerate(rec._bins):
                    assert np.array_equal(bins, other._bins[i]), (what, name, i)
            # (the moment sums are floating-point atomics: the same addends in whatever order the waves arrive)
            assert np.allclose(a.data["rec_sums"], b.data["rec_sums"], rtol=1e-12, atol=0), what
            same_captures(a.captures, b.captures)
    # a scene that reads origins alone does not count: it takes any maxsteps
    scene, _ = origin_only()
    compiled = compile_scene(scene)
    assert compiled.origin_mask == 0b0101 and not compiled.has_counter_histograms
    with Session(scene, emission="host") as s:
        got = submit(s, (pos[:64], dirs[:64], wl[:64]), 1, record_every=0, maxsteps=1 << 20)
        assert got.recorders["entering"].rays > 0 and s.dscene.launch_info()["variant"] == "rough"


# -- the Beer-Lambert law, per launch wavelength -----------------------------------------------------------------------------
def test_transmission_per_launch_wavelength_is_beer_lamberts():
    scene, n = beer_lambert_slab(), 200_000
    with Session(scene, emission="host") as s:
        result = submit(s, beer_lambert_rays(n), 37, record_every=0)
    assert result.recorders["exit"].rays + result.recorders["lost"].rays == n
    beer_lambert_law(result.recorders["exit"]._bins[0], result.recorders["lost"]._bins[0], n, "kernel")


# -- refusals ----------------------------------------------------------------------------------------------------------------------
def test_older_entries_and_the_host_buffer_entry_refuse_the_origin_ids():
    from pvtrace_amd.engine import _kernel

    scene = edge_slab(counters=False)
    node(scene, "LSC").recorders[0].histograms = [Histogram("wavelength", 400, 800, 40)]
    compiled = compile_scene(scene)
    assert compiled.origin_mask == 0 and compiled.hist_prop_a[0] == 0
    lib = native.load_library()
    st, keep = native.scene_tables_struct(compiled)
    older = {"pvt_scene_create": (), "pvt_scene_create_ex": (None,), "pvt_scene_create_phase": (None,) * 2,
             "pvt_scene_create_rough": (None,) * 3, "pvt_scene_create_field": (None,) * 4, "pvt_scene_create_maps": (None,) * 5,
             "pvt_scene_create_capture": (None,) * 6, "pvt_scene_create_absorb": (None,) * 7}

    def put(a, b):
        props = (np.array(compiled.hist_prop_a, copy=True), np.array(compiled.hist_prop_b, copy=True))
        props[0][0], props[1][0] = a, b
        st.hist_prop_a, st.hist_prop_b = native.np_ptr(props[0]), native.np_ptr(props[1])
        return props

    for prop in (10, 11, 12, 13):
        for a, b in ((prop, -1), (0, prop)):
            held = put(a, b)
            for entry, nulls in older.items():
                handle = C.c_void_p()
                assert getattr(lib, entry)(C.byref(st), *nulls, 0, C.byref(handle)) == -1, (entry, a, b)
                assert lib.pvt_last_error().decode() == "histogram property out of range" and not handle.value, (entry, a, b)
            handle = C.c_void_p()
            assert lib.pvt_scene_create_origin(C.byref(st), *(None,) * 7, 0, C.byref(handle)) == 0, (a, b)   # the newest takes them
            lib.pvt_scene_destroy(handle)
            del held
    for a, b in ((14, -1), (-1, -1), (-2, -1), (0, 14), (0, -2), (1 << 20, -1)):                             # ... and nothing beyond them
        held = put(a, b)
        handle = C.c_void_p()
        assert lib.pvt_scene_create_origin(C.byref(st), *(None,) * 7, 0, C.byref(handle)) == -1, (a, b)
        assert lib.pvt_last_error().decode() == "histogram property out of range" and not handle.value
        del held
    del keep
    scene, _ = origin_only()
    rays = emit_bundle(scene, 64, seed=1)[:3]
    with pytest.raises(UnsupportedSceneError, match="launch-origin property"):
        _kernel.trace_bundle(compile_scene(scene), *rays, 1, 1000, 16, 0, 1, 0)


# -- the example -------------------------------------------------------------------------------------------------------------------
def test_eqe_map_example_prints_the_ratios_of_its_own_histograms(capsys):
    spec = importlib.util.spec_from_file_location("eqe_map", os.path.join(ROOT, "examples", "eqe_map.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    photons = 100_000
    out = module.main(photons=photons)
    printed = capsys.readouterr().out
    recs = out["result"].recorders
    collected = sum(np.asarray(recs[f"edge-{label}"]._bins[0]) for label in module.EDGES)
    launched = sum(np.asarray(recs[name]._bins[0]) for name in module.TERMINAL)
    assert int(launched.sum()) == photons                           # every launched photon ends in a terminal recorder
    assert np.all(collected <= launched) and 0 < int(collected.sum()) < photons
    eqe = collected[launched > 0] / launched[launched > 0]
    assert np.array_equal(out["eqe"][launched > 0], eqe) and 0.0 < eqe.max() < 1.0
    for k in np.flatnonzero(launched > 0)[:4]:
        assert f"{out['wavelengths'][k]:6.1f} nm  EQE {collected[k] / launched[k]:.4f}" in printed
    eta_c = sum(np.asarray(recs[f"edge-{label}"]._bins[1]) for label in module.EDGES).reshape(module.MAP, module.MAP)
    eta_l = sum(np.asarray(recs[name]._bins[1]) for name in module.TERMINAL).reshape(module.MAP, module.MAP)
    assert int(eta_l.sum()) == photons and np.all(eta_l > 0)
    assert np.array_equal(out["eta"], eta_c / eta_l)
    assert " ".join(f"{v:.3f}" for v in (eta_c / eta_l)[0]) in printed
    assert math.isclose(out["total"], collected.sum() / photons) and f"{out['total']:.4f}" in printed
