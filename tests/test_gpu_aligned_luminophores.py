"""Aligned luminophores (`Alignment`) on the GPU.  The kernel is never its own reference: orders of zero are held bit for
bit to the scene without alignment, absorption to Beer-Lambert with the closed-form factor, the component pick to the
scaled coefficients, emission to the lowered table's own masses and to the host tracer, and every way of launching to the
same histories and tallies.  Scenes: tests/aligned_scenes.py; bars: tests/laws.py."""
import ctypes as C
import importlib.util
import math
import os
import re

import numpy as np
import pytest

from pvtrace_amd import (
    Absorber, Alignment, ConcentrationGrid, Event, PhaseFunctionTable, Ray, Scatterer, VolumeMap, photon_tracer,
)
from pvtrace_amd.engine import (
    Histogram, Recorder, Session, _kernel, capture_histories, compile_scene, map_histories, native, simulate, tally_histories,
)
from pvtrace_amd.engine.compiler import UnsupportedSceneError
from pvtrace_amd.engine.emit import emit_bundle
from tests import aligned_scenes as A
from tests import laws as L
from tests import scenes
from tests.capture_scenes import submit

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TALLY_KEYS = ("rec_distinct", "rec_crossings", "rec_bins")
HIST_KEYS = ("counts", "kind", "hit", "container", "adjacent", "component", "source", "position", "direction", "normal",
             "wavelength", "travelled", "duration")
SIZES = (1, 65, 10_000)     # the lone lane; one wave plus one lane; many workgroups with refill
ABSORB, EMIT, EXIT = Event.ABSORB.value, Event.EMIT.value, Event.EXIT.value
LAW_RAYS = 200_000


def variant(session):
    return session.dscene.launch_info()["variant"]


def history(scene, rays, seed=7, max_events=16, **kw):
    """The history launch of host rays -> (columns, variant); no history may be cut by `max_events`."""
    with Session(scene, emission="host") as s:
        h = submit(s, rays, seed, record_every=1, max_events=max_events, **kw)
        assert int(np.asarray(h.data["counts"]).max()) < max_events
        return {k: np.asarray(h.data[k]).copy() for k in HIST_KEYS}, variant(s)


def rows_of(columns, kind, max_events, first=True):
    """Flat indices of the (first) row of `kind` of every history that has one."""
    counts = columns["counts"]
    kinds = columns["kind"].reshape(len(counts), max_events)
    live = np.arange(max_events)[None, :] < counts[:, None]
    at = (kinds == kind) & live
    rays = np.flatnonzero(at.any(axis=1))
    return rays * max_events + np.argmax(at[rays], axis=1), rays


def absorbed_count(columns, max_events):
    return len(rows_of(columns, ABSORB, max_events)[1])


# -- 1. orders of zero are no alignment --------------------------------------------------------------------------------
def _tiles():
    from benchmarks.configs import tiles_lsc
    return tiles_lsc(3, recorders="all")       # 9 tiles in a world: 10 nodes


ZERO_SCENES = {"slab": (scenes.lsc_equivalent, "host"), "tiles": (_tiles, "host"), "mesh": (scenes.mesh_lsc, "host"),
               "device-emission": (scenes.lsc_equivalent, "device")}


def _both_launches(scene, emission, rays, n, seed=7, max_events=256):
    with Session(scene, emission=emission) as s:
        if emission == "device":
            h = s.collect(s.submit(n, seed, record_every=1, max_events=max_events, emit_seed=31))
            t = s.collect(s.submit(n, seed, record_every=0, emit_seed=31))
        else:
            h = submit(s, rays, seed, record_every=1, max_events=max_events)
            t = submit(s, rays, seed, record_every=0)
        assert int(np.asarray(h.data["counts"]).max()) < max_events
        return ({k: np.asarray(h.data[k]).copy() for k in HIST_KEYS + TALLY_KEYS},
                {k: np.asarray(t.data[k]).copy() for k in TALLY_KEYS + ("rec_sums",)}, variant(s))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", sorted(ZERO_SCENES))
def test_orders_of_zero_trace_bit_for_bit_as_no_alignment(name, n):
    build, emission = ZERO_SCENES[name]
    pos, dirs, wl, _ = emit_bundle(build(), n, seed=3)
    plain = _both_launches(build(), emission, (pos, dirs, wl), n)
    zero = _both_launches(A.zero_aligned(build()), emission, (pos, dirs, wl), n)
    assert compile_scene(A.zero_aligned(build())).has_alignment
    assert zero[2] == "rough" and plain[2] != "rough", (zero[2], plain[2])
    for k in HIST_KEYS + TALLY_KEYS:
        assert np.array_equal(zero[0][k], plain[0][k], equal_nan=zero[0][k].dtype.kind == "f"), (name, n, k)
    for k in TALLY_KEYS:
        assert np.array_equal(zero[1][k], plain[1][k]), (name, n, k)
    assert np.allclose(zero[1]["rec_sums"], plain[1]["rec_sums"], rtol=1e-12, atol=0), (name, n)
    if n > 1000:
        assert np.any(plain[0]["kind"] == ABSORB) and np.any(plain[0]["kind"] == EMIT)


# -- 2. the exact zero -------------------------------------------------------------------------------------------------
def test_a_pure_dipole_along_the_pencil_absorbs_nothing():
    n, me = 10_000, 16
    scene = A.slab_scene([A.absorber(5.0, (0.0, 0.0, 1.0), 1.0)])
    rays, _ = A.pencil(0.0, n)
    columns, v = history(scene, rays, max_events=me)
    assert v == "rough"
    counts = columns["counts"]
    kinds = columns["kind"].reshape(n, me)
    live = np.arange(me)[None, :] < counts[:, None]
    assert not np.any((kinds == ABSORB) & live)                        # there is NO ABSORB row ...
    assert np.all(kinds[np.arange(n), counts - 1] == EXIT)             # ... and every ray exits
    # (the same slab without alignment absorbs 1 - exp(-5) of them: the zero is the alignment's)
    bare, _ = history(A.slab_scene([Absorber(5.0)]), rays, max_events=me)
    L.assert_binomial(absorbed_count(bare, me), n, -math.expm1(-5.0), "isotropic")


# -- 3. Beer-Lambert by angle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rotate", [None, A.TILT], ids=["unrotated", "tilted"])
@pytest.mark.parametrize("order", [1.0, -0.5])
@pytest.mark.parametrize("theta", A.ANGLES)
def test_absorbed_share_of_a_pencil_is_beer_lambert_with_the_factor(theta, order, rotate):
    n, me, alpha = LAW_RAYS, 16, 1.0
    scene = A.slab_scene([A.absorber(alpha, (0.0, 0.0, 1.0), order)], rotate=rotate)   # (the director in the node's frame)
    rays, chord = A.pencil(theta, n, rotate=rotate)
    director_world = A.rotation_of(rotate) @ np.array([0.0, 0.0, 1.0])
    f = A.factor_along(rays[1][0], director_world, order)
    p = A.absorbed_probability(alpha, f, chord)
    columns, v = history(scene, rays, max_events=me)
    k = absorbed_count(columns, me)
    print("theta", theta, "S", order, "rotated", rotate is not None, "f", f, "chord", chord, "absorbed", k, "expected", p * n)
    assert v == "rough"
    L.assert_binomial(k, n, p, (theta, order, rotate is not None))


# -- 4. the pick -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", [(1.0, 0.0, 1.0), (1.0, 0.0, 2.0), (0.0, 0.0, 1.0)], ids=["101", "102", "001"])
@pytest.mark.parametrize("third", [False, True], ids=["two", "three"])
def test_absorbing_component_is_picked_by_the_scaled_coefficients(direction, third):
    n, me = LAW_RAYS, 16
    comps = [A.absorber(1.0, (0.0, 0.0, 1.0), 1.0, name="z"), A.absorber(1.0, (1.0, 0.0, 0.0), 1.0, name="x")]
    if third:    # (beyond the two-component shortcut: the walk)
        comps.append(A.absorber(1.0, (0.0, 1.0, 0.0), 1.0, name="y"))
    scene = A.slab_scene(comps)
    d = np.asarray(direction) / math.sqrt(sum(v * v for v in direction))
    start = np.array([-0.2, 0.1, 0.0]) - 4.0 * d
    rays = (np.tile(start, (n, 1)), np.tile(d, (n, 1)), np.full(n, 555.0))
    columns, v = history(scene, rays, max_events=me)
    rows, _ = rows_of(columns, ABSORB, me)
    weights = [1.0 * A.factor_along(d, c.alignment.director, 1.0) for c in comps]
    picked = columns["component"][rows]
    base = compile_scene(scene).comp_start[compile_scene(scene).node_names.index("slab")]
    print(direction, "weights", weights, "absorbed", len(rows), "by component", np.bincount(picked - base, minlength=len(comps)))
    assert v == "rough" and len(rows) > 20_000
    for i, w in enumerate(weights):
        L.assert_binomial(int(np.sum(picked == base + i)), len(rows), w / sum(weights), (direction, third, i))
    # and the depth is Beer-Lambert over the scaled sum
    chord = A.SLAB[2] / d[2]
    L.assert_binomial(len(rows), n, A.absorbed_probability(1.0, sum(weights), chord), (direction, third, "depth"))


# -- 5. emission -------------------------------------------------------------------------------------------------------
DIRECTOR = (1.0 / 3.0, 2.0 / 3.0, 2.0 / 3.0)      # not along z, not along the pencil


def _first_emissions(scene, n, seed, me=32):
    rays, _ = A.pencil(0.0, n)
    columns, v = history(scene, rays, seed=seed, max_events=me, maxsteps=12)
    assert v == "rough"
    rows, _ = rows_of(columns, EMIT, me)
    return columns["direction"].reshape(-1, 3)[rows], columns["wavelength"][rows], columns


@pytest.mark.parametrize("s_e", [1.0, -0.5, 0.6])
def test_emission_follows_the_table_about_the_director(s_e):
    n = LAW_RAYS
    dye = A.luminophore(5.0, DIRECTOR, 0.0, s_e)
    scene = A.slab_scene([dye], rotate=A.TILT, index=1.0)
    n_w = compile_scene(scene).align_axis[0]
    assert np.allclose(n_w, L.rotation(*A.TILT) @ np.asarray(DIRECTOR))
    dirs, wl, _ = _first_emissions(scene, n, seed=7)
    assert len(dirs) > 0.9 * n
    mu, phi = A.mu_and_azimuth(dirs, n_w)
    masses = A.table_bin_masses(dye.alignment.emission_table, 32)
    counts = np.histogram(mu, bins=32, range=(-1.0, 1.0))[0]
    print("S_e", s_e, "emissions", len(dirs), "mean mu^2", float(np.mean(mu * mu)), "closed form", (1.0 - 0.4 * s_e) / 3.0)
    L.assert_chi2(counts, masses, ("mu", s_e))
    L.assert_chi2(np.histogram(phi, bins=16, range=(-math.pi, math.pi))[0], np.full(16, 1.0 / 16.0), ("azimuth", s_e))
    # the emitted wavelengths are those of the same scene with S_e = 0 (another seed: two samples)
    iso = A.slab_scene([A.luminophore(5.0, DIRECTOR, 0.0, 0.0)], rotate=A.TILT, index=1.0)
    _, wl_iso, _ = _first_emissions(iso, n, seed=8)
    L.assert_ks2(wl, wl_iso, ("wavelength", s_e))
    # and an aligned emission consumes the draws an isotropic one does: under ONE seed the two scenes absorb at the same
    # points and emit the same wavelengths, ray for ray
    _, wl_same, _ = _first_emissions(iso, n, seed=7)
    assert np.array_equal(wl, wl_same)


# -- 6. host and GPU ---------------------------------------------------------------------------------------------------
def test_host_tracer_and_gpu_agree_on_depth_and_emission():
    n_host, n_gpu, me = 20_000, LAW_RAYS, 32
    scene = A.slab_scene([A.luminophore(1.5, DIRECTOR, 0.6, 0.6)], rotate=A.TILT)
    n_w = compile_scene(scene).align_axis[0]
    rays, _ = A.pencil(30.0, n_gpu, rotate=A.TILT)
    columns, v = history(scene, rays, max_events=me, maxsteps=12)
    assert v == "rough"
    start, d = rays[0][0], rays[1][0]
    a_rows, _ = rows_of(columns, ABSORB, me)
    e_rows, _ = rows_of(columns, EMIT, me)
    gpu_depth = (columns["position"].reshape(-1, 3)[a_rows] - start) @ d
    gpu_mu = columns["direction"].reshape(-1, 3)[e_rows] @ n_w
    np.random.seed(17)
    ray = Ray(position=tuple(start), direction=tuple(d), wavelength=555.0)
    host_depth, host_mu = [], []
    for _ in range(n_host):
        seen = set()
        for r, event, _ in photon_tracer.step_forward(scene, ray, maxsteps=12, backend="host"):
            if event == Event.ABSORB and Event.ABSORB not in seen:
                host_depth.append(float((np.asarray(r.position) - start) @ d))
            if event == Event.EMIT:      # (the first emission: the rest of the history is not looked at)
                host_mu.append(float(np.asarray(r.direction) @ n_w))
                break
            seen.add(event)
    print("host absorbed", len(host_depth), "of", n_host, "gpu", len(gpu_depth), "of", n_gpu)
    L.assert_binomial(len(host_depth), n_host, len(gpu_depth) / n_gpu, "absorbed share (GPU share as p)")
    L.assert_ks2(host_depth, gpu_depth, "first absorption depth")
    L.assert_ks2(host_mu, gpu_mu, "first emission mu")


# -- 7. the launch does not matter -------------------------------------------------------------------------------------
def _lsc_aligned():
    """An index-1.5 slab with an aligned dye and an aligned background, recorders, a volume map and a capture."""
    scene = A.slab_scene([A.luminophore(3.0, DIRECTOR, 0.6, 0.6, name="dye"), A.absorber(0.3, (1.0, 0.0, 0.0), -0.5, name="host")],
                         rotate=A.TILT, index=1.5)
    slab = next(n for n in scene.root.preorder() if n.name == "slab")
    slab.recorders = [Recorder("out-kept", event="escaping", histograms=[Histogram("wavelength", 400, 800, 40)], capture=8192),
                      Recorder("out", event="escaping"), Recorder("lost", event="lost"), Recorder("in", event="entering")]
    slab.volume_maps = [VolumeMap("absorbed", event="absorbed", shape=(4, 4, 2), lower=(-2.0, -2.0, -0.5), upper=(2.0, 2.0, 0.5)),
                        VolumeMap("emitted", event="emitted", shape=(2, 2, 1), lower=(-2.0, -2.0, -0.5), upper=(2.0, 2.0, 0.5))]
    scene.root.recorders = [Recorder("exit", event="exit")]
    return scene


def test_histories_tallies_and_referees_do_not_depend_on_the_launch():
    import torch

    scene = _lsc_aligned()
    n, me, seed = 10_000, 96, 23
    rng = np.random.default_rng(4)
    base, _ = A.pencil(20.0, n, rotate=A.TILT)
    pos = base[0] + (L.rotation(*A.TILT) @ np.vstack([rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n), np.zeros(n)])).T
    rays = (pos, base[1], np.full(n, 555.0))
    with Session(scene, emission="host") as s:
        hist = submit(s, rays, seed, record_every=1, max_events=me, maxsteps=40)
        assert variant(s) == "rough" and int(np.asarray(hist.data["counts"]).max()) < me
        data = {k: np.asarray(hist.data[k]) for k in HIST_KEYS}
        assert np.sum(data["kind"] == EMIT) > 2000
        for i in range(0, n, 1250):     # the same ray alone, in a launch of one: traced by the tail function
            one = submit(s, tuple(t[i:i + 1] for t in rays), seed, record_every=1, max_events=me, maxsteps=40, ray_offset=i)
            k = int(data["counts"][i])
            assert int(one.data["counts"][0]) == k, i
            for key in HIST_KEYS[1:]:
                assert np.array_equal(np.asarray(one.data[key])[:k], data[key][i * me:i * me + k], equal_nan=True), (i, key)
        tally = submit(s, rays, seed, record_every=0, maxsteps=40)
        for key in TALLY_KEYS:
            assert np.array_equal(np.asarray(hist.data[key]), np.asarray(tally.data[key])), key
        # the host referees on the launch's own log: recorders, volume maps, captures
        histories = list(hist.histories())
        referee = tally_histories(scene, histories)
        for name, rec in tally.recorders.items():
            assert (rec.rays, rec.crossings) == (referee[name].rays, referee[name].crossings), name
            assert (hist.recorders[name].rays, hist.recorders[name].crossings) == (rec.rays, rec.crossings), name
        maps = map_histories(scene, histories)
        assert sorted(maps) == sorted(tally.volume_maps) == ["absorbed", "emitted"]
        for name, want in maps.items():
            for got in (tally.volume_maps[name], hist.volume_maps[name]):
                assert np.array_equal(got.counts, want.counts) and got.outside == want.outside, name
            assert int(np.sum(want.counts)) > 1000, name
        captured = capture_histories(scene, histories)["out-kept"]
        for got in (tally.captures["out-kept"], hist.captures["out-kept"]):
            assert len(got) == len(captured) > 100 and got.matched == captured.matched
            for column in ("index", "position", "direction", "wavelength"):
                assert np.array_equal(getattr(got, column), getattr(captured, column)), column
    # two carried launches equal one
    compiled = compile_scene(scene)
    dscene = native.DeviceScene(compiled, device=0)
    try:
        dev = torch.device("cuda", 0)
        drays = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in rays)
        whole, parts = dscene.new_tallies(), dscene.new_tallies()
        dscene.trace(drays, n, seed, whole, maxsteps=40)
        cut = 4_033
        dscene.trace(tuple(t[:cut] for t in drays), cut, seed, parts, ray_offset=0, carry_out=True, maxsteps=40)
        dscene.trace(tuple(t[cut:] for t in drays), n - cut, seed, parts, ray_offset=cut, carry_out=False, maxsteps=40)
        torch.cuda.synchronize()
        assert np.array_equal(whole.ints.cpu().numpy(), parts.ints.cpu().numpy()) and int(whole.ints.sum()) > 0
    finally:
        dscene.close()


# -- 8. refusals -------------------------------------------------------------------------------------------------------
def _create(compiled, mutate=None, entry="pvt_scene_create_aligned"):
    """Call a creation entry with the scene's own structs, `mutate(keep of PvtAlignTables, struct)` having broken the
    alignment tables by hand -> (return code, message)."""
    lib = native.load_library()
    st, keep = native.scene_tables_struct(compiled)
    count = native.CREATION_ENTRIES[entry]
    made = [native.marshal(t, compiled) for t in native.EXTENSION_TABLES[:count]]
    if mutate is not None:
        mutate(made[-1][1], made[-1][0], made)
    handle = C.c_void_p()
    rc = getattr(lib, entry)(C.byref(st), *[None if m is None else C.byref(m) for m, _ in made], 0, C.byref(handle))
    message = (lib.pvt_last_error() or b"").decode()
    if rc == 0:
        lib.pvt_scene_destroy(handle)
    del keep
    return rc, message


def test_packer_refuses_hand_broken_tables_each_with_its_own_message():
    def fresh():     # (the structs point INTO the lowered tables: every case breaks a lowering of its own)
        return compile_scene(A.slab_scene([A.luminophore(1.0, DIRECTOR, 0.6, 0.6), A.absorber(1.0, (0, 0, 1), 0.5, name="host")]))

    assert _create(fresh())[0] == 0

    def put(field, index, value):
        def mutate(keep, struct, made):
            keep[field].reshape(-1)[index] = value
        return mutate

    def field_under_the_slab(keep, struct, made):
        """A lattice on the slab, handed to the entry beside the alignment."""
        grid = ConcentrationGrid(np.ones((1, 1, 1)), (-2.0, -2.0, -0.5), (2.0, 2.0, 0.5))
        fielded = compile_scene(A.slab_scene([Absorber(1.0, x=None, concentration=grid), Absorber(1.0, concentration=grid)]))
        made[3] = native.marshal(native.PvtFieldTables, fielded)

    def no_component_named(keep, struct, made):
        keep["comp_align"][:] = -1
        struct.n_components = 0     # (then the scene is the unaligned one: accepted)

    cases = [
        (put("axis", 0, 0.5), "unit vector within 1e-12"),
        (put("axis", 4, 1.0 + 1e-9), "unit vector within 1e-12"),
        (put("abs_order", 0, 1.5), r"must lie in \[-0.5, 1\]"),
        (put("abs_order", 1, -0.6), r"must lie in \[-0.5, 1\]"),
        (put("abs_order", 0, math.nan), "must be finite"),
        (put("abs_order", 0, math.inf), "must be finite"),
        (put("emit_table", 0, 7), "outside the phase tables"),
        (put("emit_table", 1, 0), "must be the phase table it names"),
        (put("comp_align", 0, 5), "names a missing record"),
        (field_under_the_slab, "concentration field is out of scope"),
    ]
    for mutate, text in cases:
        rc, message = _create(fresh(), mutate)
        assert rc == -1 and re.search(text, message), (text, rc, message)
    assert _create(fresh(), no_component_named)[0] == 0
    # a multi-row table is no emission table
    rows = PhaseFunctionTable([0.0, 180.0], [[1.0, 1.0], [1.0, 2.0]], wavelength=[500.0, 600.0])
    two = compile_scene(A.slab_scene([A.luminophore(1.0, DIRECTOR, 0.6, 0.6),
                                      Scatterer(1.0, phase_function=rows, name="fog")]))
    rc, message = _create(two, lambda keep, struct, made: (keep["emit_table"].__setitem__(0, 1)))
    assert rc == -1 and "single row" in message, message
    # the root: an aligned component there is refused by the packer too
    world = A.slab_scene([A.absorber(1.0, (0, 0, 1), 0.5)])
    c = compile_scene(world)
    c.comp_start = c.comp_start[::-1].copy()      # hand the slab's component run to the root
    c.comp_count = c.comp_count[::-1].copy()
    rc, message = _create(c)
    assert rc == -1 and "root" in message, message
    assert native.load_library().pvt_abi_version() == 13


def test_older_entries_host_buffer_entry_and_fields_refuse(monkeypatch):
    scene = A.slab_scene([A.luminophore(2.0, DIRECTOR, 0.6, 0.6)])
    compiled = compile_scene(scene)
    rays, _ = A.pencil(0.0, 16)
    with pytest.raises(UnsupportedSceneError, match="aligned components"):
        _kernel.trace_bundle(compiled, *rays, 1, 100, 16, 0, 1, 0)
    # no older entry takes the struct: Python reaches none of them, and the newest is the pattern entry without it
    lib = native.load_library()
    reached = []
    for entry in native.CREATION_ENTRIES:
        if entry != "pvt_scene_create_aligned":
            real = getattr(lib, entry)
            monkeypatch.setattr(lib, entry, lambda *a, _real=real, _entry=entry: reached.append(_entry) or _real(*a))
    r = simulate(scene, 4096, seed=2, record_every=0)
    assert not reached and r is not None
    assert native.CREATION_ENTRIES["pvt_scene_create_pattern"] == 8 < native.CREATION_ENTRIES["pvt_scene_create_aligned"]
    # ... and none of them CAN be handed the struct: that is their refusal, and the header says so
    lib_sigs = native.declare_signatures(lib, native.ABI_SYMBOLS)
    for entry in native.CREATION_ENTRIES:
        takes = C.POINTER(native.PvtAlignTables) in lib_sigs[entry][0]
        assert takes == (entry == "pvt_scene_create_aligned"), entry
    header = " ".join(open(os.path.join(ROOT, "include", "pvtrace_hip.h")).read().replace(" * ", " ").split())
    assert "entries cannot be handed this struct, and that is their refusal" in header
    bare = compile_scene(A.slab_scene([A.luminophore(2.0, None, 0.0, 0.0)]))
    assert _create(bare, entry="pvt_scene_create_pattern")[0] == 0 and _create(bare)[0] == 0
    grid = ConcentrationGrid(np.ones((2, 1, 1)), (-2.0, -2.0, -0.5), (2.0, 2.0, 0.5))
    with pytest.raises(UnsupportedSceneError, match="out of scope"):
        simulate(A.slab_scene([A.absorber(1.0, (0, 0, 1), 0.5), Absorber(1.0, name="graded", concentration=grid)]), 64, seed=1)


# -- 9. the example ----------------------------------------------------------------------------------------------------
def test_aligned_dye_example_escape_cone_shares_follow_the_closed_form():
    spec = importlib.util.spec_from_file_location("aligned_dye", os.path.join(ROOT, "examples", "aligned_dye.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    out = module.main(photons=100_000)
    print(out)
    mu_c = math.sqrt(1.0 - 1.0 / 2.25)     # the integral of f over mu_c .. 1: (1 + S / 2)(1 - mu_c) - S / 2 (1 - mu_c^3)
    for name, order in (("isotropic", 0.0), ("homeotropic", 1.0), ("planar", -0.5)):
        want = (1.0 + 0.5 * order) * (1.0 - mu_c) - 0.5 * order * (1.0 - mu_c ** 3)
        assert abs(out[name]["closed_form"] - want) < 1e-12, name
    assert round(out["homeotropic"]["closed_form"], 4) == 0.0890 and round(out["isotropic"]["closed_form"], 4) == 0.2546
    for name in ("isotropic", "homeotropic", "planar"):
        case = out[name]
        assert case["emitted"] > 20_000
        L.assert_binomial(case["in_cone"], case["emitted"], case["closed_form"], name)
    assert out["homeotropic"]["share"] < out["isotropic"]["share"] < out["planar"]["share"]
