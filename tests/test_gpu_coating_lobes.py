"""Scattering coatings (`Coating(reflection=ScatterLobe(...))`, `transmission=`) on the GPU.

Every REFLECT / TRANSMIT row at a lobe-coated point of a history launch is held to `lobe_cases.kernel_turn`, the float64
restatement of the contract, within the derived bound (`lobe_cases.pair_bound`): the inputs are the launch's own log (the
preceding row's direction, the logged normal and wavelength), the draws those of the stream SEED + i at the position the
walk over the ray's rows arrives at, so a row that consumed another number of draws moves every later row of its ray.
The rest holds the kernel to itself across the ways of launching, to the built-in specular coating where no photon
reaches the lobe, to closed-form laws and to the host delegate (tests/lobe_cases.py: cases, references, bound).

Measured on an MI355X: 29 738 rows judged over the eleven cases (1 500 ... 4 188 per case; refracted-60: 953 lobe turns
and 3 235 total reflections by the specular body), worst |direction - restatement| / bound 0.034 (cosine-reflection);
no row met an ambiguity condition (docs/parity_chain.md, "Scattering coatings")."""
import ctypes
import importlib.util
import math
import os

import numpy as np
import pytest

from pvtrace_amd import Coating, Event, ScatterLobe
from pvtrace_amd.engine import (
    Histogram, Recorder, Session, _kernel, compile_scene, native, simulate, simulate_stream, tally_histories,
)
from pvtrace_amd.engine.compiler import COAT_LOBE, UnsupportedSceneError
from pvtrace_amd.engine.emit import emit_bundle
from pvtrace_amd.material import ray_basis
from tests import laws as L
from tests import lobe_cases as LC
from tests import pattern_scenes as P
from tests.capture_scenes import history_launch, submit

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [c.name for c in LC.CASES]
TALLY_KEYS = ("rec_distinct", "rec_crossings", "rec_bins")
HIST_KEYS = ("counts", "kind", "hit", "container", "adjacent", "component", "source", "position", "direction", "normal",
             "wavelength", "travelled", "duration")


def history(scene, pos, dirs, wl, seed=LC.SEED, me=LC.ME, launch=None, ray_offset=0):
    n = len(wl)
    with Session(scene, emission="host") as s:
        r = s.collect(s.submit(n, seed, host_rays=(pos, dirs, wl, ["r"] * n), record_every=1, max_events=me,
                               maxsteps=LC.MAXSTEPS, ray_offset=ray_offset))
        data = {k: np.asarray(r.data[k]).copy() for k in HIST_KEYS}
        if launch is not None:
            launch.update(s.dscene.launch_info())
    out = {"counts": data["counts"]}
    for k in ("kind", "hit", "container", "adjacent", "wavelength"):
        out[k] = data[k].reshape(n, me)
    for k in ("position", "direction", "normal"):
        out[k] = data[k].reshape(n, me, 3)
    return out


# ---- 1. every row at a lobe-coated point, by the restatement -----------------------------------------------------------------------
@pytest.mark.parametrize("name", IDS)
def test_every_row_at_a_lobe_coated_point_equals_the_restatement(name):
    x = LC.inputs(name)
    case = x.case
    scene, _ = case.scene()
    compiled = compile_scene(scene)
    node = compiled.node_names.index("lobe")
    launch = {}
    h = history(scene, x.pos, x.dirs, x.wl, launch=launch)
    assert compiled.has_coating_lobes and launch["variant"] == "rough", launch
    if name == "cosine-4097":       # the table alone exceeds what a workgroup may stage: it is read from global memory
        assert 8 * (2 * 4097 + 3) > 64 * 1024 > launch["lds_bytes"]
    judged = lobe_rows = built_in = 0
    worst = 0.0
    kinds = {LC.REFLECT: 0, LC.TRANSMIT: 0}
    for i in range(case.n):
        at = 0                                        # the ray's position in its stream
        assert h["kind"][i, 0] == LC.GENERATE and h["counts"][i] >= 2
        for row in range(1, int(h["counts"][i])):
            kind = int(h["kind"][i, row])
            if kind in (LC.EXIT, Event.KILL.value):     # (leaving the world; a history that filled its ME rows)
                continue
            assert kind in (LC.REFLECT, LC.TRANSMIT) and h["hit"][i, row] == node, (name, i, row, kind)
            d, normal, wl = h["direction"][i, row - 1], h["normal"][i, row], float(h["wavelength"][i, row])
            inside = int(h["container"][i, row]) == node
            want, used, near = LC.outcome(case, d, normal, inside, x.draws[i][at:])
            if near:
                break                                 # (within 1e-9 of the critical cosine: this ray is judged no further)
            assert kind == want, (name, i, row, "kind", kind, want)
            at += used
            n1, n2 = LC.indices(inside)
            mode = LC.mode_of(case, kind)
            direction, used, info = LC.kernel_turn(mode, kind == LC.TRANSMIT, d, normal, wl, list(x.draws[i][at:]), n1, n2)
            at += used
            bound = LC.pair_bound(mode, d, normal, info, n1, n2)
            err = float(np.max(np.abs(h["direction"][i, row] - direction)))
            if info is not None:
                s = 1.0 if float(np.dot(normal, d)) < 0.0 else -1.0
                n_out = (-s if kind == LC.TRANSMIT else s) * normal
                t = float(np.dot(direction, n_out))
                if abs(t) <= 3.0 * bound + 6.0 * LC.U or (mode.about != "normal" and abs(info[2][2]) <= bound):
                    break                             # (the fold or the basis's sign is ambiguous: judged no further)
                assert float(np.dot(h["direction"][i, row], n_out)) >= -bound, (name, i, row, "below the horizon")
                lobe_rows += 1
            else:
                built_in += 1
            assert err <= bound, (name, i, row, kind, err, bound, h["direction"][i, row].tolist(), direction.tolist())
            worst = max(worst, err / bound)
            kinds[kind] += 1
            judged += 1
            assert row == 1 or at <= LC.DRAWS - 4
    print(f"kernel {name}: {judged} rows judged ({lobe_rows} lobe turns, {built_in} built-in), kinds {kinds}, "
          f"worst error / bound {worst:.3f}, {launch}")
    assert lobe_rows >= case.n // 2 and judged >= case.n
    if name == "refracted-60":
        assert built_in >= 400
    if name == "sphere-both":
        assert min(kinds.values()) >= 300


# ---- 2. a lobe nobody reaches is the specular coating, bit for bit -------------------------------------------------------------------
def launches(scene, rays, seed=7, max_events=64):
    with Session(scene, emission="host") as s:
        h = submit(s, rays, seed, record_every=1, max_events=max_events)
        columns = {k: np.asarray(h.data[k]).copy() for k in HIST_KEYS + TALLY_KEYS}
        t = submit(s, rays, seed, record_every=0)
        tallies = {k: np.asarray(t.data[k]).copy() for k in TALLY_KEYS + ("rec_sums",)}
        return columns, tallies, s.dscene.launch_info()["variant"], h, t


def same_launches(a, b, what):
    for k in HIST_KEYS + TALLY_KEYS:
        assert np.array_equal(a[0][k], b[0][k], equal_nan=a[0][k].dtype.kind == "f"), (what, k)
    for k in TALLY_KEYS:
        assert np.array_equal(a[1][k], b[1][k]), (what, k)
    assert np.allclose(a[1]["rec_sums"], b[1]["rec_sums"], rtol=1e-12, atol=0), what     # (sums of doubles: the order of the atomics)


def rays_of(scene, n, seed=3):
    pos, dirs, wl, _ = emit_bundle(scene, n, seed=seed)
    return pos, dirs, wl


def test_a_lobe_on_a_face_no_photon_reaches_traces_as_the_specular_coating():
    far = ((100.0, 101.0), None, None)               # (a region outside the box: nothing is covered)
    half = lambda pattern: Coating(P.TOP, reflectivity=0.6)
    lobed = lambda pattern: [Coating(None, reflectivity=1.0, region=far, reflection=LC.COSINE,
                                     transmission=ScatterLobe(LC.COSINE.table, "straight")), half(None)]
    plain = lambda pattern: [Coating(None, reflectivity=1.0, region=far), half(None)]
    rays = rays_of(P.p1(coating=plain), 20_000)
    got, want = launches(P.p1(coating=lobed), rays), launches(P.p1(coating=plain), rays)
    assert got[2] == want[2] == "rough"              # (facet=None: both run the extension family)
    same_launches(got, want, "unreached lobe")


# ---- 3. the ways of launching --------------------------------------------------------------------------------------------------------
def lobe_coatings(pattern):
    return [Coating(P.TOP, reflectivity=0.5, reflection=LC.COSINE, transmission=ScatterLobe(LC.COSINE.table, "normal"), pattern=pattern),
            Coating((0.0, 0.0, -1.0), reflectivity=1.0, reflection=ScatterLobe.gaussian(5.0, "specular"))]


def one_lobe_coating(facet):
    return lambda pattern: Coating(facet, reflectivity=0.5, reflection=LC.COSINE, transmission=ScatterLobe(LC.COSINE.table, "normal"))


@pytest.mark.parametrize("layout", ["p1", "p2", "p3", "p4", "sphere"])
def test_tally_launch_equals_history_launch_and_the_referee(layout):
    """An analytic box (p1), a rotated one (p2), a node grid of 37 nodes (p3), a scene with a mesh (p4) and a sphere."""
    build = P.sphere if layout == "sphere" else P.LAYOUTS[layout][0]
    coating = one_lobe_coating(None) if layout == "sphere" else one_lobe_coating(P.TOP) if layout == "p3" else lobe_coatings
    scene = build(coating=coating)
    rays = rays_of(scene, 20_000)
    columns, tallies, v, hist, tally = launches(scene, rays, max_events=384)
    assert v == "rough" and int(columns["counts"].max()) < 384
    for k in TALLY_KEYS:
        assert np.array_equal(columns[k], tallies[k]), (layout, k)
    referee = tally_histories(scene, list(hist.histories()))
    fired = 0
    for name, rec in tally.recorders.items():
        assert (rec.rays, rec.crossings) == (referee[name].rays, referee[name].crossings), (layout, name)
        fired += rec.rays
    assert fired > 1000
    kinds = columns["kind"]
    assert np.sum(kinds == Event.REFLECT.value) > 1000 and np.sum(kinds == Event.TRANSMIT.value) > 1000


def test_a_ray_alone_and_the_rest_are_the_whole():
    x = LC.inputs("sphere-both")
    scene, _ = x.case.scene()
    whole = history(scene, x.pos, x.dirs, x.wl)
    for i in (0, 1, 517):
        alone = history(scene, x.pos[i:i + 1], x.dirs[i:i + 1], x.wl[i:i + 1], ray_offset=i)     # (the tail function)
        count = int(whole["counts"][i])
        assert int(alone["counts"][0]) == count >= 2
        for k in whole:
            if k != "counts":
                assert np.array_equal(alone[k][0, :count], whole[k][i, :count]), (i, k)
    rest = history(scene, x.pos[1:], x.dirs[1:], x.wl[1:], ray_offset=1)
    assert np.array_equal(rest["counts"], whole["counts"][1:])
    written = np.arange(LC.ME)[None, :] < rest["counts"][:, None]
    for k in whole:
        if k != "counts":
            assert np.array_equal(rest[k][written], whole[k][1:][written]), k


def test_carried_launches_and_device_emission_give_the_tallies_of_one_launch():
    scene = P.p1(coating=lobe_coatings)
    n, seed, emit_seed = 90_000, 13, 21
    whole = simulate(scene, n, seed=seed, record_every=0, emission="device", emit_seed=emit_seed)
    assert whole.recorders["escaping"].rays > 10_000
    totals = None
    for result, _ in simulate_stream(scene, n, bundle=n // 3, seed=seed, record_every=0, emission="device", emit_seed=emit_seed):
        block = {k: np.asarray(result.data[k]).astype(np.int64) for k in TALLY_KEYS}
        totals = block if totals is None else {k: totals[k] + block[k] for k in TALLY_KEYS}
    for k in TALLY_KEYS:
        assert np.array_equal(totals[k], np.asarray(whole.data[k])), k


def test_reflections_histograms_count_lobe_reflections_as_the_log_does():
    """The `reflections` counter of a photon counts its lobe reflections: the kernel's histograms, in a history launch and
    in a tally launch, equal the host referee's count of the kernel's own log."""
    scene = P.p1(coating=lobe_coatings)
    box = next(n for n in scene.root.children if n.name == "box")
    box.recorders = [Recorder("escaping", event="escaping", histograms=[Histogram("reflections", 0, 48, 48)]),
                     Recorder("lost", event="lost", histograms=[Histogram("reflections", 0, 48, 48)])]
    hist, tally = history_launch(scene, rays_of(scene, 8192), n=8192)
    referee = tally_histories(scene, list(hist.histories()))
    for name in ("escaping", "lost"):
        want = referee[name]
        for got in (hist.recorders[name], tally.recorders[name]):
            assert (got.rays, got.crossings) == (want.rays, want.crossings), name
            assert np.array_equal(got._bins[0], want._bins[0]), name
    bins = np.asarray(referee["escaping"]._bins[0])
    print("reflections of the escaping photons", bins[:12].tolist())
    assert bins.sum() > 2000 and np.flatnonzero(bins).max() >= 3 and bins[1:].sum() > 1000


# ---- 4. laws ---------------------------------------------------------------------------------------------------------------------------
N_LAW = 200_000


def first_events(case, theta_deg, inside, n=N_LAW, seed=5):
    """The first surface row of n rays that arrive at one point of the box's top face at `theta_deg`, all alike: kind,
    direction (world), the logged normal and the incoming direction."""
    rays = LC.LobeCase(case.name, case.reflection, case.transmission, case.reflectivity, incidence=(theta_deg, theta_deg))
    rays.n = 4
    pos, dirs, wl, ins, _ = rays.rays()
    k = 1 if inside else 0
    pos, dirs, wl = np.tile(pos[k], (n, 1)), np.tile(dirs[k], (n, 1)), np.full(n, wl[k])
    scene, _ = case.scene()
    with Session(scene, emission="host") as s:
        me = 4                                   # (GENERATE, the event, and room for what follows: a full history ends in KILL)
        r = s.collect(s.submit(n, seed, host_rays=(pos, dirs, wl, ["r"] * n), record_every=1, max_events=me, maxsteps=LC.MAXSTEPS))
        kind = np.asarray(r.data["kind"]).reshape(n, me)[:, 1].copy()
        direction = np.asarray(r.data["direction"]).reshape(n, me, 3)[:, 1].copy()
        normal = np.asarray(r.data["normal"]).reshape(n, me, 3)[0, 1].copy()
    return kind, direction, normal, dirs[0]


def test_law_cosine_lobe_mu_about_the_outgoing_normal_and_a_uniform_azimuth():
    case = LC.BY_NAME["cosine-reflection"]
    kind, out, normal, d = first_events(case, 40.0, inside=False)
    assert np.all(kind == LC.REFLECT)
    n_out = normal if float(np.dot(normal, d)) < 0.0 else -normal
    table = LC.COSINE.table
    mu = np.clip(out @ n_out, -1.0, 1.0)
    assert np.all(mu >= 0.0)
    L.assert_chi2(np.histogram(mu, bins=table.mu)[0], np.diff(table.cdf[0]), "mu about N_out")
    e1, e2 = ray_basis(n_out)
    L.assert_ks(np.arctan2(out @ e2, out @ e1), L.uniform_cdf(-math.pi, math.pi), "azimuth about N_out")
    L.assert_ks(mu ** 2, L.uniform_cdf(0.0, 1.0), "the cosine law")


def test_law_a_normal_lobe_extracts_beyond_the_critical_angle_and_a_refracted_lobe_does_not():
    diffuse = LC.LobeCase("law-normal", transmission=ScatterLobe(LC.COSINE.table, "normal"), reflectivity=0.5)
    kind, out, normal, d = first_events(diffuse, 60.0, inside=True)
    L.assert_binomial(int(np.sum(kind == LC.TRANSMIT)), len(kind), 0.5, "transmitted share at R = 0.5")
    n_out = normal if float(np.dot(normal, d)) > 0.0 else -normal          # a transmission leaves along the ray's side
    assert np.all(out[kind == LC.TRANSMIT] @ n_out >= 0.0)
    guided = LC.LobeCase("law-refracted", transmission=ScatterLobe(LC.COSINE.table, "refracted"), reflectivity=0.5)
    kind, _, _, _ = first_events(guided, 60.0, inside=True, n=20_000)
    assert np.all(kind == LC.REFLECT)


def test_law_host_and_gpu_sample_the_same_lobe():
    case = LC.BY_NAME["gloss-specular-80"]
    kind, out, normal, d = first_events(case, 80.0, inside=False, n=50_000)
    assert np.all(kind == LC.REFLECT)
    np.random.seed(3)
    host = np.array([case.reflection.turn(d, normal, False, 555.0) for _ in range(20_000)])
    n_out = normal if float(np.dot(normal, d)) < 0.0 else -normal
    spec = d - 2.0 * float(np.dot(d, normal)) * normal
    L.assert_ks2(out @ n_out, host @ n_out, "height above the surface")
    L.assert_ks2(out @ spec, host @ spec, "cosine to the specular direction")


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------
def _create(compiled, entry, mutate=None):
    """Call a creation entry with the scene's own structs -> (return code, message, whether a scene came back)."""
    lib = native.load_library()
    st, keep = native.scene_tables_struct(compiled)
    count = dict(native.CREATION_ENTRIES, **dict([native.NEWEST_ENTRY]))[entry]
    made = [native.marshal(t, compiled) for t in native.EXTENSION_TABLES[:count]]
    if mutate is not None:
        mutate(st, keep, made)
    handle = ctypes.c_void_p()
    rc = getattr(lib, entry)(ctypes.byref(st), *[None if m is None else ctypes.byref(m) for m, _ in made], 0, ctypes.byref(handle))
    message = (lib.pvt_last_error() or b"").decode() if rc != 0 else ""
    came_back = bool(handle.value)
    if rc == 0:
        lib.pvt_scene_destroy(handle)
    del keep
    return rc, message, came_back


def test_the_packer_and_the_older_entries_refuse_each_with_its_own_message():
    assert native.NEWEST_ENTRY == ("pvt_scene_create_polyhedra", 10) and len(native.CREATION_ENTRIES) == 11
    case = LC.BY_NAME["sphere-both"]
    fresh = lambda: compile_scene(case.scene()[0])     # noqa: E731  (the structs point INTO the lowered tables)
    newest = native.NEWEST_ENTRY[0]
    assert _create(fresh(), newest) == (0, "", True)
    for entry in native.CREATION_ENTRIES:              # (every entry from before the scattering coatings)
        assert _create(fresh(), entry) == (-1, "coating mode out of range", False), entry

    def word(slot, value):
        def mutate(st, keep, made):
            keep[slot][0] = value
        return mutate

    def no_phase_tables(st, keep, made):
        made[1] = (None, {})

    assert _create(fresh(), newest, word("coat_reflect_mode", COAT_LOBE + 4 * 1 + 0)) == (-1, "coating lobe names a missing phase table", False)
    assert _create(fresh(), newest, word("coat_reflect_mode", COAT_LOBE + 2)) == (-1, "coating lobe axis not legal for a reflection", False)
    assert _create(fresh(), newest, word("coat_reflect_mode", COAT_LOBE + 3)) == (-1, "coating lobe axis not legal for a reflection", False)
    assert _create(fresh(), newest, word("coat_transmit_mode", COAT_LOBE + 1)) == (-1, "coating lobe axis not legal for a transmission", False)
    assert _create(fresh(), newest, no_phase_tables) == (-1, "coating lobe without phase tables", False)
    for bad in (2, COAT_LOBE - 1, -1):
        assert _create(fresh(), newest, word("coat_reflect_mode", bad)) == (-1, "coating mode out of range", False), bad
        assert _create(fresh(), newest, word("coat_transmit_mode", bad)) == (-1, "coating mode out of range", False), bad
    assert native.load_library().pvt_abi_version() == 13


def test_the_host_buffer_entry_refuses_in_python_first():
    case = LC.BY_NAME["cosine-reflection"]
    scene, _ = case.scene()
    x = LC.inputs(case.name)
    with pytest.raises(UnsupportedSceneError, match="scattering coatings"):
        _kernel.trace_bundle(compile_scene(scene), x.pos[:16], x.dirs[:16], x.wl[:16], 1, 100, 16, 0, 1, 0)


# ---- 6. the example ------------------------------------------------------------------------------------------------------------------
def test_diffuse_dots_example_extracts_with_coverage_and_its_specular_twin_extracts_nothing():
    spec = importlib.util.spec_from_file_location("diffuse_dots", os.path.join(ROOT, "examples", "diffuse_dots.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    out = module.main(photons=50_000, coverages=(0.05, 0.4))
    print(out)
    assert out["diffuse"][0] > 0.01 and out["diffuse"][1] > 1.5 * out["diffuse"][0]
    assert out["specular"] == [0.0, 0.0]
