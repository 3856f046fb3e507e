"""Patterned coatings (`Coating(..., pattern=CoatingPattern(...))`, `Coating(None, ...)`) on the GPU.  The kernel is never
its own reference: a pattern of ones is held to the scene without a pattern and a pattern of zeros to the scene without the
coating, a checker to the same coverage written as regions, and every surface event of the event log to the host's
`pattern_cell` on the local point recomputed from the logged position.  Layouts: tests/pattern_scenes.py."""
import importlib.util
import os

import numpy as np
import pytest

from pvtrace_amd import Coating, CoatingPattern, Event, pattern_cell
from pvtrace_amd.engine import (
    Session, _kernel, compile_scene, native, simulate, simulate_stream, tally_histories, trace_stream,
)
from pvtrace_amd.engine.compiler import UnsupportedSceneError
from pvtrace_amd.engine.emit import emit_bundle
from tests import pattern_scenes as P
from tests.capture_scenes import submit

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TALLY_KEYS = ("rec_distinct", "rec_crossings", "rec_bins")
HIST_KEYS = ("counts", "kind", "hit", "container", "adjacent", "component", "source", "position", "direction", "normal",
             "wavelength", "travelled", "duration")
SIZES = (1, 64, 20_000)     # the tail function alone; one wave; several workgroups with refill
SURFACE = (Event.REFLECT.value, Event.TRANSMIT.value, Event.DETECT.value)
MAX_EVENTS = 384


def variant(session):
    return session.dscene.launch_info()["variant"]


def launches(scene, rays, seed=7, max_events=MAX_EVENTS, tally=True):
    """The history launch and the tally launch of the same rays -> (columns, tallies, variant, the two results)."""
    with Session(scene, emission="host") as s:
        h = submit(s, rays, seed, record_every=1, max_events=max_events)
        assert int(np.asarray(h.data["counts"]).max()) < max_events
        columns = {k: np.asarray(h.data[k]).copy() for k in HIST_KEYS + TALLY_KEYS}
        tallies = t = None
        if tally:
            t = submit(s, rays, seed, record_every=0)
            tallies = {k: np.asarray(t.data[k]).copy() for k in TALLY_KEYS + ("rec_sums",)}
        return columns, tallies, variant(s), h, t


def rays_of(scene, n, seed=3):
    pos, dirs, wl, _ = emit_bundle(scene, n, seed=seed)
    return pos, dirs, wl


def same_launches(a, b, what):
    (ah, at), (bh, bt) = a[:2], b[:2]
    for k in HIST_KEYS + TALLY_KEYS:
        assert np.array_equal(ah[k], bh[k], equal_nan=ah[k].dtype.kind == "f"), (what, k)
    for k in TALLY_KEYS:
        assert np.array_equal(at[k], bt[k]), (what, k)
    assert np.allclose(at["rec_sums"], bt["rec_sums"], rtol=1e-12, atol=0), what


def valid_rows(columns, max_events=MAX_EVENTS):
    """Indices of the rows of the flat event log that were written (row k of ray j at j * max_events + k)."""
    counts = columns["counts"]
    keep = np.arange(max_events)[None, :] < counts[:, None]
    return np.flatnonzero(keep.reshape(-1))


def uniform_patterns(layout, value):
    """All ones / all zeros on a lattice that CONTAINS the coated face."""
    if layout == "p3":
        return tuple(CoatingPattern(np.full(s, value, dtype=np.uint8), (-3.0, -3.0, None), (3.0, 3.0, None))
                     for s in ((5, 3, 1), (7, 1, 1)))
    return CoatingPattern(np.full((8, 6, 1), value, dtype=np.uint8), (-6.0, -6.0, None), (6.0, 6.0, None))


# -- 1. all ones is no pattern, all zeros is no coating ------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("layout", sorted(P.LAYOUTS))
def test_ones_trace_as_no_pattern_and_zeros_as_no_coating(layout, n):
    build = P.LAYOUTS[layout][0]
    half_mirror = lambda pattern: Coating(P.TOP, reflectivity=0.6, pattern=pattern)     # (reflects and transmits; absorbs nothing)
    rays = rays_of(build(coating=half_mirror), n)
    plain = launches(build(coating=half_mirror), rays)
    ones = launches(build(coating=half_mirror, pattern=uniform_patterns(layout, 1)), rays)
    same_launches(ones, plain, (layout, n, "ones"))
    bare = launches(build(coating=lambda pattern: None), rays)
    zeros = launches(build(coating=half_mirror, pattern=uniform_patterns(layout, 0)), rays)
    same_launches(zeros, bare, (layout, n, "zeros"))
    assert ones[2] == zeros[2] == "rough", (ones[2], zeros[2])
    assert plain[2] == {"p1": "w4", "p2": "w4", "p3": "grid", "p4": "mesh"}[layout], plain[2]
    if n > 1000:     # the coating mattered: the two pairs differ from each other
        assert not np.array_equal(plain[0]["kind"], bare[0]["kind"])


# -- 2. a pattern is the regions it stands for -------------------------------------------------------------------------------------
def test_checker_pattern_equals_eight_region_coatings_bit_for_bit():
    checker = (np.indices((4, 4, 1)).sum(axis=0) % 2 == 0).astype(np.uint8)
    pattern = CoatingPattern(checker, (-5.0, -5.0, None), (5.0, 5.0, None))
    assert pattern.cell_widths[:2] == (2.5, 2.5)
    as_pattern = P.p1(coating=P.mirror(), pattern=pattern)
    strips = [Coating(P.TOP, reflectivity=1.0, region=((-5.0 + 2.5 * i, -2.5 + 2.5 * i), (-5.0 + 2.5 * j, -2.5 + 2.5 * j), None))
              for i in range(4) for j in range(4) if checker[i, j, 0]]
    assert len(strips) == 8
    as_regions = P.p1(coating=lambda pattern: strips)
    box = compile_scene(as_regions).node_names.index("box")
    rays = rays_of(as_pattern, 20_000)
    got, want = launches(as_pattern, rays), launches(as_regions, rays)
    # open and half-open intervals differ only ON a plane: no hit on the top face lies on one (the inputs are random doubles)
    rows = valid_rows(want[0])
    top = rows[(want[0]["hit"][rows] == box) & (want[0]["normal"].reshape(-1, 3)[rows, 2] == 1.0) & np.isin(want[0]["kind"][rows], SURFACE)]
    xy = want[0]["position"].reshape(-1, 3)[top, :2]
    assert len(top) > 10_000 and not np.any(np.remainder(xy, 2.5) == 0.0)
    same_launches(got, want, "checker")
    assert got[2] == "rough" and want[2] == "w4"
    kinds = want[0]["kind"][top]
    assert np.sum(kinds == Event.REFLECT.value) > 3000 and np.sum(kinds == Event.TRANSMIT.value) > 1000


# -- 3. every surface event, refereed on the host ------------------------------------------------------------------------------------
def referee_rows(scene, columns, names, facet, patterns):
    """Every log row at a patterned node whose normal matches the facet -> (rows checked, DETECT rows, other rows); asserts
    kind == DETECT exactly when `pattern_cell` of the recomputed local point is a set cell."""
    compiled = compile_scene(scene)
    rows = valid_rows(columns)
    kind, hit = columns["kind"][rows], columns["hit"][rows]
    position, normal = columns["position"].reshape(-1, 3)[rows], columns["normal"].reshape(-1, 3)[rows]
    surface = np.isin(kind, SURFACE)
    checked = expected = detected = other = 0
    for name, pattern in zip(names, patterns):
        node = compiled.node_names.index(name)
        at = surface & (hit == node)
        if facet is not None:
            local_normal = normal @ np.asarray(compiled.world_to_local[node])[:3, :3].T
            at &= np.all(np.abs(local_normal - np.asarray(facet)) <= 1e-8 + 1e-5 * np.abs(np.asarray(facet)) + 1e-12, axis=1)
        expected += int(np.sum(at))
        local = P.local_points(scene, name, position[at])
        flat = pattern.mask.reshape(-1)
        for p, k in zip(local, kind[at]):
            slot = pattern_cell(pattern, p)
            covered = slot is not None and bool(flat[slot])
            assert (k == Event.DETECT.value) == covered, (name, p, slot, k)
            checked += 1
            detected += covered
            other += not covered
    assert checked == expected     # no row was skipped
    # and nothing is detected anywhere else
    elsewhere = np.ones(len(rows), dtype=bool)
    for name in names:
        elsewhere &= hit != compiled.node_names.index(name)
    assert not np.any(kind[elsewhere] == Event.DETECT.value)
    return checked, detected, other


@pytest.mark.parametrize("n", (64, 20_000))
@pytest.mark.parametrize("layout", sorted(P.LAYOUTS) + ["sphere"])
def test_every_surface_event_at_a_patterned_face_follows_pattern_cell(layout, n):
    build, make, names, facet = P.SPHERE if layout == "sphere" else P.LAYOUTS[layout]
    made = make(None)
    patterns = P.patterns_of(made)
    assert all(0.25 < p.coverage < 0.45 for p in patterns)
    scene = build(pattern=made)
    rays = rays_of(scene, n)
    columns, tallies, v, hist, tally = launches(scene, rays)
    assert v == "rough"
    checked, detected, other = referee_rows(scene, columns, names, facet, patterns)
    print(layout, n, "rows checked", checked, "DETECT", detected, "other", other)
    if n > 1000:
        assert detected > 200 and other > 200
    # the tally launch's `detected` recorders equal the history launch's, and both the referee's count of the log
    referee = tally_histories(scene, list(hist.histories()))
    total = 0
    for name, rec in tally.recorders.items():
        if rec.spec.event != "detected":
            continue
        got = (rec.rays, rec.crossings)
        assert got == (hist.recorders[name].rays, hist.recorders[name].crossings) == (referee[name].rays, referee[name].crossings), name
        total += rec.rays
    assert total == detected


# -- 4. an exact count ------------------------------------------------------------------------------------------------------------------
def test_detected_count_of_rays_falling_straight_down_is_the_count_of_set_launch_cells():
    pattern = P.face_pattern(None)
    scene = P.p1(pattern=pattern)
    n = 20_000
    rng = np.random.default_rng(21)
    pos = np.column_stack([rng.uniform(-4.9, 4.9, n), rng.uniform(-4.9, 4.9, n), np.full(n, 5.0)])
    dirs = np.tile([0.0, 0.0, -1.0], (n, 1))
    flat = pattern.mask.reshape(-1)
    want = sum(bool(flat[pattern_cell(pattern, p)]) for p in pos)     # (every launch position lies inside the lattice)
    with Session(scene, emission="host") as s:
        r = submit(s, (pos, dirs, np.full(n, 555.0)), 3, record_every=0)
        assert variant(s) == "rough"
    assert 5000 < want < 9000 and r.recorders["detected"].rays == want


# -- 5. the launch does not matter -----------------------------------------------------------------------------------------------------
def test_every_way_of_launching_gives_the_same_integer_tallies():
    scene = P.p1(pattern=P.face_pattern(None))
    n, seed, emit_seed = 90_000, 13, 21
    whole = simulate(scene, n, seed=seed, record_every=0, emission="device", emit_seed=emit_seed)
    assert whole.recorders["detected"].rays > 10_000

    def same_tallies(data, what):
        for k in TALLY_KEYS:
            assert np.array_equal(np.asarray(data[k]), np.asarray(whole.data[k])), (what, k)

    with Session(scene, emission="device") as s:
        same_tallies(s.collect(s.submit(n, seed, record_every=0, emit_seed=emit_seed)).data, "session")
        assert variant(s) == "rough"
    totals = None
    for result, _ in simulate_stream(scene, n, bundle=n // 3, seed=seed, record_every=0, emission="device", emit_seed=emit_seed):
        block = {k: np.asarray(result.data[k]).astype(np.int64) for k in TALLY_KEYS}
        totals = block if totals is None else {k: totals[k] + block[k] for k in TALLY_KEYS}
    same_tallies(totals, "stream")
    compiled, data, _ = trace_stream(scene, n, n // 3 + 1, seed, emit_seed=emit_seed, depth=2)     # (BundlePipeline totals)
    same_tallies(data, "pipeline")
    sharded = simulate(scene, n, seed=seed, record_every=0, emission="device", emit_seed=emit_seed, devices=[0, 0])
    same_tallies(sharded.data, "two shards")


# -- 6. tables in LDS and in global memory -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tables", ["heads", "global"])
def test_tables_read_from_global_memory_give_the_same_logs(tables, monkeypatch):
    made = P.face_pattern(None)
    scene = P.p1(pattern=made)
    rays = rays_of(scene, 20_000)
    want = launches(scene, rays)
    monkeypatch.setenv("PVT_TABLES", tables)
    got = launches(scene, rays)
    monkeypatch.delenv("PVT_TABLES")
    assert got[2] == "rough"
    same_launches(got, want, tables)
    checked, detected, other = referee_rows(scene, got[0], ("box",), P.TOP, (made,))
    assert detected > 200 and other > 200


# -- 7. roughness in the holes -------------------------------------------------------------------------------------------------------------
def test_covered_points_of_a_rough_node_reflect_specularly_and_the_holes_are_rough():
    made = P.face_pattern(None)
    rough = P.p1(coating=P.mirror(), pattern=made, roughness=0.3)
    smooth = P.p1(coating=P.mirror(), pattern=made, roughness=0.0)
    rays = rays_of(rough, 20_000)
    got, _, v, _, _ = launches(rough, rays, tally=False)
    ref = launches(smooth, rays, tally=False)[0]
    assert v == "rough"
    box = compile_scene(rough).node_names.index("box")
    # the FIRST surface event of every ray is at the same point in both scenes (row 1; row 0 is GENERATE)
    first = np.arange(len(rays[2])) * MAX_EVENTS + 1
    ok = (got["counts"] > 1) & np.isin(got["kind"][first], SURFACE)
    first = first[ok]
    position, normal = got["position"].reshape(-1, 3), got["normal"].reshape(-1, 3)
    direction, incoming = got["direction"].reshape(-1, 3), got["direction"].reshape(-1, 3)[first - 1]
    assert np.array_equal(position[first], ref["position"].reshape(-1, 3)[first])
    at_top = (got["hit"][first] == box) & (normal[first, 2] == 1.0)
    flat = made.mask.reshape(-1)
    covered = np.zeros(len(first), dtype=bool)
    for i in np.flatnonzero(at_top):
        slot = pattern_cell(made, position[first[i]])     # (unrotated at the origin: the local point is the world point)
        covered[i] = slot is not None and bool(flat[slot])
    assert np.sum(covered) > 1000 and np.sum(at_top & ~covered) > 1000
    # covered: the mirror reflects every photon, specularly -- d - 2 (d.n) n with the normal flipped along the ray, bit for bit
    rows, d, nrm = first[covered], incoming[covered], normal[first[covered]]
    dd = nrm[:, 0] * d[:, 0] + nrm[:, 1] * d[:, 1] + nrm[:, 2] * d[:, 2]
    flip = dd < 0.0
    nf, dd = np.where(flip[:, None], -nrm, nrm), np.where(flip, -dd, dd)
    assert np.all(got["kind"][rows] == Event.REFLECT.value)
    assert np.array_equal(direction[rows], d - (2.0 * dd)[:, None] * nf)
    assert np.array_equal(direction[rows], ref["direction"].reshape(-1, 3)[rows])
    # uncovered: the rough path -- the outgoing directions differ from the smooth scene's
    holes = first[at_top & ~covered]
    differ = np.any(direction[holes] != ref["direction"].reshape(-1, 3)[holes], axis=1)
    print("holes", len(holes), "of which differ", int(np.sum(differ)))
    assert np.sum(differ) > 0.99 * len(holes)


# -- 8. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_host_buffer_entry_refuses_and_python_never_reaches_the_older_entry(monkeypatch):
    # (mirrors: an absorbing coating would be refused for its absorptivity first)
    for scene in (P.p1(coating=P.mirror(), pattern=P.face_pattern(None)), P.sphere(coating=lambda pattern: Coating(None, reflectivity=0.5))):
        with pytest.raises(UnsupportedSceneError, match="patterned coatings"):
            _kernel.trace_bundle(compile_scene(scene), *rays_of(scene, 16), 1, 100, 16, 0, 1, 0)
    lib = native.load_library()
    reached = []
    real = lib.pvt_scene_create_origin
    monkeypatch.setattr(lib, "pvt_scene_create_origin", lambda *a: reached.append(a) or real(*a))
    scene = P.p1(pattern=P.face_pattern(None))
    r = simulate(scene, 4096, seed=2, record_every=0)
    assert r.recorders["detected"].rays > 100 and not reached
    assert native.load_library().pvt_abi_version() == 13


# -- 9. the example ------------------------------------------------------------------------------------------------------------------------
def test_dot_pattern_example_graded_dots_are_more_uniform():
    spec = importlib.util.spec_from_file_location("dot_pattern", os.path.join(ROOT, "examples", "dot_pattern.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    out = module.main(photons=200_000)
    print(out)
    assert 0.0 < out["uniform"]["uniformity"] < out["graded"]["uniformity"] <= 1.0
    assert out["uniform"]["outcoupled"] > 1000 and out["graded"]["outcoupled"] > 1000
