"""Path-length volume maps (`VolumeMap(event="pathlength")`) on the GPU: the kernel's walk (`path_map_call`,
pvt_trace_kernel.h) held to integers.  An exact anchor whose every slot is known by hand; single segments whose inputs
the event log gives bit for bit, walked again on the host (`engine.tally`, pure Python floats, the contract's operation
order) and compared INTEGER FOR INTEGER; whole histories against the event log within one unit per piece; the launch
geometry (carried launches, streams, tally sets, a ray alone); the maps drawing nothing; the martingale law that ties
`absorbed` to alpha x `pathlength`; the packer's refusal; the example.

Measured on an MI355X: the four single-segment scenes equal the host walk integer for integer; on whole histories the
worst |GPU - host| over all slots was 0 units (allowed: the pieces of the slot, up to 42 426); the martingale's worst
|z| per cell 2.92, for the whole map -0.86 (docs/parity_chain.md, path-length maps)."""
import ctypes as C
import importlib.util
import math
import os

import numpy as np
import pytest

from pvtrace_amd import Absorber, Box, Material, Node, Scene, Surface, VolumeMap
from pvtrace_amd.engine import Session, compile_scene, map_histories, native, simulate, simulate_stream, trace_stream
from pvtrace_amd.engine.api import maps_from_slots
from pvtrace_amd.engine.emit import emit_bundle
from pvtrace_amd.engine.tally import path_map_slots
from pvtrace_amd.material import NullSurfaceDelegate
from tests import broken_tables as BT
from tests import exact_march as X
from tests import pathlength_cases as P
from tests import scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLAB_LO, SLAB_HI = (-2.5, -2.5, -0.5), (2.5, 2.5, 0.5)
HIST_KEYS = ("counts", "kind", "hit", "container", "component", "position", "direction", "wavelength", "duration", "travelled")
TALLY_KEYS = ("rec_distinct", "rec_crossings", "rec_bins")
EVENT_MAPS = ("absorbed", "emitted", "scattered", "lost", "reacted")


def node(scene, name):
    return next(n for n in scene.root.preorder() if n.name == name)


def submit(session, rays, seed, **kw):
    pos, dirs, wl = rays
    return session.collect(session.submit(len(wl), seed, host_rays=(pos, dirs, wl, ["r"] * len(wl)), **kw))


def same_maps(a, b):
    assert sorted(a) == sorted(b)
    for name in a:
        assert np.array_equal(a[name].counts, b[name].counts), name
        assert a[name].outside == b[name].outside, name


def thin_block(components, name="slab"):
    """A 2 x 2 x 1 block of index 1.0 in a world of index 1.0: no reflection, no refraction."""
    world = Node(name="world", geometry=Box((40.0, 40.0, 40.0), material=Material(refractive_index=1.0)))
    body = Node(name=name, parent=world, geometry=Box((2.0, 2.0, 1.0), material=Material(
        refractive_index=1.0, surface=Surface(NullSurfaceDelegate()), components=components)))
    return Scene(world), body


# -- 1. the exact anchor -----------------------------------------------------------------------------------------------------
def test_anchor_a_clear_box_crossed_on_the_columns_centres_holds_the_integers_known_by_hand():
    scene, body = thin_block([])
    body.volume_maps = [VolumeMap("path", (4, 4, 2), (-1.0, -1.0, -0.5), (1.0, 1.0, 0.5), event="pathlength")]
    centres = np.array([-0.75, -0.25, 0.25, 0.75])
    xy = np.array([(x, y) for x in centres for y in centres for _ in range(4)])        # four rays per column
    pos = np.column_stack([xy, np.full(64, 5.0)])
    dirs = np.tile([0.0, 0.0, -1.0], (64, 1))
    with Session(scene, emission="host") as s:
        result = submit(s, (pos, dirs, np.full(64, 555.0)), 3, record_every=0)
    path = result.volume_maps["path"]
    assert np.array_equal(path.counts, np.full((4, 4, 2), 4 * 2 ** 29, dtype=np.int64)) and path.outside == 0
    assert path.unit == 2.0 ** -30 and np.all(path.pathlength == 2.0) and np.all(path.fluence == 2.0 / 0.125)


# -- 2. one segment, bit for bit against the host walk -----------------------------------------------------------------------
P_SEED = 12345
_PLAIN = [(0.9, "plain")]       # one Absorber (quantum yield 0), no lattice: the scenes of tests/exact_march.py without a field
FULL_LO, FULL_HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
SEGMENT_CASES = {
    "box": (X.Case("P-box", "A", (4, 3, 2), _PLAIN, seed=21, n=256), (4, 3, 2), FULL_LO, FULL_HI),
    "rotated-box-roi": (X.Case("P-rotated", "A", (3, 5, 7), _PLAIN, rotate=X.ROT, location=(0.3, -1.7, 2.9), seed=22, n=256),
                        (3, 5, 7), (-0.7, -0.85, -0.45), (0.9, 0.6, 0.8)),      # smaller than the node
    "tile": (X.Case("P-tile", "A", (2, 2, 5), _PLAIN, container="tile", seed=23, n=256), (2, 2, 5), FULL_LO, FULL_HI),
    "mesh": (X.Case("P-mesh", "A", (6, 1, 2), _PLAIN, container="mesh", rotate=X.ROT, location=(-2.1, 0.4, 0.77), seed=24, n=256),
             (6, 1, 2), FULL_LO, FULL_HI),
}


@pytest.mark.parametrize("name", sorted(SEGMENT_CASES))
def test_one_segment_per_ray_equals_the_host_walk_integer_for_integer(name):
    case, shape, lower, upper = SEGMENT_CASES[name]
    scene, body = case.scene(fielded=False)
    body.volume_maps = [VolumeMap("path", shape, lower, upper, event="pathlength"),
                        VolumeMap("all", (1, 1, 1), lower, upper, event="pathlength")]
    compiled = compile_scene(scene)
    node_id = compiled.nodes.index(body)
    pos, dirs = case.world_rays(compiled, node_id)
    n, me = case.n, 8
    # ONE step per photon (maxsteps=1: the second step is its KILL row, which advances nothing): exactly one segment, in
    # the node, whatever the photon would have met afterwards (a tile's neighbours reflect)
    with Session(scene, emission="host") as s:
        result = submit(s, (pos, dirs, np.full(n, case.wavelength)), P_SEED, record_every=1, max_events=me, maxsteps=1)
        data = {k: np.asarray(result.data[k]).copy() for k in ("counts", "kind", "container", "travelled", "position", "direction")}
        kernel = result.volume_maps
    first = np.arange(n) * me
    position, direction = data["position"].reshape(-1, 3), data["direction"].reshape(-1, 3)
    assert np.all(data["counts"] >= 2) and np.all(data["kind"][first] == P.GENERATE)
    assert np.array_equal(position[first], pos) and np.array_equal(direction[first], dirs)      # row 0: x and d exactly
    kind = data["kind"][first + 1]
    assert np.all(data["container"][first + 1] == node_id)
    assert np.all(np.isin(kind, (P.ABSORB, P.TRANSMIT))) and 20 < (kind == P.ABSORB).sum() < n - 20   # both ends occur
    adv = data["travelled"][first + 1]                                                            # 0 + adv: bit for bit
    assert np.all(adv > 0.0)
    for j in range(n):      # ... and nothing after it moved: every later row is where row 1 is
        rows = slice(j * me + 1, j * me + int(data["counts"][j]))
        assert np.all(data["travelled"][rows] == adv[j])
    histories = [P.segment_history(compiled.node_names[node_id], pos[j], dirs[j], float(adv[j]), wavelength=case.wavelength)
                 for j in range(n)]
    host = map_histories(compiled, histories)
    same_maps(kernel, host)
    assert kernel["path"].total > 0 and np.count_nonzero(kernel["path"].counts) > kernel["path"].counts.size // 2
    if name == "rotated-box-roi":
        assert kernel["path"].outside > 0
    else:
        assert kernel["path"].outside == 0 and kernel["all"].outside == 0


# -- 3. many segments, against the event log ------------------------------------------------------------------------------------
def lumogen_slab():
    scene = scenes.lsc_equivalent(recorders=False)
    node(scene, "LSC").volume_maps = [VolumeMap("path", (8, 8, 4), SLAB_LO, SLAB_HI, event="pathlength"),
                                      VolumeMap("all", (1, 1, 1), SLAB_LO, SLAB_HI, event="pathlength")]
    return scene


def test_whole_histories_agree_with_the_event_log_within_one_unit_per_piece():
    scene = lumogen_slab()
    n, max_events = 8192, 512
    pos, dirs, wl, _ = emit_bundle(scene, n, seed=3)
    with Session(scene, emission="host") as s:
        hist = submit(s, (pos, dirs, wl), 7, record_every=1, max_events=max_events)
        tally = submit(s, (pos, dirs, wl), 7, record_every=0)
    assert int(np.asarray(hist.data["counts"]).max()) < max_events          # no history was cut
    kernel = hist.volume_maps
    same_maps(kernel, tally.volume_maps)                                    # a tally-only launch of the same rays and seed
    compiled = hist.compiled
    histories = list(hist.histories())
    host, pieces = path_map_slots(compiled, histories)
    got = np.asarray(hist.data["map_bins"]).astype(np.int64)
    worst = int(np.abs(got - host).max())
    print(f"whole histories: worst |GPU - host| {worst} units; pieces per slot up to {int(pieces.max())}")
    assert np.all(np.abs(got - host) <= pieces), (worst, int(np.argmax(np.abs(got - host) - pieces)))
    # re-emission and total internal reflection were there: more segments in the slab than rays
    inside = sum(1 for h in histories for (a, _, _), (b, _, m) in zip(h, h[1:])
                 if m["container"] == "LSC" and b.travelled > a.travelled)
    travelled = sum(b.travelled - a.travelled for h in histories for (a, _, _), (b, _, m) in zip(h, h[1:])
                    if m["container"] == "LSC" and b.travelled > a.travelled)
    assert inside > n + n // 2
    # conservation (item 14): every map's slots together are the path travelled in the node, half a unit per piece (and one
    # per piece for the `travelled` differences that stand in for the kernel's advances)
    for name, lo in zip(compiled.map_names, compiled.map_offset):
        m = kernel[name]
        p = int(pieces[int(lo):int(lo) + m.spec.size].sum())
        assert m.outside == 0                                               # the lattices cover the slab
        assert abs(m.total - travelled * 2.0 ** 30) <= 1.5 * p + 1e-9 * m.total, (name, m.total, travelled * 2.0 ** 30, p)
    assert abs(kernel["path"].total - kernel["all"].total) <= int(pieces.sum())


# -- 4. the launch does not matter ------------------------------------------------------------------------------------------------
def launch_scene():
    scene = scenes.lsc_equivalent()
    slab = node(scene, "LSC")
    slab.recorders = [r for r in slab.recorders if r.name not in EVENT_MAPS + ("path",)]
    slab.volume_maps = [VolumeMap("path", (8, 8, 4), SLAB_LO, SLAB_HI, event="pathlength", wavelength=(400.0, 800.0, 4)),
                        VolumeMap("absorbed", (8, 8, 4), SLAB_LO, SLAB_HI),
                        VolumeMap("roi", (2, 2, 1), (-1.0, -1.0, -0.25), (1.0, 1.5, 0.5), event="pathlength")]
    return scene


def test_carried_launches_streams_and_a_ray_alone_give_the_same_integers():
    scene = launch_scene()
    n, seed, emit_seed = 200_000, 13, 21
    whole = simulate(scene, n, seed=seed, record_every=0, emission="device", emit_seed=emit_seed)
    maps = whole.volume_maps
    assert maps["path"].total > n * 2 ** 28 and maps["roi"].outside > 0 and maps["roi"].counts.min() > 0
    # carried launches: three bundles on a pipeline whose launches hand their live photons on
    for depth in (1, 2):
        compiled, data, _ = trace_stream(scene, n, n // 3 + 1, seed, emit_seed=emit_seed, depth=depth)
        same_maps(maps, maps_from_slots(compiled, data["map_bins"]))
    # a stream of bundles, one map set per bundle (tally sets of grouped launches), summed
    total, bundles = None, 0
    for result, _ in simulate_stream(scene, n, bundle=10_000, seed=seed, record_every=0, emission="device",
                                     emit_seed=emit_seed):
        part = np.asarray(result.data["map_bins"]).astype(np.int64)
        total = part.copy() if total is None else total + part
        bundles += 1
    assert bundles == 20
    same_maps(maps, maps_from_slots(whole.compiled, total))
    with Session(scene, emission="device") as s:
        # a ray alone (a launch of one photon finishes in the tail function) and the rest around it
        for i in (0, 123_457, n - 1):
            parts = [s.collect(s.submit(b - a, seed, record_every=0, emit_seed=emit_seed, ray_offset=a))
                     for a, b in ((0, i), (i, i + 1), (i + 1, n)) if b > a]
            total = sum(np.asarray(p.data["map_bins"]).astype(np.int64) for p in parts)
            same_maps(maps, maps_from_slots(whole.compiled, total))


# -- 5. it draws nothing ------------------------------------------------------------------------------------------------------------
def test_a_path_length_map_changes_no_recorder_no_event_map_and_no_history():
    def scene_of(with_path):
        scene = scenes.lsc_equivalent()
        slab = node(scene, "LSC")
        slab.volume_maps = [VolumeMap(f"map-{e}", (8, 8, 4), SLAB_LO, SLAB_HI, event=e) for e in EVENT_MAPS]
        if with_path:
            slab.volume_maps.insert(2, VolumeMap("map-path", (8, 8, 4), SLAB_LO, SLAB_HI, event="pathlength"))
        return scene

    plain, mapped = scene_of(False), scene_of(True)
    pos, dirs, wl, _ = emit_bundle(plain, 100_000, seed=3)
    out = []
    for scene in (plain, mapped):
        with Session(scene, emission="host") as s:
            h = submit(s, (pos[:20_000], dirs[:20_000], wl[:20_000]), 7, record_every=1, max_events=64)
            t = submit(s, (pos, dirs, wl), 7, record_every=0)
            out.append(({k: np.asarray(h.data[k]).copy() for k in HIST_KEYS + TALLY_KEYS}, h.volume_maps,
                        {k: np.asarray(t.data[k]).copy() for k in TALLY_KEYS + ("rec_sums",)}, t.volume_maps))
    for k in HIST_KEYS + TALLY_KEYS:
        assert np.array_equal(out[0][0][k], out[1][0][k]), k
    for k in TALLY_KEYS:
        assert np.array_equal(out[0][2][k], out[1][2][k]), k
    assert np.allclose(out[0][2]["rec_sums"], out[1][2]["rec_sums"], rtol=1e-12, atol=0)   # (float atomics: order only)
    for launch in (1, 3):
        with_path = dict(out[1][launch])
        assert with_path.pop("map-path").total > 0
        same_maps(out[0][launch], with_path)
        assert out[0][launch]["map-absorbed"].total > 0


def test_a_scene_with_aligned_components_takes_a_path_length_map_and_keeps_its_histories():
    """The kernels that hold the walk hold the aligned components' code too: an aligned slab traced with and without a
    path-length map gives the same histories, recorders and event maps, and its path-length map agrees with its log."""
    from tests import aligned_scenes as A

    def scene_of(with_path):
        scene = A.slab_scene([A.luminophore(3.0, (0.0, 0.6, 0.8), 0.6, 0.6, name="dye"),
                              A.absorber(0.3, (1.0, 0.0, 0.0), -0.5, name="host")], rotate=A.TILT, index=1.5)
        slab = node(scene, "slab")
        lo, hi = (-2.0, -2.0, -0.5), (2.0, 2.0, 0.5)
        slab.volume_maps = [VolumeMap("absorbed", (4, 4, 2), lo, hi), VolumeMap("emitted", (2, 2, 1), lo, hi, event="emitted")]
        if with_path:
            slab.volume_maps.append(VolumeMap("path", (4, 4, 2), lo, hi, event="pathlength"))
        return scene

    rays, _ = A.pencil(30.0, 4096, rotate=A.TILT)
    out = []
    for scene in (scene_of(False), scene_of(True)):
        with Session(scene, emission="host") as s:
            h = submit(s, rays, 7, record_every=1, max_events=256)
            assert int(np.asarray(h.data["counts"]).max()) < 256
            out.append(({k: np.asarray(h.data[k]).copy() for k in HIST_KEYS}, h.volume_maps, h))
    for k in HIST_KEYS:
        assert np.array_equal(out[0][0][k], out[1][0][k]), k
    mapped = dict(out[1][1])
    path = mapped.pop("path")
    same_maps(out[0][1], mapped)
    assert out[0][1]["absorbed"].total > 2048 and out[0][1]["emitted"].total > 2048 and path.total > 0
    hist = out[1][2]
    host, pieces = path_map_slots(hist.compiled, list(hist.histories()))
    got = np.asarray(hist.data["map_bins"]).astype(np.int64)
    at = int(hist.compiled.map_offset[2])
    assert np.all(host[:at] == 0) and np.all(np.abs(got - host)[at:] <= pieces[at:])


# -- 6. the physical law ---------------------------------------------------------------------------------------------------------------
def test_absorptions_minus_alpha_times_track_length_is_a_martingale():
    """A_c - alpha L_c has mean 0 and variance E[alpha L_c] in every cell (the collision and the track-length estimator
    of the same absorption rate): z = (A_c - alpha L_c) / sqrt(alpha L_c), |z| < 5 per cell and for the whole map."""
    alpha, n = 1.0, 200_000
    scene, body = thin_block([Absorber(alpha, name="ink")])
    lo, hi = (-1.0, -1.0, -0.5), (1.0, 1.0, 0.5)
    body.volume_maps = [VolumeMap("absorbed", (4, 4, 2), lo, hi), VolumeMap("path", (4, 4, 2), lo, hi, event="pathlength")]
    rng = np.random.default_rng(2024)
    pos = np.column_stack([rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n), np.full(n, 5.0)])
    dirs = np.tile([0.0, 0.0, -1.0], (n, 1))
    with Session(scene, emission="host") as s:
        result = submit(s, (pos, dirs, np.full(n, 555.0)), 99, record_every=0)
    absorbed, path = result.volume_maps["absorbed"], result.volume_maps["path"]
    assert absorbed.outside == 0 and path.outside == 0 and absorbed.counts.min() > 2000
    expect = alpha * path.pathlength
    z = (absorbed.counts - expect) / np.sqrt(expect)
    z_all = (absorbed.counts.sum() - expect.sum()) / math.sqrt(expect.sum())
    print(f"martingale: worst |z| per cell {np.abs(z).max():.2f}, whole map z {z_all:.2f}")
    assert np.all(np.abs(z) < 5.0), z
    assert abs(z_all) < 5.0
    # (and the track length itself: sum L = n (1 - exp(-alpha d)) / alpha in expectation, d = 1)
    assert abs(path.pathlength.sum() / n - (1.0 - math.exp(-alpha)) / alpha) < 5.0 / math.sqrt(n)


# -- 7. the packer -----------------------------------------------------------------------------------------------------------------------
def test_the_packer_takes_the_kind_and_refuses_a_component_filter_on_it():
    compiled = compile_scene(BT.map_scene())
    lib = native.load_library()
    st, keep = native.scene_tables_struct(compiled)

    def attempt(n_nodes=2, **change):
        mt, held = BT.map_tables(n_nodes, **change)
        handle = C.c_void_p()
        rc = lib.pvt_scene_create_maps(C.byref(st), None, None, None, None, C.byref(mt), 0, C.byref(handle))
        if rc == 0:
            slots = lib.pvt_scene_map_slots(handle)
            lib.pvt_scene_destroy(handle)
            return slots
        assert not handle.value
        return lib.pvt_last_error().decode()

    kinds = np.array([3, 100], np.int32)
    assert attempt(map_kind=kinds, map_component=np.array([-1, -1], np.int32)) == BT.MAP_SLOTS
    refused = attempt(map_kind=kinds)                     # (the second map of the fixture filters by component 1)
    assert isinstance(refused, str) and "map tables" in refused and "path-length map takes no component filter" in refused
    others = [attempt(**change) for change in BT.MAP_BREAKS.values()]
    assert refused not in others
    unknown = attempt(map_kind=np.array([3, 101], np.int32))
    assert isinstance(unknown, str) and "map kind must be" in unknown and "PVT_MAP_PATHLENGTH" in unknown


# -- 8. the example ------------------------------------------------------------------------------------------------------------------------
def test_fluence_example_follows_the_exponential_within_five_sigma():
    spec = importlib.util.spec_from_file_location("fluence_map", os.path.join(ROOT, "examples", "fluence_map.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    out = module.main(photons=100_000)
    assert out["clear"]["worst_sigma"] < 5.0 and out["absorbing"]["worst_sigma"] < 5.0
    assert out["absorbing"]["absorbed_vs_path_worst_sigma"] < 5.0
    assert np.allclose(out["clear"]["profile"], 1.0, rtol=0, atol=1e-6)      # nothing absorbs: the fluence does not fall
