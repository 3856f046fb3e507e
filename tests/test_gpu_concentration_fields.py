"""Concentration fields (`ConcentrationGrid`) on the GPU.  The CPU referee knows no fields, so the engine is held to the
closed-form piecewise-exponential law of the march (tests/test_concentration_fields.py writes the chord's optical depth
from its sorted plane crossings), to the host Python tracer in distribution, and to itself: a 1 x 1 x 1 field of value 1
is today's engine bit for bit, and a ray's history does not depend on the launch, the mode or the split."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from pvtrace_amd import Absorber, Box, ConcentrationGrid, Luminophore, Material, Node, Ray, Reactor, Scene, Surface
from pvtrace_amd.algorithm import photon_tracer
from pvtrace_amd.engine import Histogram, Recorder, Session, compile_scene, native
from pvtrace_amd.engine.emit import emit_bundle
from pvtrace_amd.material import NullSurfaceDelegate
from tests import broken_tables as BT
from tests import laws as L
from tests import scenes
from tests.test_concentration_fields import chord_depth, depth_cdf
from tests.test_gpu_laws import Gpu

pytestmark = pytest.mark.gpu

B = Gpu()
ABSORB, NONRADIATIVE, REACT = 3, 4, 8
HIST_KEYS = ("counts", "kind", "position", "direction", "wavelength", "duration")
TALLY_KEYS = ("rec_distinct", "rec_crossings", "rec_bins")
LO, HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)


def block_scene(components, angle=None, axis=None, recorders=()):
    """An index-matched 2 cm cube (n = 1, NullSurfaceDelegate) in an n = 1 world, optionally rotated."""
    world = Node(name="world", geometry=Box((40.0, 40.0, 40.0), material=Material(refractive_index=1.0)))
    block = Node(name="block", parent=world, geometry=Box((2.0, 2.0, 2.0), material=Material(
        refractive_index=1.0, surface=Surface(NullSurfaceDelegate()), components=components)))
    block.recorders = list(recorders)
    if angle is not None:
        block.rotate(angle, axis)
    return Scene(world)


def first_absorptions(scene, start, d, wavelength=555.0, seed=11, n=None):
    """Rays enter the block (row 1, TRANSMIT), then row 2 is ABSORB or the TRANSMIT out: (absorbed mask, rows)."""
    n = B.n_hist if n is None else n
    data, _ = B.trace_pencil(scene, start, d, wavelength, n, seed=seed, record_every=1, max_events=6)
    me = 6
    counts = np.asarray(data["counts"])
    assert np.all(counts >= 3)
    idx = np.arange(counts.size) * me
    kind = np.asarray(data["kind"])
    assert np.all(kind[idx + 1] == 2)
    absorbed = kind[idx + 2] == ABSORB
    pos = np.asarray(data["position"]).reshape(-1, 3)
    return absorbed, pos[idx + 1], pos[idx + 2], kind[idx + 3]


# -- 1. laws ------------------------------------------------------------------------------------------------------------
def test_z_gradient_at_normal_incidence():
    values = np.linspace(0.05, 2.0, 8).reshape(1, 1, 8)
    grid = ConcentrationGrid(values, LO, HI)
    scene = block_scene([Absorber(0.9, concentration=grid)])
    start, d = np.array([0.1, -0.2, -5.0]), np.array([0.0, 0.0, 1.0])
    absorbed, entry, where, _ = first_absorptions(scene, start, d)
    s, tau = chord_depth(LO, HI, 0.9 * values, (0.1, -0.2, -1.0), d, 2.0)
    L.assert_binomial(int(absorbed.sum()), absorbed.size, 1.0 - math.exp(-tau[-1]), "P(absorbed), z gradient")
    L.assert_ks(where[absorbed, 2] + 1.0, depth_cdf(s, tau), "depth, z gradient")


def test_oblique_pencil_through_a_checkerboard_in_a_rotated_node():
    ix, iy, iz = np.indices((4, 3, 5))
    values = np.where((ix + iy + iz) % 2 == 0, 1.6, 0.0)
    grid = ConcentrationGrid(values, LO, HI)
    angle, axis = 0.7, (0.3, -1.0, 0.6)
    scene = block_scene([Absorber(0.8, concentration=grid)], angle, axis)
    R = L.rotation(angle, axis)
    ld = np.array([0.45, 0.3, 1.0])
    ld /= np.linalg.norm(ld)
    local_entry = np.array([-0.3, -0.2, -1.0])          # on the bottom face; leaves through the top (z = +1)
    t0 = 2.0 / ld[2]
    start, d = R @ (local_entry - 4.0 * ld), R @ ld
    absorbed, _, where, _ = first_absorptions(scene, start, d)
    s, tau = chord_depth(LO, HI, 0.8 * values, local_entry, ld, t0)
    L.assert_binomial(int(absorbed.sum()), absorbed.size, 1.0 - math.exp(-tau[-1]), "P(absorbed), checkerboard")
    local = L.to_local(where[absorbed], R)
    depth = (local - local_entry) @ ld
    L.assert_ks(depth, depth_cdf(s, tau), "depth, checkerboard")
    h = (np.array(HI) - np.array(LO)) / np.array(values.shape)
    f = (local - np.array(LO)) / h
    away = np.all(np.abs(f - np.round(f)) > 1e-6, axis=1)
    cell = np.clip(np.floor(f[away]), 0, np.array(values.shape) - 1).astype(int)
    assert np.all(values[cell[:, 0], cell[:, 1], cell[:, 2]] > 0.0)   # never in a clear cell


def test_two_components_with_different_fields():
    fa = ConcentrationGrid(np.array([[[1.0, 0.2, 0.0, 0.7]]]), LO, HI)
    fb = ConcentrationGrid(np.array([[[0.0, 2.0, 1.0, 0.7]]]), LO, HI)
    scene = block_scene([Absorber(0.6, concentration=fa, name="a"), Reactor(0.9, concentration=fb, name="b")])
    d = np.array([0.0, 0.0, 1.0])
    absorbed, _, where, after = first_absorptions(scene, (0.3, 0.3, -5.0), d)
    coef = 0.6 * fa.values + 0.9 * fb.values
    s, tau = chord_depth(LO, HI, coef, (0.3, 0.3, -1.0), d, 2.0)
    L.assert_binomial(int(absorbed.sum()), absorbed.size, 1.0 - math.exp(-tau[-1]), "P(absorbed), two fields")
    z = where[absorbed, 2]
    L.assert_ks(z + 1.0, depth_cdf(s, tau), "depth, two fields")
    took = after[absorbed]
    assert np.all((took == NONRADIATIVE) | (took == REACT))
    cell = np.clip(np.floor((z + 1.0) / 0.5), 0, 3).astype(int)
    for c in range(4):
        w1, w2 = 0.6 * fa.values[0, 0, c], 0.9 * fb.values[0, 0, c]
        here = took[cell == c]
        if w1 + w2 == 0.0:
            assert here.size == 0
            continue
        L.assert_binomial(int(np.sum(here == NONRADIATIVE)), here.size, w1 / (w1 + w2), ("pick", c))


@pytest.mark.parametrize("wavelength", [480.0, 650.0])
def test_two_wavelengths(wavelength):
    x = np.array([400.0, 500.0, 600.0, 700.0])
    spectrum = np.column_stack([x, [2.0, 1.2, 0.5, 0.2]])
    values = np.linspace(0.3, 1.5, 6).reshape(1, 1, 6)
    grid = ConcentrationGrid(values, LO, HI)
    scene = block_scene([Absorber(spectrum, concentration=grid)])
    alpha = float(np.interp(wavelength, x, spectrum[:, 1]))
    d = np.array([0.0, 0.0, 1.0])
    absorbed, _, where, _ = first_absorptions(scene, (0.0, 0.0, -5.0), d, wavelength=wavelength)
    s, tau = chord_depth(LO, HI, alpha * values, (0.0, 0.0, -1.0), d, 2.0)
    L.assert_binomial(int(absorbed.sum()), absorbed.size, 1.0 - math.exp(-tau[-1]), ("P(absorbed)", wavelength))
    L.assert_ks(where[absorbed, 2] + 1.0, depth_cdf(s, tau), ("depth", wavelength))


def test_tally_histogram_of_lost_events_follows_the_cells():
    values = np.array([[[0.2, 1.5, 0.0, 0.8, 2.5, 0.4, 1.0, 0.1]]])
    grid = ConcentrationGrid(values, LO, HI)
    rec = Recorder("lost", event="lost", histograms=[Histogram("z", -1.0, 1.0, 8)])
    scene = block_scene([Absorber(1.1, concentration=grid)], recorders=[rec])
    d = np.array([0.0, 0.0, 1.0])
    n = B.n_tally
    total, compiled = B.trace_pencil(scene, (0.2, 0.1, -5.0), d, 555.0, n, seed=17, record_every=0)
    bins = np.asarray(total["rec_bins"])[:8]
    s, tau = chord_depth(LO, HI, 1.1 * values, (0.2, 0.1, -1.0), d, 2.0)
    edges = np.exp(-np.interp(np.linspace(0.0, 2.0, 9), s, tau))
    probs = np.append(edges[:-1] - edges[1:], edges[-1])
    assert bins[2] == 0   # the clear cell
    keep = probs > 0.0
    counts = np.append(bins, n - bins.sum())
    L.assert_chi2(counts[keep], probs[keep] / probs[keep].sum(), "lost z histogram")


# -- 2. the host tracer -----------------------------------------------------------------------------------------------
def luminophore_block():
    x = np.linspace(400.0, 800.0, 41)
    ix, iy, iz = np.indices((3, 2, 4))
    grid = ConcentrationGrid(0.2 + ((ix + 2 * iy + iz) % 3), LO, HI)
    lum = Luminophore(np.column_stack([x, 1.5 * np.exp(-((x - 520.0) / 80.0) ** 2)]),
                      emission=np.column_stack([x, np.exp(-((x - 560.0) / 50.0) ** 2)]), quantum_yield=0.95,
                      concentration=grid)
    return block_scene([lum], 0.5, (1.0, 1.0, 0.0))


def test_host_tracer_and_gpu_agree_on_absorption_positions():
    scene = luminophore_block()
    R = L.rotation(0.5, (1.0, 1.0, 0.0))
    start, d = R @ np.array([0.2, -0.1, -4.0]), R @ np.array([0.0, 0.0, 1.0])
    data, _ = B.trace_pencil(scene, start, d, 480.0, 200_000, seed=3, record_every=1, max_events=64, emit_method=1)
    kind = np.asarray(data["kind"])
    counts = np.asarray(data["counts"])
    valid = (np.arange(64)[None, :] < counts[:, None]).ravel()
    pos = np.asarray(data["position"]).reshape(-1, 3)
    gpu = L.to_local(pos[(kind == ABSORB) & valid], R)
    np.random.seed(4)
    host = []
    for _ in range(2500):
        for r, e in photon_tracer.follow(scene, Ray(tuple(start), tuple(d), 480.0), emit_method="redshift",
                                         backend="host"):
            if e.name == "ABSORB":
                host.append(r.position)
    host = L.to_local(np.array(host), R)
    per_ray = ((kind == ABSORB) & valid).reshape(-1, 64).sum(axis=1)
    assert np.mean(per_ray >= 2) > 0.01   # (second absorptions, which start inside the lattice, are in the sample)
    # (the first absorptions sit on the pencil's line, an atom in x and y: both tracers' roundings of it are merged)
    for a in range(3):
        L.assert_ks2(np.round(gpu[:, a], 9), np.round(host[:, a], 9), ("absorption position", a))


# -- 3. identity ------------------------------------------------------------------------------------------------------
def with_fields(scene, unit=True):
    """Every component of every non-root node of `scene` with a field: 1 x 1 x 1 of value 1, or (unit=False) a
    3 x 4 x 5 pattern on a box around the node's origin (points beyond it clamp)."""
    rng = np.random.default_rng(5)
    stack = list(scene.root.children)
    while stack:
        node = stack.pop()
        stack.extend(node.children)
        g = node.geometry
        if g is None or g.material is None or not g.material.components:
            continue
        if unit:
            grid = ConcentrationGrid(np.ones((1, 1, 1)), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
        else:
            grid = ConcentrationGrid(rng.uniform(0.0, 2.0, (3, 4, 5)), (-2.0, -1.5, -0.4), (2.5, 1.5, 0.4))
        for component in g.material.components:
            component.concentration = grid
    return scene


ID_SCENES = {"lsc": scenes.lsc_equivalent, "tiles6": scenes.tiles6, "mesh_lsc": scenes.mesh_lsc}


def _submit(session, rays, seed, **kw):
    pos, dirs, wl = rays
    return session.collect(session.submit(len(wl), seed, host_rays=(pos, dirs, wl, ["r"] * len(wl)), **kw))


@pytest.mark.parametrize("name", sorted(ID_SCENES))
def test_a_unit_field_traces_bit_for_bit_like_no_field(name):
    plain, unit = ID_SCENES[name](), with_fields(ID_SCENES[name]())
    assert compile_scene(unit).has_fields and not compile_scene(plain).has_fields
    pos, dirs, wl, _ = emit_bundle(plain, 100_000, seed=3)
    hist, tally = [], []
    for scene in (plain, unit):
        with Session(scene, emission="host") as s:
            h = _submit(s, (pos[:20_000], dirs[:20_000], wl[:20_000]), 7, record_every=1, max_events=64)
            hist.append({k: np.asarray(h.data[k]).copy() for k in HIST_KEYS})
            t = _submit(s, (pos, dirs, wl), 7, record_every=0)
            tally.append({k: np.asarray(t.data[k]).copy() for k in TALLY_KEYS})
    assert np.any(hist[0]["kind"] == ABSORB)
    for k in HIST_KEYS:
        assert np.array_equal(hist[0][k], hist[1][k]), (name, k)
    for k in TALLY_KEYS:
        assert np.array_equal(tally[0][k], tally[1][k]), (name, k)


def test_a_unit_field_with_device_emission_and_carried_launches():
    plain, unit = scenes.lsc_equivalent(), with_fields(scenes.lsc_equivalent())
    out = []
    for scene in (plain, unit):
        with Session(scene, emission="device") as s:
            r = s.collect(s.submit(300_000, 13, record_every=0, emit_seed=21))
            out.append({k: np.asarray(r.data[k]).copy() for k in TALLY_KEYS})
    for k in TALLY_KEYS:
        assert np.array_equal(out[0][k], out[1][k]), k
    carried = [_carried(scene, 200_003, 29) for scene in (plain, unit)]
    assert np.array_equal(carried[0][0], carried[1][0]) and np.array_equal(carried[0][1], carried[1][1])


def _carried(scene, n, seed):
    """(totals of one launch, totals of the same rays in carried launches)."""
    compiled = compile_scene(scene)
    pos, dirs, wl, _ = emit_bundle(scenes.lsc_equivalent(), n, seed=30)
    dscene = native.DeviceScene(compiled, device=0)
    try:
        dev = torch.device("cuda", 0)
        rays = tuple(torch.from_numpy(a).to(dev) for a in (pos, dirs, wl))
        whole = dscene.new_tallies()
        dscene.trace(rays, n, seed, whole)
        parts = dscene.new_tallies()
        edges = [0, 70_000, 70_064, 150_000, n]
        for a, b in zip(edges[:-1], edges[1:]):
            dscene.trace(tuple(t[a:b] for t in rays), b - a, seed, parts, ray_offset=a, carry_out=True)
        dscene.trace(None, 0, 0, parts)
        torch.cuda.synchronize()
        return whole.ints.cpu().numpy(), parts.ints.cpu().numpy()
    finally:
        dscene.close()


# -- 4. determinism ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ID_SCENES))
def test_ray_histories_do_not_depend_on_the_launch(name):
    scene = with_fields(ID_SCENES[name](), unit=False)
    assert compile_scene(scene).has_fields
    n, every, seed, me = 1_000_000, 15_625, 23, 48
    pos, dirs, wl, _ = emit_bundle(scene, n, seed=24)
    with Session(scene, emission="host") as s:
        big = _submit(s, (pos, dirs, wl), seed, record_every=every, max_events=me, emit_method="kT")
        data = {k: np.asarray(big.data[k]) for k in HIST_KEYS}
        assert np.any(data["kind"] == ABSORB)
        for j in range(0, n // every, 4):   # the same ray alone, in a launch of one: traced in the tail
            i = j * every
            one = _submit(s, (pos[i:i + 1], dirs[i:i + 1], wl[i:i + 1]), seed, record_every=1, max_events=me,
                          emit_method="kT", ray_offset=i)
            k = int(data["counts"][j])
            assert int(one.data["counts"][0]) == k, (name, i)
            for key in HIST_KEYS[1:]:
                assert np.array_equal(np.asarray(one.data[key])[:k], data[key][j * me:j * me + k]), (name, i, key)
        m = 8192
        hist = _submit(s, (pos[:m], dirs[:m], wl[:m]), seed, record_every=1, max_events=512, maxsteps=200,
                       emit_method="kT")
        tally = _submit(s, (pos[:m], dirs[:m], wl[:m]), seed, record_every=0, maxsteps=200, emit_method="kT")
        for key in TALLY_KEYS:
            assert np.array_equal(np.asarray(hist.data[key]), np.asarray(tally.data[key])), (name, key)


def test_fields_change_the_tallies_and_carried_launches_equal_one_launch():
    plain, fielded = scenes.lsc_equivalent(), with_fields(scenes.lsc_equivalent(), unit=False)
    a, b = _carried(fielded, 200_003, 29)
    assert np.array_equal(a, b) and a.sum() > 0
    assert not np.array_equal(_carried(plain, 200_003, 29)[0], a)


# -- 5. refusals ------------------------------------------------------------------------------------------------------
def test_the_packer_refuses_each_malformed_table_with_its_own_message():
    compiled = compile_scene(BT.field_scene())
    lib = native.load_library()
    st, keep = native.scene_tables_struct(compiled)

    def attempt(**change):
        ft, held = BT.field_tables(**change)
        handle = C.c_void_p()
        rc = lib.pvt_scene_create_field(C.byref(st), None, None, None, C.byref(ft), 0, C.byref(handle))
        if rc == 0:
            lib.pvt_scene_destroy(handle)
            return None
        assert not handle.value
        return lib.pvt_last_error().decode()

    assert attempt() is None
    bad = BT.FIELD_BREAKS   # (the cases: tests/broken_tables.py)
    messages = {}
    for what, change in bad.items():
        msg = attempt(**change)
        assert msg is not None and "field tables" in msg, (what, msg)
        messages[what] = msg
    assert len(set(messages.values())) == len(messages), messages
    from pvtrace_amd.engine import _kernel
    from pvtrace_amd.engine.compiler import UnsupportedSceneError

    with pytest.raises(UnsupportedSceneError, match="concentration"):
        _kernel.trace_bundle(compiled, np.zeros((1, 3)), np.array([[0.0, 0.0, 1.0]]), np.array([555.0]), 0, 10, 4, 0, 1, 1)
