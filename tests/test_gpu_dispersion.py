"""Refractive-index tables n(wavelength) on the GPU, by properties that need no referee (the GPU against the C referee
on dispersive scenes is tests/test_gpu_table_parity.py): a table holding a constant must give, bit for bit, what the
scalar index gives (same draws, same events, same clocks); hand-traced rays through a strongly dispersive block refract, reflect totally and keep time with n at
their own wavelength; the reference's own Python tracer, with the dispersion written as a delegate the reference lets
users write, pins the outcome fractions and event counts of a dispersive Lumogen slab
(tests/golden/dispersion_tracer.npz); and pvt_scene_create_ex rejects every malformed table with its own message."""
import ctypes as C
import math

import numpy as np
import pytest

from pvtrace_amd import Box, Light, Luminophore, Material, Node, RefractiveIndexTable, Scene, Surface, rectangular_mask
from pvtrace_amd.data import lumogen_f_red_305
from pvtrace_amd.engine import Recorder, Session, UnsupportedSceneError, _kernel, compile_scene
from pvtrace_amd.engine.emit import emit_bundle
from pvtrace_amd.material import fresnel_reflectivity, fresnel_refraction
from tests import broken_tables as BT
from tests import dispersion_scene as D
from tests import scenes
from tests.util import assert_bundles_identical, load_golden

pytestmark = pytest.mark.gpu

SPEED_OF_LIGHT_CM_PER_S = 2.99792458e10


def with_index_tables(scene, points=1):
    """The same scene with every node's scalar index replaced by a table holding that constant: one point, or
    `points` points flat over 300-1000 nm."""
    for node in scene.root.preorder():
        g = node.geometry
        if g is None or isinstance(g.material.refractive_index, RefractiveIndexTable):
            continue   # (materials shared by several nodes are replaced once)
        n = float(g.material.refractive_index)
        wl = [555.0] if points == 1 else np.linspace(300.0, 1000.0, points)
        g.material.refractive_index = RefractiveIndexTable(wl, np.full(len(wl), n))
    return scene


def trace(scene, rays, seed, record_every, emit_method="kT", max_events=64, maxsteps=1000, packed_log=False):
    """One bundle of given rays through the resident-scene entry (pvt_scene_create_ex) -> EngineResult."""
    pos, dirs, wl = rays
    with Session(scene, emission="host") as session:
        pending = session.submit(len(wl), seed, maxsteps=maxsteps, max_events=max_events, emit_method=emit_method,
                                 record_every=record_every, host_rays=(pos, dirs, wl, ["rays"] * len(wl)),
                                 packed_log=packed_log)
        return session.collect(pending)


def columns(result):
    return {k: np.asarray(result.data[k]) for k in result.data}


EQUIVALENCE_SCENES = {
    "lsc_equivalent": scenes.lsc_equivalent,   # a Lumogen F Red slab
    "hello_world": scenes.hello_world,
    "nested_cylinders": scenes.nested_cylinders,
    "tiles6": scenes.tiles6,                   # 37 nodes: the node-grid kernels
    "coated_slab": scenes.coated_slab,
    "mesh_lsc": scenes.mesh_lsc,
}
# (record_every, emit_method, rays): record and tally launches, the three emission models, a tail-sized bundle
MODES = [(1, "kT", 3000), (0, "redshift", 40000), (3, "full", 6000), (1, "kT", 700)]


@pytest.mark.parametrize("points", [1, 4])
@pytest.mark.parametrize("mode", MODES, ids=lambda m: f"rec{m[0]}-{m[1]}-{m[2]}")
@pytest.mark.parametrize("name", sorted(EQUIVALENCE_SCENES))
def test_constant_table_is_bit_identical_to_the_scalar_index(name, mode, points):
    record_every, emit_method, n = mode
    scalar = EQUIVALENCE_SCENES[name]()
    pos, dirs, wl, _ = emit_bundle(scalar, n, seed=5)
    tabled = with_index_tables(EQUIVALENCE_SCENES[name](), points)
    assert compile_scene(scalar).n_ri_tables == 0 and compile_scene(tabled).n_ri_tables > 0
    want = trace(scalar, (pos, dirs, wl), 17, record_every, emit_method)
    got = trace(tabled, (pos, dirs, wl), 17, record_every, emit_method)
    assert_bundles_identical(columns(got), columns(want), sums_rtol=1e-12, what=(name, mode, points))


@pytest.mark.parametrize("tables", ["global", "heads"])
def test_constant_table_in_global_memory_is_bit_identical(tables, monkeypatch):
    monkeypatch.setenv("PVT_TABLES", tables)
    for name in ("lsc_equivalent", "mesh_lsc"):
        scalar = EQUIVALENCE_SCENES[name]()
        pos, dirs, wl, _ = emit_bundle(scalar, 4000, seed=6)
        want = trace(scalar, (pos, dirs, wl), 23, 1)
        got = trace(with_index_tables(EQUIVALENCE_SCENES[name](), 4), (pos, dirs, wl), 23, 1)
        assert_bundles_identical(columns(got), columns(want), sums_rtol=1e-12, what=(name, tables))


def test_constant_table_through_device_emission_and_a_device_list():
    from pvtrace_amd import engine

    for emit_method in ("kT", "full"):
        a = engine.simulate(scenes.lsc_equivalent(), 100000, seed=9, emit_seed=10, record_every=0, emit_method=emit_method)
        b = engine.simulate(with_index_tables(scenes.lsc_equivalent(), 3), 100000, seed=9, emit_seed=10, record_every=0,
                            emit_method=emit_method)
        assert_bundles_identical(b.data, a.data, sums_rtol=1e-12, what=emit_method)
    a = engine.simulate(scenes.hello_world(), 4000, seed=3, emit_seed=4, record_every=1, devices=[0, 0])
    b = engine.simulate(with_index_tables(scenes.hello_world()), 4000, seed=3, emit_seed=4, record_every=1, devices=[0, 0])
    assert_bundles_identical(columns(b), columns(a), sums_rtol=1e-12)


def test_the_kernel_reads_the_table_not_the_scalar_column():
    """Negative control: 1.5 at 300 nm rising to 1.6 at 1000 nm.  The flattener's scalar column holds 1.5, the first
    value, so a kernel that read the column would reproduce the scalar scene."""
    scalar = scenes.lsc_equivalent()
    pos, dirs, wl, _ = emit_bundle(scalar, 3000, seed=5)
    rising = scenes.lsc_equivalent()
    for node in rising.root.preorder():
        if node.geometry is not None and node is not rising.root:
            node.geometry.material.refractive_index = RefractiveIndexTable([300.0, 1000.0], [1.5, 1.6])
    c = compile_scene(rising)
    assert c.n_ri_tables == 1 and np.all(c.refractive_index[c.ri_table >= 0] == 1.5)
    want = columns(trace(scalar, (pos, dirs, wl), 17, 1))
    got = columns(trace(rising, (pos, dirs, wl), 17, 1))
    assert not np.array_equal(got["direction"], want["direction"]) or not np.array_equal(got["counts"], want["counts"])
    assert not np.array_equal(got["duration"], want["duration"])


# -- hand-traced rays through a strongly dispersive clear block ---------------------------------------------------------
TABLE = RefractiveIndexTable(D.BLOCK_WAVELENGTH, D.BLOCK_VALUE)
# both clamped ends, the grid points and mid-cell
FIVE_WAVELENGTHS = (350.0, 400.0, 500.0, 600.0, 950.0)


def rays_from(points, direction, wavelengths, copies):
    wl = np.repeat(np.asarray(wavelengths, dtype=float), copies)
    return (np.tile(points, (len(wl), 1)).astype(float), np.tile(direction, (len(wl), 1)).astype(float), wl)


def test_first_refraction_follows_snell_at_the_photons_wavelength():
    t = math.radians(30.0)
    d = np.array([math.sin(t), 0.0, -math.cos(t)])
    start = np.array([0.0, 0.0, 0.5]) - 2.0 * d   # meets the top face at its centre
    result = trace(D.block_scene(TABLE), rays_from(start, d, FIVE_WAVELENGTHS, 20), 7, 1, maxsteps=20, max_events=128)
    data = result.data
    checked = set()
    for j in range(result.num_recorded):
        rows = result.rows_of(j)
        kinds = np.asarray(data["kind"][rows])
        if kinds[1] != 2:   # (the few that reflect off the top face)
            continue
        wl = float(data["wavelength"][rows][1])
        want = fresnel_refraction(d, (0.0, 0.0, -1.0), 1.0, TABLE.at(wl))
        assert np.allclose(np.asarray(data["direction"][rows][1]), want, rtol=0, atol=1e-12), wl
        checked.add(wl)
    assert checked == set(FIVE_WAVELENGTHS)


def test_clock_inside_the_block_runs_at_the_phase_index():
    d = np.array([0.0, 0.0, -1.0])   # normal incidence: straight through, TRANSMIT at the top and at the bottom
    result = trace(D.block_scene(TABLE), rays_from([0.1, 0.2, 2.0], d, FIVE_WAVELENGTHS, 20), 8, 1, maxsteps=20, max_events=128)
    data = result.data
    checked = set()
    for j in range(result.num_recorded):
        rows = result.rows_of(j)
        kinds = np.asarray(data["kind"][rows])
        if list(kinds[:4]) != [0, 2, 2, 7]:
            continue
        dur = np.asarray(data["duration"][rows])
        wl = float(data["wavelength"][rows][1])
        want = D.BLOCK[2] * TABLE.at(wl) / SPEED_OF_LIGHT_CM_PER_S
        assert abs((dur[2] - dur[1]) - want) <= 1e-12 * want, wl
        checked.add(wl)
    assert checked == set(FIVE_WAVELENGTHS)


def test_total_internal_reflection_at_one_wavelength_only():
    """From inside, at 40 degrees: beyond the critical angle at 800 nm (n = 1.70, 36.0 degrees), inside it at 400 nm
    (n = 1.40, 45.6 degrees), where the photon leaves with probability 1 - R."""
    t = math.radians(40.0)
    d = np.array([math.sin(t), 0.0, math.cos(t)])
    n = 20000
    result = trace(D.block_scene(TABLE), rays_from([0.0, 0.0, 0.0], d, (800.0, 400.0), n), 9, 1, maxsteps=4,
                   max_events=32, packed_log=True)
    data = result.data
    first = np.array([int(data["kind"][result.rows_of(j)][1]) for j in range(result.num_recorded)])
    red, blue = first[:n], first[n:]
    assert np.all(red == 1)                                            # every photon reflects
    r = fresnel_reflectivity(math.acos(math.cos(t)), 1.40, 1.0)
    share = np.mean(blue == 2)
    sigma = math.sqrt(r * (1 - r) / n)
    assert np.all((blue == 1) | (blue == 2))
    assert abs(share - (1 - r)) < 4 * sigma, (share, 1 - r, sigma)


# -- anchored to the reference's Python tracer -----------------------------------------------------------------------
def gpu_outcomes(index, n=12000, seed=31):
    """Per-ray outcome classes and event counts of the Lumogen slab at `index` (engine.simulate, device emission)."""
    from pvtrace_amd import engine
    from pvtrace_amd.light import ConstantWavelengthMask

    scene, _ = D.build(Node, Scene, Box, Material, Surface, Light, rectangular_mask, ConstantWavelengthMask(D.PUMP_NM),
                       D.components(Luminophore, lumogen_f_red_305), index=index)
    r = engine.simulate(scene, n, seed=seed, emit_seed=seed + 1, record_every=1, max_events=2100, packed_log=True)
    kind, position = np.asarray(r.data["kind"]), np.asarray(r.data["position"]).reshape(-1, 3)
    last = np.zeros(n, dtype=np.int64)
    where = np.zeros((n, 3))
    counts = np.zeros((n, 10))
    for j in range(n):
        rows = r.rows_of(j)
        k = kind[rows]
        counts[j] = np.bincount(k, minlength=10)
        last[j] = k[-1]
        where[j] = position[rows][-2] if k[-1] == 7 else position[rows][-1]
    return D.outcome_class(last, where), counts


def welch(a, b):
    """|mean(a) - mean(b)| in standard errors (Welch)."""
    se = np.sqrt(a.var(axis=0, ddof=1) / len(a) + b.var(axis=0, ddof=1) / len(b))
    diff = np.abs(a.mean(axis=0) - b.mean(axis=0))
    return np.where(se > 0, diff / np.where(se > 0, se, 1.0), np.where(diff > 0, np.inf, 0.0))


def test_dispersive_slab_against_the_references_python_tracer():
    g = load_golden("dispersion_tracer.npz")
    outcome, counts = gpu_outcomes(RefractiveIndexTable(D.DISP_WAVELENGTH, D.DISP_VALUE))
    one_hot = np.eye(5)[outcome][:, :4]    # exit-facet shares: top, bottom, edge, lost
    ref = {k: (np.eye(5)[g[f"{k}/outcome"].astype(int)][:, :4], g[f"{k}/event_counts"].astype(float))
           for k in ("dispersive", "scalar")}
    z_share = welch(one_hot, ref["dispersive"][0])
    assert np.all(z_share < 5.0), dict(zip(D.CLASSES, z_share))
    z_events = welch(counts, ref["dispersive"][1])
    assert np.all(z_events < 5.0), z_events
    # power: the dispersive GPU run is far from the reference's scalar run
    z_power = np.concatenate([welch(one_hot, ref["scalar"][0]), welch(counts, ref["scalar"][1])])
    assert z_power.max() > 5.0, z_power


# -- validation ------------------------------------------------------------------------------------------------------
def _create_ex(compiled, edit):
    from pvtrace_amd.engine import native as N

    lib = N.load_library()
    st, keep = N.scene_tables_struct(compiled)
    xt, arrays = BT.index_tables(compiled, edit)
    handle = C.c_void_p()
    rc = lib.pvt_scene_create_ex(C.byref(st), C.byref(xt), 0, C.byref(handle))
    if rc == 0:
        lib.pvt_scene_destroy(handle)
    return rc, lib.pvt_last_error().decode()


_set, BREAKS = BT.index_edit, BT.INDEX_BREAKS   # (the cases: tests/broken_tables.py)


@pytest.mark.parametrize("case", sorted(BREAKS))
def test_create_ex_rejects_each_broken_field(case):
    compiled = compile_scene(D.block_scene(TABLE))
    assert _create_ex(compiled, _set())[0] == 0
    edit, message = BREAKS[case]
    rc, err = _create_ex(compiled, edit)
    assert rc == -1 and message in err, (case, rc, err)


def test_host_buffer_entry_refuses_a_dispersive_scene_and_traces_a_scalar_one():
    compiled = compile_scene(D.block_scene(TABLE))
    rays = (np.zeros((4, 3)), np.tile([0.0, 0.0, -1.0], (4, 1)), np.full(4, 500.0))
    with pytest.raises(UnsupportedSceneError, match="engine.simulate"):
        _kernel.trace_bundle(compiled, *rays, 1, 100, 16, 0, 1, 1)
    out = _kernel.trace_bundle(compile_scene(D.block_scene(1.5)), *rays, 1, 100, 16, 0, 1, 1)
    assert out["counts"].shape == (4,)
