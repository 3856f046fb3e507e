"""Scenes with refractive-index tables n(wavelength) and coating reflectivity tables R(wavelength, angle) on the GPU,
held bit for bit to the CPU referee (oracle/pvt_oracle.c), which evaluates both kinds of table itself.

Bar of tests/test_gpu_parity.py: integer columns and tallies exact, floating-point columns bit-exact, recorder moment
sums to 1e-12 relative.  Dispersive scenes go through `Session(scene, emission="host")` with host rays (the resident
scene, pvt_scene_create_ex); the referee's own table semantics are pinned to the reference's Python tracer by
tests/test_oracle_tables.py and to exact arithmetic by tests/test_table_lookup_exact.py.

The cases are built so that every lookup path of the kernel runs (CASES: what each is meant to reach, asserted from
the compiled scene: node and recorder counts, meshes, the node grid, table sizes): the out-of-line index lookup of
the 2-node and mesh kernels, the inlined one of the wide-mask and grid kernels, the hoisted tail step (a bundle of a
few hundred rays), the coating lookup inlined and called, tables in LDS, in global memory and split between them.
Then the shortcut switches, a carried stream of launches, device emission, fuzz, and physics checks of the GPU's own
histories that need no referee: Snell's law, the clock and the critical angle at n(lambda)."""
import math
import os

import numpy as np
import pytest

from oracle import oracle as O
from pvtrace_amd import (
    Box, CoatedSurfaceDelegate, Coating, Material, Node, ReflectivityTable, RefractiveIndexTable, Scene, Surface,
)
from pvtrace_amd.engine import Session, compile_scene, native
from pvtrace_amd.engine.emit import EmitterTables, emit_bundle
from tests import dispersion_scene as D
from tests import scenes
from tests.util import assert_bundles_identical

pytestmark = pytest.mark.gpu

EMIT = {0: "kT", 1: "redshift", 2: "full"}
TALLY_KEYS = ("rec_distinct", "rec_crossings", "rec_sums", "rec_bins")
C_CM_PER_S = 2.99792458e10


# -- tables ------------------------------------------------------------------------------------------------------------
BLOCK_TABLE = RefractiveIndexTable(D.BLOCK_WAVELENGTH, D.BLOCK_VALUE)           # 1.40 .. 1.70: TIR at some wavelengths
RISING = RefractiveIndexTable([300.0, 560.0, 620.0, 700.0, 1000.0], [1.38, 1.42, 1.62, 1.78, 1.80])   # steep over Lumogen
FALLING = RefractiveIndexTable([350.0, 450.0, 600.0, 900.0], [1.75, 1.60, 1.52, 1.47])
GLASS = RefractiveIndexTable(np.linspace(380.0, 820.0, 12), 1.5 + 6000.0 / np.linspace(380.0, 820.0, 12) ** 2)
AIR = RefractiveIndexTable([300.0, 1000.0], [1.0003, 1.0001])
R_FULL = ReflectivityTable([400.0, 480.0, 555.0, 640.0, 800.0],
                           [[0.9, 0.2, 0.6, 0.1, 0.8], [0.7, 0.3, 0.5, 0.2, 0.9], [0.4, 0.5, 0.3, 0.6, 0.2],
                            [0.1, 0.9, 0.2, 0.8, 0.4], [1.0, 1.0, 0.9, 0.95, 1.0]],
                           angle=[0.0, 20.0, 45.0, 70.0, 90.0])
R_NW1 = ReflectivityTable([555.0], [[0.8], [0.5], [0.05]], angle=[0.0, 40.0, 90.0])
R_NA1 = ReflectivityTable([420.0, 520.0, 610.0, 760.0], [0.05, 0.6, 0.15, 0.9])


def _wl_spread(n, seed, lo=350.0, hi=900.0):
    return np.random.default_rng(seed).uniform(lo, hi, n)


def _set_index(node, table):
    g = node.geometry
    g.material = Material(refractive_index=table, surface=g.material.surface, components=g.material.components)


def block_dispersive():
    return D.block_scene(BLOCK_TABLE)


def block_rays(n, seed):
    """Into the block from above at random angles and from inside it in random directions, 350-950 nm."""
    rng = np.random.default_rng(seed)
    half = n // 2
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    d[:half, 2] = -np.abs(d[:half, 2])
    d /= np.linalg.norm(d, axis=1)[:, None]
    pos = np.zeros((n, 3))
    pos[:half] = np.column_stack([rng.uniform(-1.5, 1.5, half), rng.uniform(-1.5, 1.5, half), np.full(half, 3.0)])
    pos[:half, :2] -= d[:half, :2] * (2.5 / -d[:half, 2:3])   # aimed at the top face
    pos[half:] = rng.uniform(-0.4, 0.4, (n - half, 3))
    return pos, d, rng.uniform(350.0, 950.0, n)


def lsc_rising():
    scene = scenes.lsc_equivalent()
    _set_index([c for c in scene.root.children if c.name == "LSC"][0], RISING)
    return scene


def nested_two_tables():
    scene = scenes.nested_cylinders()
    a = [c for c in scene.root.children if c.name == "A"][0]
    _set_index(a, GLASS)
    _set_index(a.children[0], FALLING)
    return scene


def nested_shared_table():
    """A and B index-matched through ONE table object (one index class), in air that is itself dispersive."""
    scene = scenes.nested_cylinders()
    _set_index(scene.root, AIR)
    a = [c for c in scene.root.children if c.name == "A"][0]
    _set_index(a, FALLING)
    _set_index(a.children[0], FALLING)
    return scene


def tiles_dispersive():
    scene = scenes.tiles6()
    tables = (GLASS, FALLING, RISING)
    for k, node in enumerate(n for n in scene.root.preorder() if n is not scene.root and n.geometry is not None):
        _set_index(node, tables[k % 3])
    return scene


def wide_mask_slab():
    from tests.test_gpu_parity import _scene_with_many_recorders

    scene = _scene_with_many_recorders(150)
    _set_index(scene.root.children[0], FALLING)
    return scene


def mesh_dispersive():
    scene = scenes.mesh_lsc()
    slab = [c for c in scene.root.children if c.name == "LSC"][0]
    g = slab.geometry
    g.material = Material(refractive_index=RISING, components=g.material.components,
                          surface=Surface(delegate=CoatedSurfaceDelegate([Coating((0, 0, -1), reflectivity=R_FULL)])))
    return scene


def _coatings():
    return [Coating((0, 0, 1), reflectivity=R_FULL, region=((0.0, None), (0.0, None), None)),     # specular, Fresnel
            Coating((0, 0, -1), reflectivity=R_NW1, reflection="lambertian"),
            Coating((1, 0, 0), reflectivity=R_NA1, transmission="matched"),
            Coating((-1, 0, 0), reflectivity=R_FULL, reflection="lambertian", transmission="matched"),
            Coating((0, 1, 0), reflectivity=R_NA1)]                                                 # keep_tir


def coated_rtables():
    scene = scenes.coated_slab()
    slab = [c for c in scene.root.children if c.geometry is not None][0]
    slab.geometry.material = Material(refractive_index=1.5, components=slab.geometry.material.components,
                                      surface=Surface(delegate=CoatedSurfaceDelegate(_coatings())))
    return scene


def coated_dispersive():
    scene = coated_rtables()
    _set_index([c for c in scene.root.children if c.geometry is not None][0], GLASS)
    return scene


def large_tables():
    """A 5000-point index table and an 8 x 4000 reflectivity table: more than LDS holds."""
    x = np.linspace(300.0, 1000.0, 5000)
    big_n = RefractiveIndexTable(x, 1.5 + 0.05 * np.sin(x / 23.0))
    wl_axis, ang_axis = np.linspace(300.0, 1000.0, 4000), np.linspace(0.0, 90.0, 8)
    big_r = ReflectivityTable(wl_axis, np.clip(0.5 + 0.45 * np.sin(wl_axis / 37.0)[None, :]
                                               * np.cos(np.radians(ang_axis))[:, None], 0.0, 1.0), angle=ang_axis)
    scene = scenes.lsc_equivalent()
    slab = [c for c in scene.root.children if c.name == "LSC"][0]
    slab.geometry.material = Material(refractive_index=big_n, components=slab.geometry.material.components,
                                      surface=Surface(delegate=CoatedSurfaceDelegate([Coating((0, 0, 1), reflectivity=big_r)])))
    return scene


def _n_nodes(c):
    return int(c.geom_type.shape[0])


def _n_rec(c):
    return int(c.rec_node.shape[0])


# name -> (builder, rays: None = the scene's lights, wavelengths spread: rays' wavelengths redrawn, what it reaches, check)
CASES = {
    "block_dispersive": (block_dispersive, block_rays, False,
                         "analytic 2 nodes, SEENW 1, out-of-line index_class_n_call, critical angle formed per hit",
                         lambda c: _n_nodes(c) == 2 and _n_rec(c) <= 64 and c.n_ri_tables == 1),
    "lsc_rising": (lsc_rising, None, False, "re-emission changes n mid-history; Lumogen emission with the clock",
                   lambda c: c.n_ri_tables == 1 and int(np.sum(c.comp_type == 2)) >= 1),
    "nested_two_tables": (nested_two_tables, None, True, "dispersive-dispersive interface, two classes",
                          lambda c: c.n_ri_tables == 2 and c.ri_table[1] != c.ri_table[2] >= 0),
    "nested_shared_table": (nested_shared_table, None, True, "index-matched pair pooled by identity into one table",
                            lambda c: c.n_ri_tables == 2 and c.ri_table[1] == c.ri_table[2] >= 0 and c.ri_table[0] >= 0),
    "tiles_dispersive": (tiles_dispersive, None, True, "node grid, 82 recorders -> SEENW 4, inlined index_table_n",
                         lambda c: _n_nodes(c) == 37 and _n_rec(c) == 82 and c.n_ri_tables == 3
                         and (native.node_grid_plan(c) is None) == bool(os.environ.get("PVT_NO_GRID"))),
    "wide_mask_slab": (wide_mask_slab, None, True, "2 nodes, 150 recorders: inlined lookup in the non-grid wide mask",
                       lambda c: _n_nodes(c) == 2 and _n_rec(c) == 150 and c.n_ri_tables == 1),
    "mesh_dispersive": (mesh_dispersive, None, False, "MESH kernels: out-of-line index lookup and coat_table_r_call",
                        lambda c: int(np.sum(c.geom_type == 3)) == 1 and c.n_ri_tables == 1 and c.n_coat_tables == 1),
    "coated_rtables": (coated_rtables, None, True, "UF_CTAB: nw, na > 1 / nw == 1 / na == 1, Lambertian and specular, "
                       "Fresnel and matched transmission, keep_tir", lambda c: c.n_coat_tables == 3 and c.n_ri_tables == 0),
    "coated_dispersive": (coated_dispersive, None, True, "UF_CTAB and UF_DISP on one node",
                          lambda c: c.n_coat_tables == 3 and c.n_ri_tables == 1),
    "large_tables": (large_tables, None, True, "tables too large for LDS: TAB_LDS 2 / 0",
                     lambda c: c.rtab_wavelength.size == 5000 and c.ctab_value.size == 32000),
}
# (record_every, max_events, maxsteps, emit_method, rays): test_gpu_parity.MODES, a tail-sized bundle (the hoisted
# tail step of a lone wave), a small maxsteps (the kill path)
MODES = {"rec1": (1, 64, 1000, 0, 3000), "tally": (0, 128, 50, 1, 3000), "rec7": (7, 16, 1000, 2, 3000),
         "tail": (1, 64, 1000, 0, 300), "kill": (1, 32, 4, 0, 2000)}


def rays_for(name, scene, n, seed):
    _, rays, spread, _, _ = CASES[name]
    if rays is not None:
        return rays(n, seed)
    pos, dirs, wl, _ = emit_bundle(scene, n, seed=seed)
    return pos, dirs, (_wl_spread(n, seed) if spread else wl)


def gpu_trace(scene, rays, seed, mode):
    record_every, max_events, maxsteps, emit_method = mode[:4]
    pos, dirs, wl = rays
    with Session(scene, emission="host") as session:
        pending = session.submit(len(wl), seed, maxsteps=maxsteps, max_events=max_events, emit_method=EMIT[emit_method],
                                 record_every=record_every, host_rays=(pos, dirs, wl, ["rays"] * len(wl)))
        return session.collect(pending)


def oracle_trace(compiled, rays, seed, mode):
    record_every, max_events, maxsteps, emit_method = mode[:4]
    return O.trace_bundle(compiled, *rays, seed, maxsteps, max_events, emit_method, 4, record_every,
                          math_mode=O.MATH_PORTABLE)


def assert_same(result, cpu, record_every, what):
    keys = list(cpu) if record_every > 0 else list(TALLY_KEYS)
    got = {k: np.asarray(result.data[k]) for k in keys}
    assert_bundles_identical(got, {k: cpu[k] for k in keys}, sums_rtol=1e-12, what=what)


def run_case(name, mode, seed=42):
    scene = CASES[name][0]()
    compiled = compile_scene(scene)
    assert CASES[name][4](compiled), (name, CASES[name][3])
    rays = rays_for(name, scene, mode[4], seed + 1)
    result = gpu_trace(scene, rays, seed, mode)
    cpu = oracle_trace(result.compiled, rays, seed, mode)
    assert_same(result, cpu, mode[0], (name, mode))
    return result, cpu


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", sorted(CASES))
def test_table_scene_is_bit_identical_to_the_oracle(name, mode):
    result, cpu = run_case(name, MODES[mode])
    if mode == "rec1":   # the histories are long enough to reach the surfaces many times
        assert int(np.sum(cpu["kind"] == 2)) > 100 and int(np.sum(cpu["kind"] == 1)) > 20, name
    if mode == "kill":
        assert int(np.sum(cpu["kind"] == 9)) > 0, name


@pytest.mark.parametrize("tables", ["global", "heads"])
@pytest.mark.parametrize("name", ["block_dispersive", "coated_dispersive", "mesh_dispersive"])
def test_tables_placed_in_global_memory(name, tables, monkeypatch):
    monkeypatch.setenv("PVT_TABLES", tables)
    run_case(name, MODES["rec1"])


@pytest.mark.parametrize("switch", ["PVT_NO_FUSED_EXIT", "PVT_NO_LAZY_ROOT", "PVT_NO_GRID"])
@pytest.mark.parametrize("name", ["block_dispersive", "tiles_dispersive"])
def test_shortcut_switches_off(name, switch, monkeypatch):
    monkeypatch.setenv(switch, "1")
    run_case(name, MODES["rec1"], seed=7)


def test_carried_launches_on_a_dispersive_scene():
    """A stream of launches that park their last photons for the next one (PVT_FLAG_CARRY_OUT): tallies equal the
    referee's exactly."""
    import torch

    scene = lsc_rising()
    compiled = compile_scene(scene)
    n, seed = 30_011, 77
    pos, dirs, wl, _ = emit_bundle(scene, n, seed=4)
    cpu = O.trace_bundle(compiled, pos, dirs, wl, seed, 1000, 16, 0, 4, 0, math_mode=O.MATH_PORTABLE)
    dscene = native.DeviceScene(compiled, device=0)
    try:
        dev = torch.device("cuda", 0)
        rays = tuple(torch.from_numpy(a).to(dev) for a in (pos, dirs, wl))
        tallies = dscene.new_tallies()
        edges = [0, 9000, 9000 + 64, 21_000, n]
        for a, b in zip(edges[:-1], edges[1:]):
            dscene.trace(tuple(t[a:b] for t in rays), b - a, seed, tallies, ray_offset=a, carry_out=True)
        torch.cuda.synchronize()
        assert dscene.carry_pending()
        dscene.trace(None, 0, 0, tallies)
        torch.cuda.synchronize()
        assert not dscene.carry_pending()
        got = tallies.host(0)
        assert np.array_equal(got["rec_distinct"], cpu["rec_distinct"])
        assert np.array_equal(got["rec_crossings"], cpu["rec_crossings"])
        assert np.array_equal(got["rec_bins"], cpu["rec_bins"])
        assert np.allclose(got["rec_sums"], cpu["rec_sums"], rtol=1e-12, atol=0.0)
        assert cpu["rec_distinct"].sum() > 0
    finally:
        dscene.close()


def test_device_emission_on_a_dispersive_scene():
    from pvtrace_amd import engine

    scene = lsc_rising()
    result = engine.simulate(scene, 6000, seed=3, emission="device", emit_seed=12, max_events=64)
    assert result.compiled.n_ri_tables == 1
    pos, dirs, wl = O.emit(EmitterTables(scene), 6000, emit_seed=12)
    cpu = O.trace_bundle(result.compiled, pos, dirs, wl, 3, 1000, 64, 0, 4, 1, math_mode=O.MATH_PORTABLE)
    assert_bundles_identical(result.data, cpu, sums_rtol=1e-12)


# -- fuzz ----------------------------------------------------------------------------------------------------------------
def _fuzz(scene, seed, n=1000):
    mode = [(1, 48, 300, 0), (3, 16, 40, 1), (0, 8, 300, 2)][seed % 3]
    pos, dirs, wl, _ = emit_bundle(scene, n, seed=seed)
    result = gpu_trace(scene, (pos, dirs, wl), 9 + seed, mode)
    cpu = oracle_trace(result.compiled, (pos, dirs, wl), 9 + seed, mode)
    assert_same(result, cpu, mode[0], f"fuzz scene {seed}")


@pytest.mark.parametrize("seed", range(100))
def test_random_scenes_with_tables_gpu_equals_oracle(seed):
    from tests.fuzz import random_scene

    _fuzz(random_scene(3000 + seed, extensions=True, tables=True), seed)


@pytest.mark.parametrize("seed", range(30))
def test_random_many_node_scenes_with_tables_gpu_equals_oracle(seed):
    from tests.fuzz import random_many_scene

    _fuzz(random_many_scene(300 + seed, tables=True), seed)


# -- physics of the GPU's own histories, without the referee ----------------------------------------------------------
def _index_of(compiled):
    tables = [RefractiveIndexTable(compiled.rtab_wavelength[s:s + k], compiled.rtab_value[s:s + k])
              for s, k in zip(compiled.rtab_start, compiled.rtab_n)]

    def n(node, wl):
        j = int(compiled.ri_table[node])
        return tables[j].at(wl) if j >= 0 else float(compiled.refractive_index[node])
    return n


@pytest.mark.parametrize("name", ["block_dispersive", "lsc_rising", "nested_two_tables", "nested_shared_table",
                                  "tiles_dispersive", "wide_mask_slab"])
def test_histories_obey_snell_the_clock_and_the_critical_angle(name):
    """Every Fresnel-refracted TRANSMIT is vector Snell from the incoming direction and the logged normal (atol 1e-12);
    every segment's clock increment is its path increment x n_container(lambda) / c (rtol 1e-12, plus the rounding of
    the two running sums it is read from); no TRANSMIT lies beyond asin(n2 / n1) (a 1e-12 rad band excluded).  n from
    RefractiveIndexTable.at at the logged wavelength, evaluated in long double."""
    scene = CASES[name][0]()
    rays = rays_for(name, scene, 3000, 5)
    result = gpu_trace(scene, rays, 11, (1, 64, 1000, 0))
    c = result.compiled
    n_of = _index_of(c)
    d = result.data
    m = 64
    kind, hit, cont, adj = (np.asarray(d[k]) for k in ("kind", "hit", "container", "adjacent"))
    direc, nrm = np.asarray(d["direction"]).reshape(-1, 3), np.asarray(d["normal"]).reshape(-1, 3)
    wl, trav, dur = (np.asarray(d[k]) for k in ("wavelength", "travelled", "duration"))
    counts = np.asarray(d["counts"])
    L = np.longdouble
    snell = clocks = 0
    for j in range(len(counts)):
        for row in range(j * m + 1, j * m + int(counts[j])):
            k = int(kind[row])
            if k in (1, 2, 3, 7) and trav[row] > trav[row - 1]:
                n_c = n_of(int(cont[row]), float(wl[row]))
                dt = L(trav[row]) - L(trav[row - 1])
                want = dt * L(n_c) / L(C_CM_PER_S)
                slack = 1e-12 * want + (np.spacing(dur[row]) + np.spacing(trav[row]) * n_c / C_CM_PER_S) * 2
                assert abs((L(dur[row]) - L(dur[row - 1])) - want) <= slack, (name, j, row)
                clocks += 1
            if k != 2 or int(c.surface_type[int(hit[row])]) != 0:
                continue
            n1, n2 = n_of(int(cont[row]), float(wl[row])), n_of(int(adj[row]), float(wl[row]))
            d_in = direc[row - 1].astype(L)
            nf = nrm[row].astype(L)
            if np.dot(nf, d_in) < 0:
                nf = -nf
            ci = min(np.dot(nf, d_in), L(1))
            theta = math.acos(float(ci))
            if n2 < n1:
                assert theta <= math.asin(n2 / n1) + 1e-12, (name, j, row, theta, n1, n2)
            r = L(n1) / L(n2)
            want = r * d_in + (np.sqrt(L(1) - r * r * (L(1) - ci * ci)) - r * ci) * nf
            assert np.allclose(direc[row].astype(L), want, rtol=0, atol=1e-12), (name, j, row)
            snell += 1
    assert snell > 100 and clocks > 300, (snell, clocks)
