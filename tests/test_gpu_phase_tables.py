"""Tabulated phase functions (PhaseFunctionTable) on the GPU.  The CPU referee does not know the tables, so the engine
is held to laws computed here from each table's own (angle, values) (tests/laws.py statistics, 1e6 photons per law),
to the host Python tracer in distribution, and to itself: a ray's history does not depend on the launch, the mode or
the kernel variant that traces it."""
import math

import numpy as np
import pytest
import torch

from pvtrace_amd import Luminophore, PhaseFunctionTable, Ray, Scatterer
from pvtrace_amd.algorithm import photon_tracer
from pvtrace_amd.engine import Session, compile_scene, native
from pvtrace_amd.engine.emit import emit_bundle
from pvtrace_amd.material import ray_basis
from tests import laws as L
from tests import scenes
from tests.law_cases import EMS_X, EMS_Y, medium_scene, rows
from tests.test_gpu_laws import Gpu

pytestmark = pytest.mark.gpu

B = Gpu()
ABSORB, SCATTER, EMIT = 3, 5, 6
OBLIQUE = tuple(np.array([0.48, -0.6, 0.64]) / np.linalg.norm([0.48, -0.6, 0.64]))


def hg_table(g, n=1801):
    angle = np.linspace(0.0, 180.0, n)
    mu = np.cos(np.radians(angle))
    return PhaseFunctionTable(angle, (1.0 - g * g) / (1.0 + g * g - 2.0 * g * mu) ** 1.5)


def rayleigh():
    angle = np.linspace(0.0, 180.0, 91)
    return PhaseFunctionTable(angle, 1.0 + np.cos(np.radians(angle)) ** 2)


TABLES = {
    "constant": lambda: PhaseFunctionTable([0.0, 180.0], [1.0, 1.0]),
    "rayleigh": rayleigh,
    "hg0.9-1801": lambda: hg_table(0.9),
    "zero-mass": lambda: PhaseFunctionTable([0.0, 30.0, 60.0, 100.0, 140.0, 180.0], [1.0, 0.0, 0.0, 0.0, 2.0, 2.0]),
}


def segment_masses(angle, values):
    """(mu axis ascending, probability of each mu segment): the trapezoid rule in mu from (angle, values) alone."""
    mu = np.cos(np.radians(np.asarray(angle, float)))[::-1]
    mu[0], mu[-1] = -1.0, 1.0
    p = np.asarray(values, float)[::-1]
    m = 0.5 * (p[1:] + p[:-1]) * np.diff(mu)
    return mu, m / m.sum()


def assert_mu_law(table, mu, what, values=None):
    axis, masses = segment_masses(table.angle, table.values if values is None else values)
    seg = np.clip(np.searchsorted(axis, mu, side="right") - 1, 0, axis.size - 2)
    if axis.size > 2:
        L.assert_chi2(np.bincount(seg, minlength=axis.size - 1), masses, what)
    else:   # one segment: mu uniform on [-1, 1]
        L.assert_ks(mu, L.uniform_cdf(-1.0, 1.0), what)
    # the contract inverts a CDF linear in mu within a segment: the table's own mean is that of uniform segments
    L.assert_mean(mu, float(np.sum(masses * 0.5 * (axis[1:] + axis[:-1]))), what)
    assert np.all(masses[seg] > 0.0), (what, "a zero-mass segment was sampled")


def assert_azimuth_uniform(d, d_in, what):
    e1, e2 = ray_basis(np.asarray(d_in, float))
    L.assert_ks(np.arctan2(d @ e2, d @ e1), L.uniform_cdf(-math.pi, math.pi), (what, "azimuth about d_in"))


def first_scatter(table, direction, wavelength=555.0, n=None, seed=15):
    n = B.n_hist if n is None else n
    scene = medium_scene(Scatterer(1.0, quantum_yield=1.0, phase_function=table))
    data, _ = B.trace_pencil(scene, (0.0, 0.0, 0.0), direction, wavelength, n, seed=seed, record_every=1, max_events=3)
    row, have = rows(data, 2, 3)
    assert have.all() and np.all(row["kind"] == SCATTER)
    return row["direction"]


# -- 7. the mu law at a scatter event, about the incoming direction ---------------------------------------------------
@pytest.mark.parametrize("direction", ["x", "oblique"])
@pytest.mark.parametrize("key", sorted(TABLES))
def test_mu_law_about_the_incoming_direction(key, direction):
    table = TABLES[key]()
    d_in = (1.0, 0.0, 0.0) if direction == "x" else OBLIQUE
    d = first_scatter(table, d_in)
    assert np.allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-12)
    mu = d @ np.asarray(d_in)
    assert_mu_law(table, mu, (key, direction))
    assert_azimuth_uniform(d, d_in, (key, direction))


# -- 8. wavelength rows ---------------------------------------------------------------------------------------------
def test_rows_mix_linearly_in_wavelength_and_clamp_at_the_ends():
    fwd, back = [1.0, 1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0, 1.0]   # the sign of mu tells the row
    table = PhaseFunctionTable([0.0, 45.0, 90.0, 135.0, 180.0], [fwd, back], wavelength=[500.0, 600.0])
    n = B.n_hist
    mu = first_scatter(table, (1.0, 0.0, 0.0), wavelength=530.0)[:, 0]
    L.assert_binomial(int((mu < 0.0).sum()), n, 0.3, "row mixture at 530 nm")
    for wl, back_row in ((420.0, False), (500.0, False), (600.0, True), (900.0, True)):
        mu = first_scatter(table, (1.0, 0.0, 0.0), wavelength=wl, n=100_000, seed=16)[:, 0]
        assert np.all((mu < 0.0) == back_row), wl


# -- 9. luminophore re-emission -------------------------------------------------------------------------------------
def test_luminophore_reemits_about_the_absorbed_direction_and_keeps_its_spectrum():
    table = rayleigh()
    dye = Luminophore(5.0, emission=np.column_stack((EMS_X, EMS_Y)), quantum_yield=1.0, phase_function=table, name="dye")
    data, compiled = B.trace_pencil(medium_scene(dye), (0.0, 0.0, 0.0), OBLIQUE, 560.0, B.n_hist, seed=17,
                                    record_every=1, max_events=3, emit_method=2)
    absorb, _ = rows(data, 1, 3)
    after, have = rows(data, 2, 3)
    assert have.all() and np.all(absorb["kind"] == ABSORB) and np.all(after["kind"] == EMIT)
    d = after["direction"]
    assert_mu_law(table, d @ np.asarray(OBLIQUE), "re-emission mu")
    assert_azimuth_uniform(d, OBLIQUE, "re-emission")
    # the wavelength draw follows the phase draws and keeps its law ('full': the whole compiled emission CDF)
    x, cdf = np.asarray(compiled.ems_x), np.asarray(compiled.ems_cdf)
    edges = np.arange(402.5, 800.0, 5.0)
    counts = np.bincount(np.searchsorted(edges, after["wavelength"], side="right"), minlength=edges.size + 1)
    L.assert_chi2(counts, L.bin_probabilities(L.emission_cdf(x, cdf, None), edges), "re-emission wavelength")


# -- 10. host Python tracer == engine, in distribution ----------------------------------------------------------------
def test_host_tracer_and_engine_agree_in_distribution():
    table = hg_table(0.6, 181)
    scene = medium_scene(Scatterer(1.0, quantum_yield=1.0, phase_function=table))
    np.random.seed(18)
    host = []
    for _ in range(4000):
        history = photon_tracer.follow(scene, Ray((0.0, 0.0, 0.0), OBLIQUE, 555.0), maxsteps=2, backend="host")
        host.append([r for r, e in history if e.name == "SCATTER"][0].direction)
    gpu = first_scatter(table, OBLIQUE, n=200_000, seed=19)
    L.assert_ks2(np.asarray(host) @ np.asarray(OBLIQUE), gpu @ np.asarray(OBLIQUE), "mu host vs GPU")


# -- 11. per-ray determinism across launches, modes and kernel variants ----------------------------------------------
TABLE_2ROW = PhaseFunctionTable(np.linspace(0.0, 180.0, 37), np.vstack([
    1.0 + 0.8 * np.cos(np.radians(np.linspace(0.0, 180.0, 37))),
    1.0 - 0.5 * np.cos(np.radians(np.linspace(0.0, 180.0, 37)))]), wavelength=[500.0, 700.0])


def with_tables(scene):
    """Every scattering component of `scene` draws from TABLE_2ROW, and every non-root material gets a table
    scatterer too (shared materials once)."""
    seen = set()
    for node in scene.root.preorder():
        g = node.geometry
        if g is None or node is scene.root or id(g.material) in seen:
            continue
        seen.add(id(g.material))
        for c in g.material.components:
            if type(c) in (Scatterer, Luminophore):
                c.phase_function = TABLE_2ROW
        g.material.components.append(Scatterer(0.4, quantum_yield=0.95, phase_function=TABLE_2ROW, name="mist"))
    return scene


DET_SCENES = {"lsc": scenes.lsc_equivalent, "tiles6": scenes.tiles6, "mesh_lsc": scenes.mesh_lsc}
HIST_KEYS = ("counts", "kind", "position", "direction", "wavelength", "duration")
TALLY_KEYS = ("rec_distinct", "rec_crossings", "rec_bins")


def _submit(session, rays, seed, **kw):
    pos, dirs, wl = rays
    return session.collect(session.submit(len(wl), seed, host_rays=(pos, dirs, wl, ["r"] * len(wl)), **kw))


@pytest.mark.parametrize("name", sorted(DET_SCENES))
def test_ray_histories_do_not_depend_on_the_launch(name):
    scene = with_tables(DET_SCENES[name]())
    n, every, seed, me = 1_000_000, 15_625, 23, 48
    pos, dirs, wl, _ = emit_bundle(scene, n, seed=24)
    assert compile_scene(scene).n_phase_tables == 1
    with Session(scene, emission="host") as s:
        big = _submit(s, (pos, dirs, wl), seed, record_every=every, max_events=me, emit_method="kT")
        data = {k: np.asarray(big.data[k]) for k in HIST_KEYS}
        assert data["counts"].size == n // every
        assert np.any(data["kind"] == SCATTER), "the tables were never sampled"
        for j in range(0, n // every, 4):   # the same ray alone, in a launch of one: traced in the tail
            i = j * every
            one = _submit(s, (pos[i:i + 1], dirs[i:i + 1], wl[i:i + 1]), seed, record_every=1, max_events=me,
                          emit_method="kT", ray_offset=i)
            k = int(data["counts"][j])
            assert int(one.data["counts"][0]) == k, (name, i)
            for key in HIST_KEYS[1:]:
                assert np.array_equal(np.asarray(one.data[key])[:k], data[key][j * me:j * me + k]), (name, i, key)
        # tally mode and history mode count the same photons (a log long enough for every event of 200 steps: a
        # history launch ends a photon whose log is full)
        m = 8192
        hist = _submit(s, (pos[:m], dirs[:m], wl[:m]), seed, record_every=1, max_events=512, maxsteps=200,
                       emit_method="kT")
        tally = _submit(s, (pos[:m], dirs[:m], wl[:m]), seed, record_every=0, maxsteps=200, emit_method="kT")
        for key in TALLY_KEYS:
            assert np.array_equal(np.asarray(hist.data[key]), np.asarray(tally.data[key])), (name, key)


def test_carried_launches_give_the_totals_of_one_launch():
    scene = with_tables(scenes.lsc_equivalent())
    compiled = compile_scene(scene)
    n, seed = 200_003, 29
    pos, dirs, wl, _ = emit_bundle(scene, n, seed=30)
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
        ints_a, ints_b = whole.ints.cpu().numpy(), parts.ints.cpu().numpy()
        assert np.array_equal(ints_a, ints_b)
        assert ints_a.sum() > 0
    finally:
        dscene.close()


# -- 12. large tables: out of LDS, same law -------------------------------------------------------------------------
def test_a_table_too_large_for_lds_keeps_the_law():
    angle = np.linspace(0.0, 180.0, 1801)
    wls = np.linspace(400.0, 800.0, 20)
    g = np.linspace(0.2, 0.9, 20)[:, None]
    mu = np.cos(np.radians(angle))[None, :]
    values = (1.0 - g * g) / (1.0 + g * g - 2.0 * g * mu) ** 1.5
    table = PhaseFunctionTable(angle, values, wavelength=wls)
    assert 8 * table.cdf.size > 160 * 1024   # (more than a workgroup's LDS)
    d = first_scatter(table, OBLIQUE, wavelength=wls[7])   # exactly on a row: that row alone
    assert_mu_law(table, d @ np.asarray(OBLIQUE), "large table, row 7", values=values[7])
    assert_azimuth_uniform(d, OBLIQUE, "large table")
