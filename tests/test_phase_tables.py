"""Tabulated phase functions (PhaseFunctionTable) on the host: the constructor's validation, the sampler held to laws
computed here from (angle, values) alone, the Python tracer's frame (the incoming ray, not +z), the flattener's pools,
the C ABI of PvtPhaseTables, the refusals of the host-buffer entries, the spec reader and lights.  No GPU needed."""
import math
import os
import subprocess

import ctypes as C
import numpy as np
import pytest

from pvtrace_amd import Box, Light, Luminophore, Material, Node, PhaseFunctionTable, Ray, Scatterer, Scene, spec
from pvtrace_amd.algorithm import photon_tracer
from pvtrace_amd.engine import emit as E
from pvtrace_amd.engine.compiler import PHASE_TABLE, UnsupportedSceneError, compile_scene
from pvtrace_amd.material import HenyeyGreenstein, isotropic, ray_basis
from tests import laws as L
from tests.law_cases import medium_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pvtrace_hip.h")

ANGLE = np.array([0.0, 20.0, 45.0, 70.0, 90.0, 120.0, 150.0, 180.0])
VALUES = np.array([6.0, 4.0, 2.0, 1.0, 0.5, 0.5, 1.5, 3.0])


def segment_masses(angle, values):
    """Probability of each mu segment of the table, ascending mu: the trapezoid rule in mu = cos(theta), from the
    table's own (angle, values) -- written independently of the class."""
    mu = np.cos(np.radians(np.asarray(angle, float)))[::-1]
    mu[0], mu[-1] = -1.0, 1.0
    p = np.asarray(values, float)[::-1]
    m = 0.5 * (p[1:] + p[:-1]) * np.diff(mu)
    return mu, m / m.sum()


def mu_counts(mu_axis, mu):
    return np.bincount(np.clip(np.searchsorted(mu_axis, mu, side="right") - 1, 0, mu_axis.size - 2),
                       minlength=mu_axis.size - 1)


# -- 1. constructor -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("angle, values, wavelength", [
    ([1.0, 90.0, 180.0], [1.0, 1.0, 1.0], None),                 # does not start at 0
    ([0.0, 90.0, 179.0], [1.0, 1.0, 1.0], None),                 # does not end at 180
    ([0.0, 100.0, 90.0, 180.0], [1.0, 1.0, 1.0, 1.0], None),     # not increasing
    ([0.0, 90.0, 90.0, 180.0], [1.0, 1.0, 1.0, 1.0], None),      # repeated angle
    ([0.0], [1.0], None),                                        # one point
    ([0.0, 90.0, 180.0], [1.0, -0.1, 1.0], None),                # negative
    ([0.0, 90.0, 180.0], [1.0, np.nan, 1.0], None),              # not finite
    ([0.0, 90.0, 180.0], [1.0, np.inf, 1.0], None),
    ([0.0, 90.0, 180.0], [0.0, 0.0, 0.0], None),                 # zero row
    ([0.0, 90.0, 180.0], [[1.0, 1.0, 1.0], [0.0, 0.0, 0.0]], [400.0, 500.0]),   # one zero row
    ([0.0, 90.0, 180.0], [1.0, 1.0], None),                      # shape
    ([0.0, 90.0, 180.0], [[1.0, 1.0, 1.0]], None),               # 2-D without wavelengths
    ([0.0, 90.0, 180.0], [1.0, 1.0, 1.0], [500.0]),              # 1-D with wavelengths
    ([0.0, 90.0, 180.0], [[1.0, 1.0, 1.0]] * 2, [500.0]),        # rows != wavelengths
    ([0.0, 90.0, 180.0], [[1.0, 1.0, 1.0]] * 2, [500.0, 400.0]),  # wavelengths not increasing
    ([0.0, 90.0, 180.0], [[1.0, 1.0, 1.0]] * 2, [500.0, np.nan]),
])
def test_constructor_rejects(angle, values, wavelength):
    with pytest.raises(ValueError):
        PhaseFunctionTable(angle, values, wavelength=wavelength)


def test_axis_and_cdf_follow_the_contract():
    t = PhaseFunctionTable(ANGLE, VALUES)
    mu, masses = segment_masses(ANGLE, VALUES)
    assert t.mu[0] == -1.0 and t.mu[-1] == 1.0 and np.all(np.diff(t.mu) > 0)
    assert np.array_equal(t.mu, mu)
    assert t.cdf.shape == (1, ANGLE.size) and t.cdf[0, 0] == 0.0 and t.cdf[0, -1] == 1.0
    assert np.allclose(np.diff(t.cdf[0]), masses, rtol=0, atol=1e-15)
    t2 = PhaseFunctionTable(ANGLE, np.vstack([VALUES, 7.0 * VALUES[::-1]]), wavelength=[450.0, 650.0])
    assert t2.cdf.shape == (2, ANGLE.size) and np.all(t2.cdf[:, -1] == 1.0) and np.all(t2.cdf[:, 0] == 0.0)
    assert np.allclose(t2.cdf[0], t.cdf[0], rtol=0, atol=1e-15)   # (normalised: the row's scale does not matter)


# -- 2. host sampler laws -------------------------------------------------------------------------------------------
def test_host_sampler_mu_law_and_uniformity_within_segments():
    np.random.seed(11)
    t = PhaseFunctionTable(ANGLE, VALUES)
    d = t.sample(200_000)
    assert d.shape == (200_000, 3)
    assert np.allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-12)
    mu_axis, masses = segment_masses(ANGLE, VALUES)
    mu = d[:, 2]
    L.assert_chi2(mu_counts(mu_axis, mu), masses, "mu segments")
    # the contract inverts a CDF that is linear in mu inside each segment: mu is uniform there
    for j in (0, 3, 6):
        inside = mu[(mu >= mu_axis[j]) & (mu < mu_axis[j + 1])]
        L.assert_ks(inside, L.uniform_cdf(mu_axis[j], mu_axis[j + 1]), ("segment", j))
    L.assert_ks(L.azimuth(d), L.uniform_cdf(-math.pi, math.pi), "azimuth")


def test_zero_mass_segments_are_never_sampled():
    angle = [0.0, 30.0, 60.0, 100.0, 140.0, 180.0]
    values = [1.0, 0.0, 0.0, 0.0, 2.0, 2.0]   # (30, 100) carries nothing
    t = PhaseFunctionTable(angle, values)
    u = np.concatenate([np.linspace(0.0, 1.0, 100_001)[:-1], t.cdf[0, 1:-1]])   # every CDF knot itself
    mu = t.sample_mu(u)
    theta = np.degrees(np.arccos(mu))
    assert not np.any((theta > 30.0 + 1e-9) & (theta < 100.0 - 1e-9))


def test_row_mixture_is_binomial_and_the_ends_are_deterministic():
    # row 0 only scatters forward (mu > 0), row 1 only backward: the row a photon took is the sign of mu
    fwd = [1.0, 1.0, 0.0, 0.0, 0.0]
    back = [0.0, 0.0, 0.0, 1.0, 1.0]
    t = PhaseFunctionTable([0.0, 45.0, 90.0, 135.0, 180.0], [fwd, back], wavelength=[500.0, 600.0])
    np.random.seed(12)
    n = 20_000
    out = np.array([t((0.0, 0.0, 1.0), 530.0) for _ in range(n)])
    L.assert_binomial(int((out[:, 2] < 0.0).sum()), n, 0.3, "row mixture at 530 nm")
    for wl, want_back in ((420.0, False), (500.0, False), (600.0, True), (900.0, True)):
        out = np.array([t((0.0, 0.0, 1.0), wl) for _ in range(500)])
        assert np.all((out[:, 2] < 0.0) == want_back), wl
    # u1 is drawn whenever there are several rows, even at a clamped end: three draws per call
    np.random.seed(5)
    t((0.0, 0.0, 1.0), 900.0)
    after = np.random.uniform()
    np.random.seed(5)
    np.random.uniform(size=3)
    assert np.random.uniform() == after


def test_the_basis_is_orthonormal_and_right_handed():
    rng = np.random.default_rng(3)
    d = rng.normal(size=(1000, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    d[:5] = [[0, 0, 1], [0, 0, -1], [1, 0, 0], [1, 0, -0.0], [0, 1e-300, -1]]   # (the poles and z = -0)
    e1, e2 = ray_basis(d)
    for a, b in ((e1, e2), (e1, d), (e2, d)):
        assert np.allclose(np.sum(a * b, axis=1), 0.0, atol=1e-12)
    assert np.allclose(np.linalg.norm(e1, axis=1), 1.0) and np.allclose(np.linalg.norm(e2, axis=1), 1.0)
    assert np.allclose(np.cross(e1, e2), d, atol=1e-12)


# -- 3. host Python tracer: the frame is the ray ----------------------------------------------------------------------
def test_host_tracer_scatters_about_the_incoming_ray():
    t = PhaseFunctionTable(ANGLE, VALUES)
    scene = medium_scene(Scatterer(1.0, quantum_yield=1.0, phase_function=t))
    d_in = np.array([0.48, -0.6, 0.64])
    d_in /= np.linalg.norm(d_in)
    np.random.seed(13)
    out = []
    for _ in range(3000):
        history = photon_tracer.follow(scene, Ray((0.0, 0.0, 0.0), tuple(d_in), 555.0), maxsteps=2, backend="host")
        scatters = [r for r, event in history if event.name == "SCATTER"]
        out.append(scatters[0].direction)
    d = np.array(out)
    mu = d @ d_in
    mu_axis, masses = segment_masses(ANGLE, VALUES)
    L.assert_chi2(mu_counts(mu_axis, mu), masses, "mu about d_in")
    e1, e2 = ray_basis(d_in)
    L.assert_ks(np.arctan2(d @ e2, d @ e1), L.uniform_cdf(-math.pi, math.pi), "azimuth about d_in")
    # about +z the law would be another one: the forward peak is along d_in, not along z
    assert abs(float(np.mean(mu)) - float(np.mean(d[:, 2]))) > 0.05


def test_luminophore_emit_passes_the_direction_and_keeps_its_draw_order():
    t = PhaseFunctionTable([0.0, 180.0], [1.0, 1.0])
    lum = Luminophore(1.0, emission=np.column_stack(([500.0, 600.0, 700.0], [0.0, 1.0, 0.0])), phase_function=t)
    ray = Ray((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), 450.0)
    np.random.seed(21)
    new = lum.emit(ray, method="full")
    np.random.seed(21)
    u2, u3, u_wl = np.random.uniform(size=3)
    assert np.isclose(float(np.dot(new.direction, ray.direction)), 2.0 * u2 - 1.0, atol=1e-12)
    assert np.isclose(new.wavelength, lum._ems_dist.sample(u_wl))
    # the built-ins are still called without arguments, about +z
    np.random.seed(22)
    iso = Scatterer(1.0, phase_function=isotropic).emit(ray)
    np.random.seed(22)
    assert np.array_equal(np.asarray(iso.direction), isotropic())


# -- 4. flattener ---------------------------------------------------------------------------------------------------
def test_flattener_pools_tables_by_identity():
    shared = PhaseFunctionTable(ANGLE, VALUES)
    other = PhaseFunctionTable([0.0, 90.0, 180.0], [[1.0, 2.0, 3.0], [3.0, 2.0, 1.0]], wavelength=[400.0, 700.0])
    world = Node(name="world", geometry=Box((100.0, 100.0, 100.0), material=Material(refractive_index=1.0)))
    Node(name="a", parent=world, geometry=Box((1.0, 1.0, 1.0), material=Material(refractive_index=1.5, components=[
        Scatterer(1.0, phase_function=shared, name="s1"), Scatterer(2.0, phase_function=HenyeyGreenstein(0.5))])))
    b = Node(name="b", parent=world, geometry=Box((1.0, 1.0, 1.0), material=Material(refractive_index=1.5, components=[
        Scatterer(1.0, phase_function=other), Scatterer(3.0, phase_function=shared, name="s2")])))
    b.location = (3.0, 0.0, 0.0)
    c = compile_scene(Scene(world))
    assert c.comp_phase_type.tolist() == [PHASE_TABLE, 1, PHASE_TABLE, PHASE_TABLE]
    assert c.comp_phase_table.tolist() == [0, -1, 1, 0]
    assert c.n_phase_tables == 2
    assert c.ptab_nw.tolist() == [1, 2] and c.ptab_nmu.tolist() == [ANGLE.size, 3]
    assert c.ptab_wl_start.tolist() == [0, 1] and c.ptab_mu_start.tolist() == [0, ANGLE.size]
    assert c.ptab_cdf_start.tolist() == [0, ANGLE.size]
    assert np.array_equal(c.ptab_mu, np.concatenate([shared.mu, other.mu]))
    assert np.array_equal(c.ptab_cdf, np.concatenate([shared.cdf.ravel(), other.cdf.ravel()]))
    assert c.ptab_wavelength.tolist()[1:] == [400.0, 700.0]
    for name in ("comp_phase_table", "ptab_nw", "ptab_nmu", "ptab_mu", "ptab_cdf"):
        assert name in c.TABLE_FIELDS and name in c.tables()
    assert c.comp_phase_table.dtype == np.int32 and c.ptab_cdf.dtype == np.float64


def test_scenes_without_tables_have_empty_pools():
    c = compile_scene(medium_scene(Scatterer(1.0, phase_function=isotropic)))
    assert c.comp_phase_table.tolist() == [-1] and c.n_phase_tables == 0 and c.ptab_cdf.size == 0
    from pvtrace_amd.engine import native as N
    assert N.phase_tables_struct(c) == (None, {})


def test_lambda_phase_function_still_raises():
    with pytest.raises(UnsupportedSceneError, match="custom phase functions are not supported"):
        compile_scene(medium_scene(Scatterer(1.0, phase_function=lambda: (0.0, 0.0, 1.0))))


# -- 5. ABI and refusals --------------------------------------------------------------------------------------------
def test_phase_tables_struct_matches_the_header(tmp_path):
    from pvtrace_amd.engine import native as N

    fields = [f for f, _ in N.PvtPhaseTables._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("size %zu\\n", sizeof(PvtPhaseTables));']
    lines += [f'printf("{f} %zu\\n", offsetof(PvtPhaseTables, {f}));' for f in fields]
    lines += ['printf("tag %d\\n", (int)PVT_PHASE_TABLE);', "return 0;}"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).strip().splitlines())
    assert int(got.pop("size")) == C.sizeof(N.PvtPhaseTables)
    assert int(got.pop("tag")) == PHASE_TABLE == 4
    for f, off in got.items():
        assert getattr(N.PvtPhaseTables, f).offset == int(off), f
    text = open(HEADER).read()
    assert "int pvt_scene_create_phase(" in text and "pvt_scene_create_phase" in N.ABI_SYMBOLS
    assert N.load_library().pvt_abi_version() == 13   # (an extension within v13)


def test_host_buffer_entry_refuses_table_scenes():
    from pvtrace_amd.engine import _kernel

    c = compile_scene(medium_scene(Scatterer(1.0, phase_function=PhaseFunctionTable(ANGLE, VALUES))))
    with pytest.raises(UnsupportedSceneError, match="phase"):
        _kernel._host_buffer_scene(c)
    with pytest.raises(UnsupportedSceneError, match="phase"):
        _kernel.trace_bundle(c, np.zeros((1, 3)), np.array([[1.0, 0.0, 0.0]]), np.array([555.0]), 0, 10, 4, 0, 1, 1)


# -- 6. spec reader and lights --------------------------------------------------------------------------------------
def test_spec_reader_builds_the_table():
    base = {
        "version": "1.0",
        "nodes": {
            "world": {"box": {"size": [20, 20, 20], "material": {"refractive-index": 1.0}}},
            "slab": {"box": {"size": [4, 4, 1], "material": {"refractive-index": 1.5, "components": ["mist"]}}},
        },
        "components": {"mist": {"scatterer": {"coefficient": 0.7, "phase-function": {"table": {
            "angle": [0, 90, 180], "values": [[3, 1, 2], [1, 1, 1]], "wavelength": [450, 650]}}}}},
    }
    scene = spec.load(base)
    c = compile_scene(scene)
    assert c.comp_phase_type.tolist() == [PHASE_TABLE] and c.n_phase_tables == 1 and c.ptab_nw.tolist() == [2]
    table = scene.root.children[0].geometry.material.components[0].phase_function
    assert isinstance(table, PhaseFunctionTable) and table.wavelength.tolist() == [450.0, 650.0]
    bad = dict(base, components={"mist": {"scatterer": {"coefficient": 0.7, "phase-function": {"table": {
        "angle": [0, 90, 170], "values": [1, 1, 1]}}}}})
    with pytest.raises(spec.SpecError):
        spec.load(bad)


def light_scene(direction):
    world = Node(name="world", geometry=Box((100.0, 100.0, 100.0), material=Material(refractive_index=1.0)))
    Node(name="lamp", parent=world, light=Light(direction=direction, name="lamp"))
    return Scene(world)


def test_a_table_as_a_light_direction_samples_on_the_host():
    t = PhaseFunctionTable(ANGLE, VALUES)
    scene = light_scene(t)
    np.random.seed(31)
    one = t()
    assert one.shape == (3,) and np.isclose(np.linalg.norm(one), 1.0)
    np.random.seed(32)
    _, dirs, _, _ = E.emit_bundle(scene, 100_000)
    mu_axis, masses = segment_masses(ANGLE, VALUES)
    L.assert_chi2(mu_counts(mu_axis, dirs[:, 2]), masses, "light mu about +z")
    with pytest.raises(UnsupportedSceneError):
        E.EmitterTables(scene, strict=True)   # what emission="device" builds: the light cannot be lowered
    tab = E.EmitterTables(scene, strict=False)   # emission="auto" / "host": the table is the light's user delegate
    assert tab.custom[0]["direction"] is t
