"""Aligned luminophores (`Alignment`) without a GPU: the constructors' refusals, `Alignment.factor` against exact rational
arithmetic, the lowered emission table against the closed form, what the flattener lowers and refuses, and the host
tracer's Beer-Lambert law by angle.  Scenes: tests/aligned_scenes.py; bars: tests/laws.py."""
import hashlib
import json
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from pvtrace_amd import (
    Absorber, Alignment, ConcentrationGrid, Event, Luminophore, PhaseFunctionTable, Ray, Reactor, Scatterer, photon_tracer,
)
from pvtrace_amd.engine import compile_scene
from pvtrace_amd.engine.compiler import PHASE_ISOTROPIC, PHASE_TABLE, CompiledScene, UnsupportedSceneError
from pvtrace_amd.material import ALIGN_TABLE_NODES
from tests import aligned_scenes as A
from tests import laws as L
from tests import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


# -- constructors ------------------------------------------------------------------------------------------------------
def test_alignment_normalises_its_director_and_refuses_bad_arguments():
    a = Alignment((0.0, 3.0, 4.0), 0.25, -0.5)
    assert a.director == (0.0, 0.6, 0.8) and a.absorption_order == 0.25 and a.emission_order == -0.5
    assert Alignment((0, 0, 1)).absorption_order == 0.0 and Alignment((0, 0, 1)).emission_order == 0.0
    for bad in ((0.0, 0.0, 0.0), (1.0, 2.0), (1.0, math.nan, 0.0), (math.inf, 0.0, 0.0), "abc"):
        with pytest.raises(ValueError):
            Alignment(bad)
    for bad in (-0.5000001, 1.0000001, math.nan, math.inf, -math.inf, "x"):
        with pytest.raises(ValueError, match="absorption_order"):
            Alignment((0, 0, 1), absorption_order=bad)
        with pytest.raises(ValueError, match="emission_order"):
            Alignment((0, 0, 1), emission_order=bad)
    for edge in (-0.5, 1.0):
        Alignment((0, 0, 1), edge, edge)


def test_components_take_an_alignment_and_refuse_emission_where_it_cannot_apply():
    absorbing, emitting = Alignment((0, 0, 1), 0.6), Alignment((0, 0, 1), 0.6, 0.6)
    for make in (lambda **kw: Scatterer(1.0, **kw), lambda **kw: Absorber(1.0, **kw), lambda **kw: Reactor(1.0, **kw),
                 lambda **kw: Luminophore(1.0, x=A.X, **kw)):
        assert make().alignment is None and make(alignment=None).alignment is None
        assert make(alignment=absorbing).alignment is absorbing
        with pytest.raises(ValueError, match="Alignment"):
            make(alignment=(0, 0, 1))
    for make in (lambda **kw: Scatterer(1.0, **kw), lambda **kw: Absorber(1.0, **kw), lambda **kw: Reactor(1.0, **kw)):
        with pytest.raises(ValueError, match="Luminophore only"):
            make(alignment=emitting)
    assert Luminophore(1.0, x=A.X, alignment=emitting).alignment is emitting
    table = PhaseFunctionTable([0.0, 90.0, 180.0], [1.0, 0.5, 1.0])
    with pytest.raises(ValueError, match="phase_function"):
        Luminophore(1.0, x=A.X, alignment=emitting, phase_function=table)
    Luminophore(1.0, x=A.X, alignment=absorbing, phase_function=table)     # (absorption alone: any phase function)


# -- the law -----------------------------------------------------------------------------------------------------------
def _rounded(q):
    """The double nearest to the rational q (Python's int / int division is correctly rounded)."""
    return q.numerator / q.denominator


def _factor_exact(mu, s):
    """The stated operation order, each operation rounded once: mu mu; 1.5 x; - 0.5; S x; 1.0 -."""
    F = lambda v: Fraction(float(v))
    sq = _rounded(F(mu) * F(mu))
    a = _rounded(F(1.5) * F(sq))
    b = _rounded(F(a) - F(0.5))
    c = _rounded(F(s) * F(b))
    return _rounded(F(1.0) - F(c))


def test_factor_is_the_correctly_rounded_result_of_the_stated_operations():
    for mu in (-1.0, -1.0 / 3.0, 0.0, 0.5, 1.0):
        for s in (-0.5, 0.25, 1.0):
            got = Alignment.factor(mu, s)
            assert got == _factor_exact(mu, s), (mu, s, got)
            assert got >= 0.0
    assert Alignment.factor(1.0, 1.0) == 0.0 and Alignment.factor(0.0, 1.0) == 1.5
    assert Alignment.factor(0.3, 0.0) == 1.0
    mu = np.array([-1.0, 0.0, 1.0])
    assert Alignment.factor(mu, 1.0).tolist() == [0.0, 1.5, 0.0]


@pytest.mark.parametrize("s", [1.0, -0.5, 0.6, 0.25])
def test_emission_table_masses_are_the_closed_form_within_the_trapezoid_bound(s):
    table = Alignment((0, 0, 1), 0.0, s).emission_table
    n = ALIGN_TABLE_NODES
    assert n == 513 and table.cdf.shape == (1, n) and table.n_wavelength == 1 and table.wavelength is None
    h = 2.0 / (n - 1)
    assert table.mu[0] == -1.0 and table.mu[-1] == 1.0 and np.allclose(np.diff(table.mu), h, rtol=0, atol=1e-15)
    assert table.cdf[0, 0] == 0.0 and table.cdf[0, -1] == 1.0 and np.all(np.diff(table.cdf[0]) >= 0.0)
    # integral of f / 2 over [a, b] with f = 1 - S (1.5 mu^2 - 0.5): F(mu) = ((1 + S / 2) mu - S mu^3 / 2) / 2
    F = lambda m: 0.5 * ((1.0 + 0.5 * s) * m - 0.5 * s * m ** 3)
    exact = F(table.mu[1:]) - F(table.mu[:-1])
    bound = h ** 3 * 3.0 * abs(s) / 24.0       # trapezoid rule on f / 2: h^3 |f''| / 2 / 12, f'' = -3 S
    got = np.diff(table.cdf[0])
    print("S", s, "largest segment error", float(np.max(np.abs(got - exact))), "bound", bound)
    assert np.all(np.abs(got - exact) <= bound)
    assert abs(float(np.sum(exact)) - 1.0) < 1e-15
    assert Alignment((0, 0, 1), 0.3, 0.0).emission_table is None


# -- the flattener -----------------------------------------------------------------------------------------------------
def _digest(tables):
    h = hashlib.sha256()
    for key in sorted(tables):
        a = np.ascontiguousarray(tables[key])
        h.update(key.encode()); h.update(a.dtype.str.encode()); h.update(repr(a.shape).encode()); h.update(a.tobytes())
    return h.hexdigest()


def test_scenes_without_alignment_lower_to_the_committed_digests():
    golden = json.load(open(os.path.join(GOLD, "lowering_digests.json")))
    assert len(golden) > 5
    for name in sorted(golden):
        compiled = compile_scene(getattr(scenes, name)())
        tables = compiled.tables()
        assert not compiled.has_alignment
        assert sorted(tables) == golden[name]["keys"], name
        assert not set(tables) & set(CompiledScene.ALIGN_TABLE_FIELDS), name
        assert _digest(tables) == golden[name]["sha256"], name


def test_a_scene_with_alignment_differs_only_by_the_new_keys():
    assert set(CompiledScene.ALIGN_TABLE_FIELDS) == {"comp_align", "align_axis", "align_abs_order", "align_emit_table"}
    plain = compile_scene(scenes.lsc_equivalent()).tables()
    aligned = compile_scene(A.zero_aligned(scenes.lsc_equivalent())).tables()
    assert set(aligned) - set(CompiledScene.ALIGN_TABLE_FIELDS) == set(plain)
    for name, table in plain.items():
        assert np.array_equal(np.asarray(table), np.asarray(aligned[name]), equal_nan=True), name
    assert aligned["comp_align"].dtype == np.int32 and aligned["comp_align"].tolist() == [0, 1]
    assert aligned["align_emit_table"].tolist() == [-1, -1] and aligned["align_abs_order"].tolist() == [0.0, 0.0]


def test_directors_are_lowered_once_to_the_root_frame_and_tables_are_pooled_by_order():
    shared = Alignment((0.0, 0.0, 1.0), 0.6, 0.6)
    other = Alignment((1.0, 0.0, 0.0), 1.0, 0.6)      # an equal emission order: the same table
    third = Alignment((0.0, 1.0, 0.0), -0.5, 1.0)
    comps = [Luminophore(1.0, x=A.X, name="a", alignment=shared), Luminophore(1.0, x=A.X, name="b", alignment=shared),
             Luminophore(1.0, x=A.X, name="c", alignment=other), Luminophore(1.0, x=A.X, name="d", alignment=third),
             Absorber(1.0, name="e"), Absorber(1.0, name="f", alignment=Alignment((0, 0, 1), 0.3))]
    c = compile_scene(A.slab_scene(comps, rotate=A.TILT))
    assert c.has_alignment and c.comp_align.tolist() == [0, 0, 1, 2, -1, 3]
    R = np.asarray(c.local_to_world[c.node_names.index("slab")])[:3, :3]
    for rec, a in enumerate((shared, other, third)):
        n = a.director
        w = [(R[r, 0] * n[0] + R[r, 1] * n[1]) + R[r, 2] * n[2] for r in range(3)]
        norm = math.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
        assert c.align_axis[rec].tolist() == [v / norm for v in w]
        assert abs(float(np.dot(c.align_axis[rec], c.align_axis[rec])) - 1.0) <= 1e-12
    assert np.allclose(c.align_axis[0], [0.0, -0.5, math.sqrt(0.75)])
    assert c.align_abs_order.tolist() == [0.6, 1.0, -0.5, 0.3]
    assert c.align_emit_table.tolist() == [0, 0, 1, -1] and c.n_phase_tables == 2
    assert c.comp_phase_type.tolist() == [PHASE_TABLE] * 4 + [PHASE_ISOTROPIC] * 2
    assert c.comp_phase_table.tolist() == [0, 0, 0, 1, -1, -1]
    assert c.ptab_nw.tolist() == [1, 1] and c.ptab_nmu.tolist() == [ALIGN_TABLE_NODES] * 2
    assert np.array_equal(c.ptab_cdf[:ALIGN_TABLE_NODES], shared.emission_table.cdf[0])
    # an emission order of 0 lowers as the isotropic phase function, with no table
    iso = compile_scene(A.slab_scene([A.luminophore(1.0, (0, 0, 1), 0.6, 0.0)]))
    assert iso.comp_phase_type.tolist() == [PHASE_ISOTROPIC] and iso.n_phase_tables == 0 and iso.align_emit_table.tolist() == [-1]


def test_flattener_refusals():
    grid = ConcentrationGrid(np.ones((2, 1, 1)), (-2.0, -2.0, -0.5), (2.0, 2.0, 0.5))
    with pytest.raises(UnsupportedSceneError, match="out of scope"):
        compile_scene(A.slab_scene([A.absorber(1.0, (0, 0, 1), 0.5), Absorber(1.0, name="graded", concentration=grid)]))
    with pytest.raises(UnsupportedSceneError, match="out of scope"):
        compile_scene(A.slab_scene([Absorber(1.0, concentration=grid, alignment=Alignment((0, 0, 1), 0.5))]))
    scene = A.slab_scene([])
    scene.root.geometry.material.components = [A.absorber(0.01, (0, 0, 1), 0.5)]
    with pytest.raises(UnsupportedSceneError, match="root"):
        compile_scene(scene)
    # assigned after construction: what the constructors refuse is refused again
    late = Absorber(1.0)
    late.alignment = Alignment((0, 0, 1), 0.5, 0.5)
    with pytest.raises(UnsupportedSceneError, match="Luminophore only"):
        compile_scene(A.slab_scene([late]))
    late = Luminophore(1.0, x=A.X, phase_function=PhaseFunctionTable([0.0, 180.0], [1.0, 1.0]))
    late.alignment = Alignment((0, 0, 1), 0.5, 0.5)
    with pytest.raises(UnsupportedSceneError, match="phase function"):
        compile_scene(A.slab_scene([late]))
    late = Absorber(1.0)
    late.alignment = (0, 0, 1)
    with pytest.raises(UnsupportedSceneError, match="must be an Alignment"):
        compile_scene(A.slab_scene([late]))


def test_header_and_docstring_state_the_rule_identically():
    header = " ".join(open(os.path.join(ROOT, "include", "pvtrace_hip.h")).read().replace(" * ", " ").split())
    doc = " ".join(Alignment.__doc__.split())
    for sentence in (
        "n_w,i = (Ri,0 nx + Ri,1 ny) + Ri,2 nz, then divided by sqrt((x x + y y) + z z) of the result, without FMA.",
        "At the free-path site mu_k = (dx nx + dy ny) + dz nz, without FMA, clamped to [-1, 1].",
        "f_k = 1.0 - S_k (1.5 (mu_k mu_k) - 0.5), exactly these operations in this order.",
        "A component without alignment has f_k = 1 and is not multiplied.",
        "The depth is +inf when the scaled sum is exactly 0.",
        "the polarisation memory between a dipole emission and the next absorption is ignored.",
    ):
        assert sentence in header and sentence in doc, sentence
    assert "pvt_scene_create_aligned(" in header and "PvtAlignTables" in header


# -- host objects and tracer -------------------------------------------------------------------------------------------
def test_material_methods_keep_their_results_without_alignment_and_scale_with_it():
    from pvtrace_amd import Material

    plain = Material(1.0, components=[Absorber(2.0), Absorber(1.0)])
    assert not plain.has_alignment and plain.total_attenutation_coefficient(555.0) == 3.0
    assert plain.total_attenutation_coefficient_along(555.0, (0.0, 0.6, 0.8)) == 3.0
    m = Material(1.0, components=[A.absorber(2.0, (0, 0, 1), 1.0), Absorber(1.0)])
    assert m.has_alignment and m.total_attenutation_coefficient(555.0) == 3.0
    assert m.alignment_factors((0.0, 0.0, 1.0)) == [0.0, 1.0] and m.alignment_factors((1.0, 0.0, 0.0)) == [1.5, 1.0]
    assert m.total_attenutation_coefficient_along(555.0, (1.0, 0.0, 0.0)) == 4.0
    np.random.seed(3)
    assert all(m.component_along(555.0, (0.0, 0.0, 1.0)) is m.components[1] for _ in range(50))
    only = Material(1.0, components=[A.absorber(2.0, (0, 0, 1), 1.0)])
    np.random.seed(3)
    second = np.random.uniform(size=2)[1]
    np.random.seed(3)
    assert only.penetration_depth_along(555.0, (0.0, 0.0, 1.0)) == math.inf      # the scaled sum is exactly 0 ...
    assert np.random.uniform() == second                                         # ... and the draw was taken all the same


@pytest.mark.parametrize("theta", A.ANGLES)
def test_host_tracer_absorbs_a_pencil_by_beer_lambert_with_the_factor(theta, order=1.0):
    n, alpha = 20_000, 1.0
    scene = A.slab_scene([A.absorber(alpha, (0.0, 0.0, 1.0), order)])
    (pos, dirs, wl), chord = A.pencil(theta, 1)
    f = A.factor_along(dirs[0], (0.0, 0.0, 1.0), order)
    p = A.absorbed_probability(alpha, f, chord)
    np.random.seed(11)
    ray = Ray(position=tuple(pos[0]), direction=tuple(dirs[0]), wavelength=555.0)
    absorbed = 0
    for _ in range(n):
        events = [event for _, event, _ in photon_tracer.step_forward(scene, ray, backend="host")]
        absorbed += Event.ABSORB in events
        assert events[-1] in (Event.EXIT, Event.NONRADIATIVE)
    print("theta", theta, "S", order, "f", f, "chord", chord, "absorbed", absorbed, "of", n, "expected", p * n)
    L.assert_binomial(absorbed, n, p, (theta, order))


def test_host_luminophore_emits_about_the_director_in_the_frame_of_the_ray():
    n_dir = (1.0 / 3.0, 2.0 / 3.0, 2.0 / 3.0)
    dye = A.luminophore(5.0, n_dir, 0.0, 1.0)
    table = dye.alignment.emission_table
    ray = Ray(position=(0.0, 0.0, 0.0), direction=(0.0, 0.0, 1.0), wavelength=555.0)
    np.random.seed(5)
    out = np.array([dye.emit(ray, method="full").direction for _ in range(20_000)])
    assert np.allclose(np.linalg.norm(out, axis=1), 1.0, rtol=0, atol=1e-12)
    mu, phi = A.mu_and_azimuth(out, n_dir)
    L.assert_chi2(np.histogram(mu, bins=32, range=(-1.0, 1.0))[0], A.table_bin_masses(table, 32), "mu")
    L.assert_chi2(np.histogram(phi, bins=16, range=(-math.pi, math.pi))[0], np.full(16, 1.0 / 16.0), "azimuth")
    # the draws of an aligned emission are the isotropic one's: two, then the wavelength (no delay here)
    np.random.seed(9)
    dye.emit(ray, method="full")
    after_aligned = np.random.uniform()
    np.random.seed(9)
    A.luminophore(5.0, n_dir, 0.0, 0.0).emit(ray, method="full")
    assert np.random.uniform() == after_aligned
