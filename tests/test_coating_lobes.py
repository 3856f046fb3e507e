"""Scattering coatings without a GPU: the constructors, the flattener's rows and pooling, the float64 restatement of the
rule against the exact reference ray by ray, the named wrong rules, the host delegate on the same rays, and the law of
mu about the axis (tests/lobe_cases.py holds the cases, the references and the derivation of the bound)."""
import math

import numpy as np
import pytest
from mpmath import mpf

from pvtrace_amd import Box, CoatedSurfaceDelegate, Coating, Material, Node, Ray, ScatterLobe, Scene, Surface
from pvtrace_amd.engine import _kernel
from pvtrace_amd.engine.compiler import COAT_LOBE, UnsupportedSceneError, compile_scene
from pvtrace_amd.material import ray_basis
from tests import laws as L
from tests import lobe_cases as LC

IDS = [c.name for c in LC.CASES]


# ---- constructors --------------------------------------------------------------------------------------------------------------
def test_scatter_lobe_checks_its_table_and_its_axis():
    table = LC.COSINE.table
    for about in ("normal", "specular", "refracted", "straight"):
        assert ScatterLobe(table, about).about == about
    assert ScatterLobe(table).about == "normal"
    with pytest.raises(ValueError, match="about must be one of"):
        ScatterLobe(table, "mirror")
    with pytest.raises(ValueError, match="PhaseFunctionTable"):
        ScatterLobe([0.0, 1.0])


def test_a_coating_checks_the_slot_a_lobe_sits_in():
    table = LC.COSINE.table
    for about in ("normal", "specular"):
        assert Coating(None, reflection=ScatterLobe(table, about)).reflection.about == about
    for about in ("normal", "refracted", "straight"):
        assert Coating(None, transmission=ScatterLobe(table, about)).transmission.about == about
    for about in ("refracted", "straight"):
        with pytest.raises(ValueError, match="a reflection lobe must be about"):
            Coating(None, reflection=ScatterLobe(table, about))
    with pytest.raises(ValueError, match="a transmission lobe must be about"):
        Coating(None, transmission=ScatterLobe(table, "specular"))
    # the strings keep working exactly as before
    c = Coating((0, 0, 1), reflection="lambertian", transmission="matched")
    assert (c.reflection, c.transmission) == ("lambertian", "matched")
    with pytest.raises(ValueError, match="reflection must be one of"):
        Coating(None, reflection="glossy")
    with pytest.raises(ValueError, match="transmission must be one of"):
        Coating(None, transmission="diffuse")


def test_the_lambertian_builder_has_a_knot_at_ninety_degrees():
    lobe = ScatterLobe.lambertian()
    t = lobe.table
    assert lobe.about == "normal" and t.angle.size == 257 and t.angle[128] == 90.0
    assert np.all(t.values[128:] == 0.0) and np.all(t.values[:128] > 0.0)
    assert np.array_equal(t.values[:128], np.cos(np.radians(t.angle[:128])))
    assert t.cdf[0, 128] == 0.0 and t.cdf[0, 129] > 0.0            # (mu runs from -1: no mass below the horizon)
    # p = mu is linear in mu: the trapezoid CDF is the cosine law's, F(mu) = mu^2
    assert np.allclose(t.cdf[0, 128:], t.mu[128:] ** 2, rtol=0, atol=1e-12)
    assert ScatterLobe.lambertian(nodes=5, about="specular").about == "specular"
    with pytest.raises(ValueError):
        ScatterLobe.lambertian(nodes=256)


def test_the_gaussian_builder_tabulates_the_lobe_it_names():
    lobe = ScatterLobe.gaussian(5.0, "specular", nodes=721)
    t = lobe.table
    assert lobe.about == "specular" and t.angle.size == 721 and t.angle[0] == 0.0 and t.angle[-1] == 180.0
    assert np.allclose(t.values, np.exp(-0.5 * (t.angle / 5.0) ** 2), rtol=1e-15, atol=0)
    with pytest.raises(ValueError):
        ScatterLobe.gaussian(0.0, "normal")
    with pytest.raises(ValueError, match="about must be one of"):
        ScatterLobe.gaussian(5.0, "sideways")
    with pytest.raises(ValueError, match="too small"):
        ScatterLobe.gaussian(0.01, "normal", nodes=181)


# ---- the flattener -------------------------------------------------------------------------------------------------------------
def _scene(coatings):
    world = Node(name="world", geometry=Box((50.0, 50.0, 50.0), material=Material(refractive_index=1.0)))
    material = Material(refractive_index=1.5, surface=Surface(delegate=CoatedSurfaceDelegate(coatings)))
    Node(name="plate", parent=world, geometry=Box((4.0, 4.0, 1.0), material=material))
    return Scene(world)


def test_the_flattener_lowers_table_and_axis_and_pools_a_shared_table_once():
    table = LC.COSINE.table
    shared = ScatterLobe(table, "normal")
    gloss = ScatterLobe.gaussian(5.0, "specular")
    coatings = [
        Coating((0, 0, 1), reflectivity=1.0, reflection=shared),
        Coating((0, 0, -1), reflectivity=0.0, transmission=ScatterLobe(table, "straight")),     # (another lobe, the same table)
        Coating((1, 0, 0), reflectivity=0.5, reflection=gloss, transmission=shared),
        Coating((0, 1, 0), reflectivity=0.5, reflection="lambertian", transmission=ScatterLobe(gloss.table, "refracted")),
    ]
    c = compile_scene(_scene(coatings))
    assert c.has_coating_lobes and c.n_phase_tables == 2
    assert c.ptab_nmu.tolist() == [table.mu.size, gloss.table.mu.size]
    assert c.coat_reflect_mode.tolist() == [COAT_LOBE + 0, 0, COAT_LOBE + 4 * 1 + 1, 1]
    assert c.coat_transmit_mode.tolist() == [0, COAT_LOBE + 3, COAT_LOBE + 0, COAT_LOBE + 4 * 1 + 2]
    assert np.array_equal(c.ptab_cdf[:table.cdf.size], table.cdf.ravel())
    with pytest.raises(UnsupportedSceneError, match="scattering coatings"):
        _kernel._host_buffer_scene(c)


def test_a_scene_without_a_lobe_lowers_as_before():
    plain = [Coating((0, 0, 1), reflectivity=1.0, reflection="lambertian"), Coating((0, 0, -1), reflectivity=0.0, transmission="matched")]
    c = compile_scene(_scene(plain))
    assert not c.has_coating_lobes and c.n_phase_tables == 0 and c.ptab_cdf.size == 0
    assert c.coat_reflect_mode.tolist() == [1, 0] and c.coat_transmit_mode.tolist() == [0, 1]
    lobed = compile_scene(_scene(plain + [Coating((1, 0, 0), reflection=LC.COSINE)]))
    assert sorted(lobed.tables()) == sorted(c.tables())                # (no new key: the mode words carry table and axis)
    for key, value in c.tables().items():
        if key.startswith("coat_") or key.startswith("ptab_"):
            continue
        assert np.array_equal(np.asarray(value), np.asarray(lobed.tables()[key])), key


def test_a_lobe_tampered_with_after_construction_is_refused_by_the_flattener():
    lobe = ScatterLobe(LC.COSINE.table, "normal")
    coating = Coating((0, 0, 1), reflection=lobe)
    lobe.about = "straight"
    with pytest.raises(UnsupportedSceneError, match="reflection lobe"):
        compile_scene(_scene([coating]))


# ---- the restatement against the exact reference -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", IDS)
def test_the_restatement_agrees_with_the_exact_reference_ray_by_ray(name):
    x, refs, got = LC.inputs(name), LC.references(name), LC.restated(name)
    lobed = [i for i, r in enumerate(refs) if r is not None]
    ambiguous = [i for i in lobed if refs[i].ambiguous]
    assert len(lobed) >= 400 and not any(x.near), (name, len(lobed))
    assert len(ambiguous) * 100 <= len(lobed), (name, "ambiguous", len(ambiguous), len(lobed))
    assert {bool(x.inside[i]) for i in lobed} == {False, True} or name in ("refracted-60",), (name, "both sides")
    tight = sum(refs[i].bound < mpf(10) ** -12 for i in lobed)
    assert tight * 100 >= 99 * len(lobed), (name, tight)
    worst = 0.0
    for i in lobed:
        kind, direction = got[i]
        assert kind == x.kind[i]
        r = LC.ratio(direction, refs[i])
        assert r <= 1.0, (name, i, r, direction.tolist(), refs[i].ambiguous)
        assert abs(float(np.linalg.norm(direction)) - 1.0) < 1e-12
        if not refs[i].ambiguous:
            worst = max(worst, r)
    folded = sum(refs[i].folded for i in lobed)
    print(f"restatement {name}: {len(lobed)} lobe rays, {len(ambiguous)} ambiguous, {folded} folded, worst error / bound {worst:.3f}")
    if name == "gloss-specular-80":
        assert folded * 20 >= len(lobed), (name, "the fold is taken by a large share", folded)
    if name in ("cosine-reflection", "cosine-transmission", "cosine-4097"):
        assert folded == 0
    if name == "two-rows-between":
        assert {refs[i].phase.row for i in lobed} == {0, 1}
    if name == "refracted-60":         # from inside, beyond the critical angle: total reflection, the specular body
        inside = [i for i in range(x.case.n) if x.inside[i]]
        assert all(refs[i] is None and x.kind[i] == LC.REFLECT and x.at[i] == 1 for i in inside)
    if name == "straight-60":          # ... and a lobe about "straight" transmits there
        assert all(x.kind[i] == LC.TRANSMIT for i in range(x.case.n))


@pytest.mark.parametrize("fault", LC.FAULTS)
def test_every_named_wrong_rule_moves_at_least_twenty_rays_of_some_case(fault):
    moved = {}
    for name in IDS:
        x, refs, got = LC.inputs(name), LC.references(name), LC.restated(name, fault=fault)
        count = 0
        for i, r in enumerate(refs):
            kind, direction = got[i]
            if kind != x.kind[i]:
                count += 1
            elif r is not None and not r.ambiguous and LC.ratio(direction, r) > 1.0:
                count += 1
        moved[name] = count
    print(f"wrong rule {fault}: rays moved per case {moved}")
    assert max(moved.values()) >= 20, (fault, moved)


# ---- the host delegate -------------------------------------------------------------------------------------------------------
class _Geometry:
    def __init__(self, normal, index):
        self._normal = normal
        self.material = Material(refractive_index=index)

    def normal(self, position):
        return self._normal


class _Side:
    def __init__(self, geometry):
        self.geometry = geometry


class _Replay:
    """numpy's global generator replaced by a list of draws, for one call."""

    def __init__(self, draws):
        self.draws, self.at = list(draws), 0

    def __enter__(self):
        self._saved = np.random.uniform
        np.random.uniform = self._next
        return self

    def __exit__(self, *exc):
        np.random.uniform = self._saved

    def _next(self, *args, **kwargs):
        assert not args and not kwargs
        self.at += 1
        return self.draws[self.at - 1]


@pytest.mark.parametrize("name", IDS)
def test_the_host_delegate_follows_the_rule_on_the_same_rays(name):
    x, refs = LC.inputs(name), LC.references(name)
    case = x.case
    delegate = CoatedSurfaceDelegate([case.coating()])
    worst, judged = 0.0, 0
    for i in range(0, case.n, 2 if name != "refracted-60" else 1):
        inside = bool(x.inside[i])
        n1, n2 = LC.indices(inside)
        geometry = _Geometry(tuple(x.normals[i].tolist()), LC.N_BOX)
        container, adjacent = _Side(_Geometry(None, n1)), _Side(_Geometry(None, n2))
        ray = Ray(position=(0.0, 0.0, 0.0), direction=tuple(x.dirs[i].tolist()), wavelength=float(x.wl[i]))
        r = delegate.reflectivity(None, ray, geometry, container, adjacent)
        expected_r = 1.0 if (inside and x.kind[i] == LC.REFLECT and case.reflectivity == 0.0) else case.reflectivity
        assert r == expected_r, (name, i, r)
        with _Replay(x.draws[i][x.at[i]:]) as replay:
            method = delegate.transmitted_direction if x.kind[i] == LC.TRANSMIT else delegate.reflected_direction
            direction = np.array(method(None, ray, geometry, container, adjacent))
        if refs[i] is None:
            assert replay.at == 0
            continue
        assert replay.at == refs[i].used, (name, i, "draws", replay.at, refs[i].used)
        ratio = LC.ratio(direction, refs[i])
        assert ratio <= 1.0, (name, i, ratio)
        worst, judged = max(worst, ratio), judged + 1
    print(f"host delegate {name}: {judged} rays, worst error / bound {worst:.3f}")
    assert judged >= 200


# ---- the law of mu about the axis ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lobe, transmit", [(LC.COSINE, False), (ScatterLobe(LC.COSINE.table, "normal"), True),
                                            (ScatterLobe.gaussian(5.0, "specular", nodes=361), False)],
                         ids=["cosine-reflection", "cosine-transmission", "gloss-specular"])
def test_mu_about_the_axis_follows_the_tables_own_segments(lobe, transmit):
    np.random.seed(23)
    n = 20_000
    normal = np.array([0.36, -0.48, 0.8])
    d = np.array([0.6, 0.0, -0.8]) if not transmit else np.array([0.0, 0.6, 0.8])
    d = d if float(np.dot(d, normal)) < 0.0 or transmit else -d
    out = np.array([lobe.turn(d, normal, transmit, 555.0, 1.0, 1.5) for _ in range(n)])
    s = 1.0 if float(np.dot(normal, d)) < 0.0 else -1.0
    n_out = (-s if transmit else s) * normal
    axis = n_out if lobe.about == "normal" else d - 2.0 * float(np.dot(d, normal)) * normal
    assert np.all(out @ n_out >= 0.0)
    assert np.allclose(np.linalg.norm(out, axis=1), 1.0, atol=1e-12)
    table = lobe.table
    mu = np.clip(out @ axis, -1.0, 1.0)
    counts = np.histogram(mu, bins=table.mu)[0]
    L.assert_chi2(counts, np.diff(table.cdf[0]), "mu about the axis")
    e1, e2 = ray_basis(axis)
    L.assert_ks(np.arctan2(out @ e2, out @ e1), L.uniform_cdf(-math.pi, math.pi), "azimuth about the axis")
