"""Concentration fields (`ConcentrationGrid`, the `concentration=` keyword of the volume components) on the host: the
constructor's and the flattener's validation, the lowered tables, the ctypes struct against the C header, the host
tracer's free path held to the piecewise-exponential law, and draw-for-draw identity of a 1 x 1 x 1 field of value 1.
No GPU needed.  The expected optical depth of a chord is computed here from the exact plane-crossing parameters of the
chord, sorted -- not by a cell walk like the tracer's."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from pvtrace_amd import (
    Absorber, Box, ConcentrationGrid, Luminophore, Material, Node, Ray, Reactor, Scatterer, Scene, Surface,
)
from pvtrace_amd.algorithm import photon_tracer
from pvtrace_amd.engine import native
from pvtrace_amd.engine.compiler import UnsupportedSceneError, compile_scene
from pvtrace_amd.material import NullSurfaceDelegate
from tests import laws as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- the law, independently ---------------------------------------------------------------------------------------------
def chord_depth(lower, upper, coefficients, start, direction, t0):
    """Breakpoints s_j and optical depths tau(s_j) along start + s direction, s in [0, t0], of a lattice (lower, upper)
    with cell coefficients `coefficients` (nx, ny, nz): every interior plane's crossing parameter, sorted, and the
    coefficient of each segment's midpoint cell (clamped into the lattice)."""
    lower, upper = np.asarray(lower, float), np.asarray(upper, float)
    k = np.asarray(coefficients, float)
    n = np.array(k.shape)
    h = (upper - lower) / n
    p, d = np.asarray(start, float), np.asarray(direction, float)
    cuts = [0.0, float(t0)]
    for a in range(3):
        if d[a] == 0.0:
            continue
        for i in range(1, n[a]):
            s = (lower[a] + i * h[a] - p[a]) / d[a]
            if 0.0 < s < t0:
                cuts.append(float(s))
    s = np.unique(cuts)
    mid = p[None, :] + 0.5 * (s[:-1] + s[1:])[:, None] * d[None, :]
    cell = np.clip(np.floor((mid - lower) / h), 0, n - 1).astype(int)
    seg = k[cell[:, 0], cell[:, 1], cell[:, 2]] * np.diff(s)
    return s, np.concatenate([[0.0], np.cumsum(seg)])


def depth_cdf(s, tau):
    """The conditional CDF of the absorption depth: (1 - e^-tau(x)) / (1 - e^-tau(t0)), tau piecewise linear."""
    total = 1.0 - math.exp(-tau[-1])
    return lambda x: (1.0 - np.exp(-np.interp(x, s, tau))) / total


# -- scenes -------------------------------------------------------------------------------------------------------------
def slab_scene(components, size=(2.0, 2.0, 2.0), world_field=None):
    """An index-matched block (n = 1, NullSurfaceDelegate: no surface draws) in an n = 1 world."""
    world_components = [] if world_field is None else [Absorber(0.01, concentration=world_field)]
    world = Node(name="world", geometry=Box((40.0, 40.0, 40.0), material=Material(
        refractive_index=1.0, components=world_components)))
    block = Node(name="block", parent=world, geometry=Box(size, material=Material(
        refractive_index=1.0, surface=Surface(NullSurfaceDelegate()), components=components)))
    return Scene(world), world, block


def unit_grid():
    return ConcentrationGrid(np.ones((1, 1, 1)), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


# -- 1. the constructor -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("values, lower, upper", [
    (np.ones((2, 2)), (0, 0, 0), (1, 1, 1)),                      # not 3-D
    (np.ones((2, 0, 2)), (0, 0, 0), (1, 1, 1)),                   # an empty axis
    (np.ones((1, 1, 1, 1)), (0, 0, 0), (1, 1, 1)),                # 4-D
    (np.array([[[1.0, -0.5]]]), (0, 0, 0), (1, 1, 1)),            # negative
    (np.array([[[1.0, np.nan]]]), (0, 0, 0), (1, 1, 1)),          # NaN
    (np.array([[[1.0, np.inf]]]), (0, 0, 0), (1, 1, 1)),          # inf
    (np.ones((1, 1, 2)), (0, 0, 1), (1, 1, 1)),                   # lower == upper
    (np.ones((1, 1, 2)), (0, 2, 0), (1, 1, 1)),                   # lower > upper
    (np.ones((1, 1, 2)), (0, 0, -np.inf), (1, 1, 1)),             # infinite bound
    (np.ones((1, 1, 2)), (0, 0, 0), (1, 1, np.nan)),              # NaN bound
    (np.ones((1, 1, 2)), (0, 0), (1, 1)),                         # 2-vectors
    (np.ones((1, 1, 2)), "abc", (1, 1, 1)),                       # not numeric
])
def test_constructor_refuses_malformed_grids(values, lower, upper):
    with pytest.raises(ValueError):
        ConcentrationGrid(values, lower, upper)


def test_constructor_keeps_float64_values_and_cells_clamp():
    g = ConcentrationGrid([[[0, 1, 2, 3]]], (0.0, 0.0, -1.0), (1.0, 1.0, 1.0))
    assert g.values.dtype == np.float64 and g.shape == (1, 1, 4)
    assert np.array_equal(g.h, [1.0, 1.0, 0.5])
    assert g.cell_of((0.5, 0.5, -0.75)) == (0, 0, 0)
    assert g.cell_of((0.5, 0.5, 0.25)) == (0, 0, 2)
    assert g.cell_of((-7.0, 9.0, -30.0)) == (0, 0, 0)     # outside: the nearest edge cell
    assert g.cell_of((0.5, 0.5, 30.0)) == (0, 0, 3)


@pytest.mark.parametrize("cls", [Scatterer, Absorber, Reactor, Luminophore])
def test_every_component_takes_the_keyword(cls):
    g = unit_grid()
    kw = {"x": np.linspace(400.0, 800.0, 5)} if cls is Luminophore else {}
    assert cls(1.0, concentration=g, **kw).concentration is g
    assert cls(1.0, **kw).concentration is None
    with pytest.raises(ValueError):
        cls(1.0, concentration=np.ones((1, 1, 1)), **kw)


# -- 2. the flattener ---------------------------------------------------------------------------------------------------
def test_unfielded_scenes_lower_no_field_and_pass_no_struct():
    scene, _, _ = slab_scene([Absorber(1.0), Scatterer(0.5)])
    c = compile_scene(scene)
    assert not c.has_fields
    assert np.array_equal(c.node_field, [-1, -1]) and np.array_equal(c.comp_values, [-1, -1])
    assert c.n_fields == 0 and c.n_value_tables == 0 and c.field_values.size == 0
    assert native.field_tables_struct(c)[0] is None


def test_lowered_tables_match_hand_written_expectations():
    a = ConcentrationGrid(np.arange(8.0).reshape(2, 2, 2), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    b = ConcentrationGrid(np.full((2, 2, 2), 0.5), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    c3 = ConcentrationGrid(np.array([[[1.0, 2.0, 3.0]]]), (0.0, 0.0, 0.0), (1.0, 1.0, 3.0))
    scene, world, _ = slab_scene([Absorber(1.0, concentration=a), Scatterer(0.5), Absorber(2.0, concentration=b)])
    other = Node(name="other", parent=world, geometry=Box((1.0, 1.0, 3.0), material=Material(
        refractive_index=1.0, components=[Absorber(1.0, concentration=c3), Absorber(3.0, concentration=a.__class__(
            c3.values * 2.0, c3.lower, c3.upper)), Reactor(0.2, concentration=c3)])))
    other.translate((10.0, 0.0, 0.0))
    plain = Node(name="plain", parent=world, geometry=Box((1.0, 1.0, 1.0), material=Material(
        refractive_index=1.0, components=[Absorber(1.0)])))
    plain.translate((-10.0, 0.0, 0.0))
    c = compile_scene(scene)
    assert c.has_fields
    assert c.node_names == ["world", "block", "other", "plain"]
    assert np.array_equal(c.node_field, [-1, 0, 1, -1])
    assert np.array_equal(c.field_shape, [[2, 2, 2], [1, 1, 3]])
    assert np.array_equal(c.field_lower, [[-1.0, -1.0, -1.0], [0.0, 0.0, 0.0]])
    assert np.array_equal(c.field_upper, [[1.0, 1.0, 1.0], [1.0, 1.0, 3.0]])
    # value tables: a, ones(2,2,2) for the Scatterer, b, c3, 2 c3 -- c3 pooled once for the Reactor
    assert np.array_equal(c.comp_values, [0, 1, 2, 3, 4, 3, -1])
    assert np.array_equal(c.values_start, [0, 8, 16, 24, 27])
    assert np.array_equal(c.values_count, [8, 8, 8, 3, 3])
    want = np.concatenate([np.arange(8.0), np.ones(8), np.full(8, 0.5), [1.0, 2.0, 3.0], [2.0, 4.0, 6.0]])
    assert np.array_equal(c.field_values, want)
    for name in ("node_field", "field_shape", "field_lower", "field_upper", "comp_values", "values_start",
                 "values_count", "field_values"):
        assert name in c.TABLE_FIELDS and name in c.tables()
    st, keep = native.field_tables_struct(c)
    assert (st.n_nodes, st.n_fields, st.n_components, st.n_values, st.n_points) == (4, 2, 7, 5, 30)
    assert [st.node_field[i] for i in range(4)] == [-1, 0, 1, -1]
    assert [st.values[i] for i in range(30)] == want.tolist()


def test_mismatched_lattices_in_one_material_are_refused():
    a = ConcentrationGrid(np.ones((2, 2, 2)), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    for b in (ConcentrationGrid(np.ones((2, 2, 1)), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)),       # shape
              ConcentrationGrid(np.ones((2, 2, 2)), (-1.0, -1.0, -1.0), (1.0, 1.0, np.nextafter(1.0, 2.0))),  # a bit
              ConcentrationGrid(np.ones((2, 2, 2)), (-1.0, -1.5, -1.0), (1.0, 1.0, 1.0))):      # lower
        scene, _, _ = slab_scene([Absorber(1.0, concentration=a), Absorber(2.0, concentration=b)])
        with pytest.raises(UnsupportedSceneError, match="share their lattice"):
            compile_scene(scene)
        with pytest.raises(ValueError, match="share their lattice"):
            scene.root.children[0].geometry.material.concentration_lattice
    # the same lattice, other values: accepted
    same = ConcentrationGrid(np.full((2, 2, 2), 3.0), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    scene, _, _ = slab_scene([Absorber(1.0, concentration=a), Absorber(2.0, concentration=same)])
    assert compile_scene(scene).n_fields == 1


def test_a_field_on_the_root_is_refused():
    scene, _, _ = slab_scene([Absorber(1.0)], world_field=unit_grid())
    with pytest.raises(UnsupportedSceneError, match="root"):
        compile_scene(scene)
    with pytest.raises(UnsupportedSceneError, match="root"):
        photon_tracer.follow(scene, Ray((0.0, 0.0, 5.0), (0.0, 0.0, -1.0), 555.0), backend="host")


def test_host_buffer_entry_refuses_field_scenes():
    from pvtrace_amd.engine import _kernel

    scene, _, _ = slab_scene([Absorber(1.0, concentration=unit_grid())])
    c = compile_scene(scene)
    with pytest.raises(UnsupportedSceneError, match="concentration"):
        _kernel._host_buffer_scene(c)
    with pytest.raises(UnsupportedSceneError, match="concentration"):
        _kernel.trace_bundle(c, np.zeros((1, 3)), np.array([[1.0, 0.0, 0.0]]), np.array([555.0]), 0, 10, 4, 0, 1, 1)
    _kernel._host_buffer_scene(compile_scene(slab_scene([Absorber(1.0)])[0]))   # unfielded: as before


# -- 3. the C ABI -------------------------------------------------------------------------------------------------------
def test_field_tables_struct_matches_the_header_and_the_entry_is_exported(tmp_path):
    text = open(os.path.join(ROOT, "include", "pvtrace_hip.h")).read()
    assert "int pvt_scene_create_field(" in text and "typedef struct PvtFieldTables" in text
    assert "pvt_scene_create_field" in native.ABI_SYMBOLS
    fields = [name for name, _ in native.PvtFieldTables._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "pvtrace_hip.h"\nint main(void) {\n'
                   '    printf("%zu\\n", sizeof(PvtFieldTables));\n'
                   + "".join(f'    printf("%zu\\n", offsetof(PvtFieldTables, {f}));\n' for f in fields)
                   + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(native.PvtFieldTables)
    assert got[1:] == [getattr(native.PvtFieldTables, f).offset for f in fields]


# -- 4. the host tracer's law -------------------------------------------------------------------------------------------
def local_ray(position, direction, wavelength=555.0):
    d = np.asarray(direction, float)
    return Ray(tuple(position), tuple(d / np.linalg.norm(d)), wavelength)


def sample_absorptions(material, ray, t0, n, seed):
    np.random.seed(seed)
    out = [material.is_absorbed_in(ray, t0) for _ in range(n)]
    hit = np.array([a for a, _, _ in out])
    return hit, np.array([d for a, d, _ in out if a]), [c for a, _, c in out if a]


def test_free_path_through_a_z_gradient():
    values = np.linspace(0.1, 3.0, 8).reshape(1, 1, 8)
    grid = ConcentrationGrid(values, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    material = Material(1.0, components=[Absorber(0.8, concentration=grid)])
    ray, t0 = local_ray((0.1, -0.2, -1.0), (0.0, 0.0, 1.0)), 2.0
    s, tau = chord_depth(grid.lower, grid.upper, 0.8 * values, ray.position, ray.direction, t0)
    n = 20_000
    hit, depth, _ = sample_absorptions(material, ray, t0, n, 1)
    L.assert_binomial(int(hit.sum()), n, 1.0 - math.exp(-tau[-1]), "P(absorbed), z gradient")
    L.assert_ks(depth, depth_cdf(s, tau), "depth, z gradient")


def test_free_path_through_an_oblique_checkerboard_never_absorbs_in_a_clear_cell():
    ix, iy, iz = np.indices((4, 3, 5))
    values = np.where((ix + iy + iz) % 2 == 0, 1.5, 0.0)
    grid = ConcentrationGrid(values, (-1.0, -0.75, -1.25), (1.0, 0.75, 1.25))
    material = Material(1.0, components=[Absorber(0.7, concentration=grid)])
    start, d = np.array([-1.0, -0.6, -1.2]), np.array([0.7, 0.45, 0.8])
    ray = local_ray(start, d)
    d = np.asarray(ray.direction)
    t0 = 2.5
    s, tau = chord_depth(grid.lower, grid.upper, 0.7 * values, start, d, t0)
    assert len(s) > 6   # the chord crosses planes of all three axes
    n = 20_000
    hit, depth, cells = sample_absorptions(material, ray, t0, n, 2)
    L.assert_binomial(int(hit.sum()), n, 1.0 - math.exp(-tau[-1]), "P(absorbed), checkerboard")
    L.assert_ks(depth, depth_cdf(s, tau), "depth, checkerboard")
    assert all(values[c] > 0.0 for c in cells)
    points = start[None, :] + depth[:, None] * d[None, :]
    h = grid.h
    away = np.all(np.abs((points - grid.lower) / h - np.round((points - grid.lower) / h)) > 1e-9, axis=1)
    pc = np.clip(np.floor((points[away] - grid.lower) / h), 0, np.array(values.shape) - 1).astype(int)
    assert np.all(values[pc[:, 0], pc[:, 1], pc[:, 2]] > 0.0)


def test_clamping_for_a_lattice_smaller_than_the_node():
    values = np.array([[[0.2, 3.0]]])
    grid = ConcentrationGrid(values, (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))
    material = Material(1.0, components=[Absorber(1.0, concentration=grid)])
    ray, t0 = local_ray((0.9, 0.0, -1.0), (-0.3, 0.1, 1.0)), 2.0 / 1.0488088481701516
    s, tau = chord_depth(grid.lower, grid.upper, values, ray.position, ray.direction, t0)
    n = 20_000
    hit, depth, cells = sample_absorptions(material, ray, t0, n, 3)
    L.assert_binomial(int(hit.sum()), n, 1.0 - math.exp(-tau[-1]), "P(absorbed), clamped")
    L.assert_ks(depth, depth_cdf(s, tau), "depth, clamped")
    assert {c for c in cells} == {(0, 0, 0), (0, 0, 1)}


def test_two_components_with_different_fields_pick_per_cell():
    fa = ConcentrationGrid(np.array([[[1.0, 0.2, 0.0]]]), (-1.0, -1.0, -1.5), (1.0, 1.0, 1.5))
    fb = ConcentrationGrid(np.array([[[0.0, 2.0, 1.0]]]), (-1.0, -1.0, -1.5), (1.0, 1.0, 1.5))
    a, b = Absorber(0.6, concentration=fa, name="a"), Reactor(0.9, concentration=fb, name="b")
    material = Material(1.0, components=[a, b])
    for cell in [(0, 0, 0), (0, 0, 1), (0, 0, 2)]:
        w1, w2 = 0.6 * fa.values[cell], 0.9 * fb.values[cell]
        np.random.seed(sum(cell) + 7)
        picks = [material.component_at(555.0, cell) for _ in range(4000)]
        L.assert_binomial(sum(p is a for p in picks), len(picks), w1 / (w1 + w2), ("pick", cell))
    # and through the march: the cell absorbed in decides
    ray, t0 = local_ray((0.0, 0.0, -1.5), (0.0, 0.0, 1.0)), 3.0
    coef = 0.6 * fa.values + 0.9 * fb.values
    s, tau = chord_depth(fa.lower, fa.upper, coef, ray.position, ray.direction, t0)
    hit, depth, cells = sample_absorptions(material, ray, t0, 20_000, 8)
    L.assert_binomial(int(hit.sum()), hit.size, 1.0 - math.exp(-tau[-1]), "P(absorbed), two fields")
    L.assert_ks(depth, depth_cdf(s, tau), "depth, two fields")


def test_host_tracer_absorbs_in_the_rotated_nodes_frame():
    ix, iy, iz = np.indices((3, 3, 3))
    values = np.where((ix + iy + iz) % 2 == 0, 2.0, 0.1)
    grid = ConcentrationGrid(values, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    scene, world, block = slab_scene([Absorber(0.9, concentration=grid)])
    angle, axis = 0.6, (1.0, 2.0, 0.5)
    block.rotate(angle, axis)
    R = L.rotation(angle, axis)
    local_start, local_d = np.array([-1.5, -0.3, 0.2]), np.array([1.0, 0.35, -0.2])
    local_d /= np.linalg.norm(local_d)
    start, d = R @ local_start, R @ local_d
    t_in, t_out = 0.5 / local_d[0], 2.5 / local_d[0]   # (the chord enters at x = -1 and leaves at x = +1)
    s, tau = chord_depth(grid.lower, grid.upper, 0.9 * values, local_start + t_in * local_d, local_d, t_out - t_in)
    np.random.seed(5)
    n, where = 3000, []
    for _ in range(n):
        hist = photon_tracer.follow(scene, Ray(tuple(start), tuple(d), 555.0), backend="host")
        for r, e in hist:
            if e.name == "ABSORB":
                where.append(r.position)
    where = L.to_local(np.array(where), R)
    L.assert_binomial(len(where), n, 1.0 - math.exp(-tau[-1]), "P(absorbed), rotated node")
    L.assert_ks((where - local_start)[:, 0] / local_d[0] - t_in, depth_cdf(s, tau), "depth, rotated node")


# -- 5. identity --------------------------------------------------------------------------------------------------------
def luminophore_scene(grid):
    x = np.linspace(400.0, 800.0, 41)
    lum = Luminophore(np.column_stack([x, 2.0 * np.exp(-((x - 500.0) / 60.0) ** 2)]),
                      emission=np.column_stack([x, np.exp(-((x - 600.0) / 40.0) ** 2)]), quantum_yield=0.9,
                      concentration=grid)
    scat = Scatterer(0.3, concentration=grid)
    world = Node(name="world", geometry=Box((40.0, 40.0, 40.0), material=Material(refractive_index=1.0)))
    block = Node(name="block", parent=world, geometry=Box((2.0, 3.0, 1.0), material=Material(
        refractive_index=1.5, components=[lum, scat])))
    block.rotate(0.4, (0.0, 1.0, 1.0))
    return Scene(world)


def test_a_unit_field_traces_draw_for_draw_like_no_field():
    plain, unit = luminophore_scene(None), luminophore_scene(unit_grid())
    assert compile_scene(unit).has_fields and not compile_scene(plain).has_fields
    for k in range(200):
        ray = Ray((0.05 * (k % 7) - 0.15, 0.0, 5.0), (0.01 * (k % 5), 0.02, -1.0), 450.0 + k)
        np.random.seed(k)
        a = photon_tracer.follow(plain, ray, backend="host")
        after_a = np.random.uniform()
        np.random.seed(k)
        b = photon_tracer.follow(unit, ray, backend="host")
        after_b = np.random.uniform()
        assert len(a) == len(b) and after_a == after_b, k   # (the same number of draws)
        for (ra, ea), (rb, eb) in zip(a, b):
            assert ea == eb, (k, ea, eb)
            for f in ("position", "direction", "wavelength", "travelled", "duration", "source"):
                assert np.array_equal(getattr(ra, f), getattr(rb, f)), (k, f)
