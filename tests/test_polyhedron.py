"""Convex polyhedra (`pvtrace_amd.Polyhedron`, PVT_GEOM_POLYHEDRON) on the host: no GPU needed.

1. The class against the exact rational reference of tests/polyhedron_cases.py, per shape and family: count, order and the
   derived bound B of every crossing distance; at most 2 % of a family's rays may be ambiguous.
2. The normal rule (nearest row, the first of equals), `contains` / `is_on_surface` with the tolerances of `Box`, and the
   box as six planes against `Box` itself.
3. The constructors: prism plane order, `from_vertices`, volume and surface area against closed forms.
4. Every refusal, with its message.
5. The flattener's tables, and that a scene without the shape lowers as before; the spec reader; the library's packer
   (host code only) never plans a node grid for such a scene; the host tracer through a hexagonal plate.
"""
import math

import numpy as np
import pytest

from pvtrace_amd import Absorber, Box, Material, Node, Polyhedron, Ray, Scene, Sphere
from pvtrace_amd import spec as spec_mod
from pvtrace_amd.algorithm import photon_tracer
from pvtrace_amd.engine import compile_scene, native
from pvtrace_amd.engine.compiler import GEOM_POLYHEDRON, UnsupportedSceneError
from pvtrace_amd.geometry import EPS_ZERO, MAX_POLYHEDRON_PLANES
from tests import polyhedron_cases as C


# -- 1. the exact reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", C.SHAPES)
def test_crossing_distances_against_the_exact_reference(shape):
    solid = C.shape(shape)
    assert C.families_of(shape) == [f for f in C.FAMILIES if f != "parallel" or shape != "tetra"]
    for family in C.families_of(shape):
        o, d = C.rays(shape, family)
        ambiguous, hits, worst = 0, 0, 0.0
        for i in range(C.N_RAYS):
            found = solid._ray_distances(o[i], d[i])
            verdict, ratio = C.judge(solid.planes, o[i], d[i], found)
            if verdict == "ambiguous":
                ambiguous += 1
                continue
            assert verdict == "ok", (shape, family, i, verdict)
            hits += bool(found)
            worst = max(worst, ratio)
        print(f"{shape} {family}: {hits} hits, {ambiguous} ambiguous, worst |dt| / B = {worst:.3f}")
        assert ambiguous <= C.MAX_AMBIGUOUS * C.N_RAYS, (shape, family, ambiguous)
        assert hits >= C.N_RAYS // 2, (shape, family, hits)
        if family == "parallel":
            assert ambiguous == 0
            assert all(np.count_nonzero(row) == 1 for row in d)


def test_the_reference_notices_a_wrong_distance_a_lost_and_an_invented_crossing():
    solid = C.shape("hexagon")
    o, d = C.rays("hexagon", "outside")
    i = next(i for i in range(C.N_RAYS) if len(solid._ray_distances(o[i], d[i])) == 2)
    found = solid._ray_distances(o[i], d[i])
    assert C.judge(solid.planes, o[i], d[i], found)[0] == "ok"
    assert "off the exact" in C.judge(solid.planes, o[i], d[i], [found[0] * (1.0 + 1e-13), found[1]])[0]
    assert "crossings" in C.judge(solid.planes, o[i], d[i], found[:1])[0]
    assert "off the exact" in C.judge(solid.planes, o[i], d[i], found[::-1])[0]
    j = next(j for j in range(C.N_RAYS) if not solid._ray_distances(o[j], d[j]))
    assert "crossings" in C.judge(solid.planes, o[j], d[j], [1.0])[0]
    # a ray through an edge, exactly, is a graze the reference sets aside
    assert C.exact_crossings(Polyhedron.box((2.0, 2.0, 2.0)).planes, (-3.0, 1.0, -1.0), (1.0, 0.0, 1.0))[1]


# -- 2. normal, contains, is_on_surface ---------------------------------------------------------------------------------
def test_the_normal_is_the_nearest_row_and_the_first_of_equals():
    box = Polyhedron.box((2.0, 4.0, 6.0))
    assert box.normal((1.0, 0.3, 0.2)) == (1.0, 0.0, 0.0) == box.facet_normal(1)
    assert box.normal((0.2, -2.0, 0.2)) == (0.0, -1.0, 0.0)
    assert box.normal((1.0, 2.0, 3.0)) == (1.0, 0.0, 0.0)         # a corner: rows 1, 3 and 5 tie, the first wins
    assert box.normal((-1.0, 2.0, -3.0)) == (-1.0, 0.0, 0.0)
    assert box.normal((0.0, 2.0, 3.0)) == (0.0, 1.0, 0.0)
    for shape in C.SHAPES:
        solid = C.shape(shape)
        o, d = C.rays(shape, "inside")
        for i in range(0, C.N_RAYS, 7):
            (t,) = solid._ray_distances(o[i], d[i])
            p = o[i] + t * d[i]
            values = [abs(((nx * p[0] + ny * p[1]) + nz * p[2]) - h) for nx, ny, nz, h in solid.planes]
            k = values.index(min(values))
            assert solid.normal(p) == tuple(solid.planes[k, :3]) == solid.facet_normal(k)
            assert float(np.dot(solid.normal(p), d[i])) > 0.0 and not solid.is_entering(p, d[i])
            assert solid.is_on_surface(p) and not solid.contains(p) and solid.contains(o[i])


def test_the_box_of_six_planes_is_the_box():
    size = (1.0, 2.5, 0.75)
    box, planes = Box(size), Polyhedron.box(size)
    assert planes.planes.tolist() == [[-1, 0, 0, 0.5], [1, 0, 0, 0.5], [0, -1, 0, 1.25], [0, 1, 0, 1.25], [0, 0, -1, 0.375], [0, 0, 1, 0.375]]
    rng = np.random.default_rng(5)
    o = rng.uniform(-2.0, 2.0, (400, 3))
    d = C._unit(rng.uniform(-0.5, 0.5, (400, 3)) * np.array(size) - o)      # aimed into the box
    d[:60] = np.eye(3)[rng.integers(0, 3, 60)] * np.where(rng.integers(0, 2, 60) == 1, 1.0, -1.0)[:, None]
    hits = 0
    for oi, di in zip(o, d):
        a, b = box._ray_distances(oi, di), planes._ray_distances(oi, di)
        assert len(a) == len(b) and np.allclose(a, b, rtol=1e-12, atol=0.0)
        hits += bool(a)
        assert box.contains(oi) == planes.contains(oi)
        for t in b:
            assert box.normal(oi + t * di) == planes.normal(oi + t * di)
    assert hits > 100
    for p in ((0.5, 0.0, 0.0), (0.5, 1.25, 0.375), (0.5 + 0.5 * EPS_ZERO, 0.1, 0.1), (0.5 + 2 * EPS_ZERO, 0.1, 0.1),
              (0.5 - 2 * EPS_ZERO, 0.1, 0.1), (0.0, 0.0, 0.0), (0.5, 2.0, 0.0)):
        assert box.is_on_surface(p) == planes.is_on_surface(p), p
        assert box.contains(p) == planes.contains(p), p


def test_the_solid_need_not_contain_the_origin():
    rows = Polyhedron.box((1.0, 1.0, 1.0)).planes.copy()
    rows[:, 3] += rows[:, :3] @ np.array([3.0, 0.0, 0.0])
    away = Polyhedron(rows)
    assert not away.contains((0.0, 0.0, 0.0)) and away.contains((3.0, 0.1, -0.2))
    assert away._ray_distances((0.0, 0.0, 0.0), (1.0, 0.0, 0.0)) == [2.5, 3.5]
    assert away.volume == pytest.approx(1.0, rel=1e-12) and away.bounding_radius == pytest.approx(math.sqrt(3.5 ** 2 + 0.5), rel=1e-12)


# -- 3. constructors and properties -------------------------------------------------------------------------------------
def test_prism_plane_order_and_normalisation():
    wedge = C.shape("wedge")
    assert wedge.planes.shape == (6, 4)
    pts = np.array(C.WEDGE)
    for i in range(4):
        nx, ny, nz, h = wedge.planes[i]
        assert nz == 0.0
        for p in (pts[i], pts[(i + 1) % 4]):           # side i runs from point i to point i + 1
            assert abs(nx * p[0] + ny * p[1] - h) < 1e-15
        assert nx * pts[(i + 2) % 4][0] + ny * pts[(i + 2) % 4][1] < h
    assert wedge.planes[4].tolist() == [0.0, 0.0, -1.0, 0.75] and wedge.planes[5].tolist() == [0.0, 0.0, 1.0, 0.75]
    assert np.all(np.abs(np.sqrt(np.sum(wedge.planes[:, :3] ** 2, axis=1)) - 1.0) <= 2.0 ** -52)
    assert not wedge.planes.flags.writeable
    scaled = Polyhedron(wedge.planes * np.array([[2.0], [3.0], [0.5], [7.0], [1.0], [4.0]]))   # rows are normalised once
    assert np.allclose(scaled.planes, wedge.planes, rtol=1e-15, atol=0.0)
    with pytest.raises(ValueError, match="counter-clockwise"):
        Polyhedron.prism(C.WEDGE[::-1], 1.0)
    with pytest.raises(ValueError, match="counter-clockwise"):
        Polyhedron.prism([(0, 0), (2, 0), (0.5, 0.5), (0, 2)], 1.0)
    with pytest.raises(ValueError, match="length"):
        Polyhedron.prism(C.WEDGE, 0.0)
    with pytest.raises(ValueError, match="at least 3"):
        Polyhedron.regular_prism(2, 1.0, 1.0)


def test_from_vertices_of_a_box_gives_the_six_planes_of_the_box():
    box = Polyhedron.box((1.0, 2.0, 3.0))
    assert len(box.vertices) == 8 and sorted(len(loop) for loop in box.faces) == [4] * 6
    hull = Polyhedron.from_vertices(box.vertices)
    assert sorted(map(tuple, hull.planes.tolist())) == sorted(map(tuple, box.planes.tolist()))
    inner = np.vstack([box.vertices, [[0.1, 0.2, 0.3]], 0.5 * (box.vertices[0] + box.vertices[1])[None]])
    assert sorted(map(tuple, Polyhedron.from_vertices(inner).planes.tolist())) == sorted(map(tuple, box.planes.tolist()))
    assert C.shape("tetra").planes.shape == (4, 4) and C.shape("pyramid").planes.shape == (6, 4)
    assert C.shape("round").planes.shape == (MAX_POLYHEDRON_PLANES, 4)
    ring = [(math.cos(a), math.sin(a), z) for a in np.linspace(0.0, 2.0 * math.pi, 63, endpoint=False) for z in (-1.0, 1.0)]
    with pytest.raises(ValueError, match="more than 64 planes"):
        Polyhedron.from_vertices(ring)
    with pytest.raises(ValueError, match="span no solid"):
        Polyhedron.from_vertices([(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0)])


def test_volume_surface_area_and_bounding_radius_against_closed_forms():
    hexagon = C.shape("hexagon")
    area = 1.5 * math.sqrt(3.0)
    assert hexagon.volume == pytest.approx(area * 0.4, rel=1e-12)
    assert hexagon.surface_area == pytest.approx(2.0 * area + 6.0 * 0.4, rel=1e-12)
    assert hexagon.bounding_radius == pytest.approx(math.hypot(1.0, 0.2), rel=1e-12)
    assert len(hexagon.vertices) == 12 and sorted(len(loop) for loop in hexagon.faces) == [4] * 6 + [6] * 2
    tetra = C.shape("tetra")
    edge = 0.8 * 2.0 * math.sqrt(2.0)
    assert tetra.volume == pytest.approx(edge ** 3 / (6.0 * math.sqrt(2.0)), rel=1e-12)
    assert tetra.surface_area == pytest.approx(math.sqrt(3.0) * edge ** 2, rel=1e-12)
    pyramid = C.shape("pyramid")    # a frustum of a square pyramid: h/3 (A1 + A2 + sqrt(A1 A2))
    assert pyramid.volume == pytest.approx((4.0 + 0.64 + 1.6) / 3.0, rel=1e-12)
    assert pyramid.surface_area == pytest.approx(4.0 + 0.64 + 4.0 * 0.5 * (2.0 + 0.8) * math.hypot(1.0, 0.6), rel=1e-12)
    n = 62
    assert C.shape("round").volume == pytest.approx(0.5 * n * math.sin(2.0 * math.pi / n) * 0.4, rel=1e-12)
    wedge = C.shape("wedge")
    assert wedge.volume == pytest.approx(0.5 * (0.5 + 0.1) * 2.0 * 1.5, rel=1e-12)
    for solid in (hexagon, tetra, pyramid, wedge):    # every face's loop runs counter-clockwise seen from outside
        for k, loop in enumerate(solid.faces):
            q = solid.vertices[loop]
            assert float(np.dot(solid.facet_normal(k), np.sum(np.cross(q, np.roll(q, -1, axis=0)), axis=0))) > 0.0


# -- 4. refusals ---------------------------------------------------------------------------------------------------------
CUBE = [[-1, 0, 0, 1], [1, 0, 0, 1], [0, -1, 0, 1], [0, 1, 0, 1], [0, 0, -1, 1], [0, 0, 1, 1]]
REFUSALS = [
    ([1.0, 2.0, 3.0], "array of rows"),
    ([[1.0, 0.0, 0.0]] * 6, "array of rows"),
    ("planes", "array of rows"),
    ([[1, 0, 0, math.nan]] + CUBE[1:], "entries must be finite"),
    ([[math.inf, 0, 0, 1]] + CUBE[1:], "entries must be finite"),
    (CUBE[:3], "between 4 and 64 planes"),
    (CUBE * 11, "between 4 and 64 planes"),
    ([[0, 0, 0, 1]] + CUBE[1:], "normals must not be zero"),
    (CUBE[:5], "is unbounded"),
    (CUBE[:4] + [[1, 1, 0, 3], [-1, -1, 0, 3]], "is unbounded"),                     # all normals in a plane
    ([[-1, 0, 0, -2]] + CUBE[1:], "empty or has no interior"),                        # x > 2 and x < 1
    ([[-1, 0, 0, -1]] + CUBE[1:], "empty or has no interior"),                        # x > 1 and x < 1: a square, no interior
    (CUBE + [[1, 1, 0, 5]], "plane 6 is redundant"),                                  # clear of the solid
    (CUBE + [[1, 1, 0, 2]], "plane 6 is redundant"),                                  # touches an edge
    (CUBE + [[1, 1, 1, 3]], "plane 6 is redundant"),                                  # touches a vertex
    (CUBE + [[2, 0, 0, 2]], "plane 6 is redundant"),                                          # a plane twice
]


@pytest.mark.parametrize("planes, message", REFUSALS)
def test_bad_plane_tables_are_refused_each_with_its_own_message(planes, message):
    assert message in Polyhedron.parameter_problem(planes)
    with pytest.raises(ValueError, match=message):
        Polyhedron(planes)


def test_a_table_is_analysed_once_and_a_copy_is_the_same_shape_bit_for_bit():
    from pvtrace_amd import geometry

    calls = []
    real = geometry._polyhedron_analysis_of
    rows = Polyhedron.regular_prism(7, 1.3, 0.9).planes * np.array([[3.0], [5.0], [7.0], [1.5], [2.5], [3.5], [6.0], [1.0], [9.0]])
    geometry._polyhedron_analysis_of = lambda planes: calls.append(1) or real(planes)
    try:
        solid = Polyhedron(rows)
        assert len(calls) == 1                                          # the constructor analyses the normalised rows, once
        twin = solid.copy(material=Material(refractive_index=1.4))
        assert Polyhedron.parameter_problem(solid.planes) is None and len(calls) == 1
        world = Node(name="world", geometry=Sphere(radius=20.0, material=Material(refractive_index=1.0)))
        Node(name="tile", parent=world, geometry=twin)
        for _ in range(3):
            compile_scene(Scene(world))                                 # every `simulate` lowers the scene again
        assert len(calls) == 1
    finally:
        geometry._polyhedron_analysis_of = real
    assert np.array_equal(twin.planes, solid.planes) and twin.volume == solid.volume and twin.material.refractive_index == 1.4
    for shape in C.SHAPES:      # the constructor divides once more: a last bit may move, and nothing else
        again = Polyhedron(C.shape(shape).planes).planes
        assert np.allclose(again, C.shape(shape).planes, rtol=4e-16, atol=0.0)
        assert np.array_equal(C.shape(shape).copy().planes, C.shape(shape).planes)


def test_sound_tables_have_no_problem():
    assert Polyhedron.parameter_problem(CUBE) is None
    assert Polyhedron.parameter_problem(CUBE + [[1, 1, 0, 1.9]]) is None       # cuts the edge off
    for shape in C.SHAPES:
        assert Polyhedron.parameter_problem(C.shape(shape).planes) is None
    assert len({message for _, message in REFUSALS}) == 7


# -- 5. through the layers ------------------------------------------------------------------------------------------------
def plate_scene(second=False):
    world = Node(name="world", geometry=Sphere(radius=20.0, material=Material(refractive_index=1.0)))
    Node(name="plate", parent=world,
         geometry=Polyhedron.regular_prism(6, 1.0, 0.4, material=Material(refractive_index=1.5, components=[Absorber(0.5)])))
    if second:
        other = Node(name="wedge", parent=world, geometry=Polyhedron.prism(C.WEDGE, 1.5, material=Material(refractive_index=1.3)))
        other.location = (4.0, 0.0, 0.0)
    return Scene(world)


def test_lowering():
    compiled = compile_scene(plate_scene(second=True))
    assert GEOM_POLYHEDRON == 5 and compiled.geom_type.tolist() == [1, 5, 5] and compiled.has_polyhedron
    assert compiled.geom_params[1].tolist() == [C.shape("hexagon").bounding_radius, 0.0, 0.0, 0.0]
    assert compiled.geom_params[2].tolist() == [C.shape("wedge").bounding_radius, 0.0, 0.0, 0.0]
    assert compiled.poly_start.tolist() == [0, 0, 8] and compiled.poly_count.tolist() == [0, 8, 6]
    assert compiled.poly_planes.shape == (14, 4) and compiled.poly_planes.dtype == np.float64
    assert np.array_equal(compiled.poly_planes[:8], C.shape("hexagon").planes)
    assert np.array_equal(compiled.poly_planes[8:], C.shape("wedge").planes)
    tables = compiled.tables()
    assert {"poly_start", "poly_count", "poly_planes"} <= set(tables)
    st, keep = native.marshal(native.PvtPolyhedronTables, compiled)
    assert (st.n_nodes, st.n_planes) == (3, 14) and np.array_equal(keep["planes"], compiled.poly_planes)
    assert native.EXTENSION_TABLES[-1] is native.PvtPolyhedronTables and native.NEWEST_ENTRY == ("pvt_scene_create_polyhedra", 10)


def test_a_scene_without_the_shape_lowers_as_before():
    world = Node(name="world", geometry=Sphere(radius=20.0, material=Material(refractive_index=1.0)))
    Node(name="block", parent=world, geometry=Box((1.0, 1.0, 1.0), material=Material(refractive_index=1.5)))
    compiled = compile_scene(Scene(world))
    assert not compiled.has_polyhedron
    assert not {"poly_start", "poly_count", "poly_planes"} & set(compiled.tables())
    assert native.marshal(native.PvtPolyhedronTables, compiled) == (None, {})
    assert compiled.poly_count.tolist() == [0, 0] and compiled.poly_planes.shape == (0, 4)


def test_lowering_refuses_planes_changed_after_construction():
    scene = plate_scene()
    solid = scene.root.children[0].geometry
    rows = solid.planes.copy()
    rows[0, :3] *= 1.0 + 1e-9
    solid._planes = rows
    with pytest.raises(UnsupportedSceneError, match="unit vectors"):
        compile_scene(scene)
    solid._planes = solid.planes[:5]
    with pytest.raises(UnsupportedSceneError, match="unbounded"):
        compile_scene(scene)
    solid._planes = np.vstack([C.shape("hexagon").planes, [[1.0, 0.0, 0.0, 5.0]]])
    with pytest.raises(UnsupportedSceneError, match="redundant"):
        compile_scene(scene)


def test_spec_reader():
    material = {"refractive-index": 1.5}
    world = {"sphere": {"radius": 10.0, "material": {"refractive-index": 1.0}}}
    base = {"version": "1.0", "nodes": {
        "world": world,
        "cube": {"location": [0, 0, 1], "polyhedron": {"planes": CUBE, "material": material}},
        "guide": {"prism": {"polygon": [list(p) for p in C.WEDGE], "length": 1.5, "material": material}},
    }}
    scene = spec_mod.load(base)
    nodes = {n.name: n for n in scene.root.children}
    assert isinstance(nodes["cube"].geometry, Polyhedron) and np.array_equal(nodes["cube"].geometry.planes, np.array(CUBE, dtype=float))
    assert np.array_equal(nodes["guide"].geometry.planes, C.shape("wedge").planes)
    assert compile_scene(scene).has_polyhedron
    bad = dict(base, nodes={"world": world, "cube": {"polyhedron": {"planes": CUBE[:5], "material": material}}})
    with pytest.raises(spec_mod.SpecError, match="unbounded"):
        spec_mod.load(bad)
    bad = dict(base, nodes={"world": world, "guide": {"prism": {"polygon": [list(p) for p in C.WEDGE[::-1]], "length": 1, "material": material}}})
    with pytest.raises(spec_mod.SpecError, match="counter-clockwise"):
        spec_mod.load(bad)
    with pytest.raises(spec_mod.SpecError, match="polyhedron"):
        spec_mod.load(dict(base, nodes={"world": world, "cube": {"location": [0, 0, 1]}}))


def test_the_library_plans_no_node_grid_for_a_scene_with_a_polyhedron(built):

    def array(make):
        world = Node(name="world", geometry=Box((20.0, 20.0, 20.0), material=Material(refractive_index=1.0)))
        for i in range(3):
            for j in range(3):
                node = Node(name=f"tile-{i}{j}", parent=world, geometry=make(material=Material(refractive_index=1.5)))
                node.location = (2.5 * (i - 1), 2.5 * (j - 1), 0.0)
        return compile_scene(Scene(world))

    assert native.node_grid_plan(array(lambda material: Box((1.0, 1.0, 0.4), material=material))) is not None
    assert native.node_grid_plan(array(lambda material: Polyhedron.regular_prism(6, 0.5, 0.4, material=material))) is None
    # the lean check is an entry from before the shape: the type is unknown to it
    with pytest.raises(ValueError, match="unknown geometry type"):
        native.lean_kind(compile_scene(plate_scene()))


def test_the_host_tracer_through_a_hexagonal_plate():
    world = Node(name="world", geometry=Sphere(radius=20.0, material=Material(refractive_index=1.0)))
    Node(name="plate", parent=world, geometry=Polyhedron.regular_prism(6, 1.0, 0.4, material=Material(refractive_index=1.0)))
    scene = Scene(world)
    solid = C.shape("hexagon")
    o, d = C.rays("hexagon", "outside")
    np.random.seed(7)   # (an n = 1 scene draws nothing; fixed all the same)
    through = 0
    for i in range(0, C.N_RAYS, 5):
        history = photon_tracer.follow(scene, Ray(tuple(o[i]), tuple(d[i]), 555.0), backend="host")
        names = [event.name for _, event in history]
        ts = solid._ray_distances(o[i], d[i])
        assert names == (["GENERATE", "TRANSMIT", "TRANSMIT", "EXIT"] if ts else ["GENERATE", "EXIT"]), (i, names)
        for (ray, _), t in zip(history[1:3], ts):
            assert np.allclose(ray.position, o[i] + t * d[i], rtol=0.0, atol=1e-12)
        through += bool(ts)
    assert through > 40
    # an index step and an absorber: the ray goes in, may be absorbed, and whatever leaves the plate leaves through a face
    np.random.seed(11)
    scene = plate_scene()
    kinds = set()
    for i in range(40):
        history = photon_tracer.follow(scene, Ray((0.1, 0.05 * (i % 7), -3.0), (0.0, 0.0, 1.0), 555.0), backend="host")
        kinds |= {event.name for _, event in history}
        assert np.allclose(history[1][0].position, (0.1, 0.05 * (i % 7), -0.2), rtol=0.0, atol=1e-12)
    assert {"GENERATE", "TRANSMIT", "ABSORB"} <= kinds
