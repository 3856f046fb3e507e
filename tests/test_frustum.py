"""`pvtrace_amd.Frustum` (a truncated cone; an extension, the reference has no such shape) on the host: its crossing
distances against an exact rational reference, the cylinder it becomes with equal radii, the geometry protocol, the
plumbing down to the packed tables, and two closed-form laws on the host tracer.

1. Exact reference (tests/frustum_cases.py writes the reference and derives the bound B): every distance
   `Frustum._ray_distances` accepts lies within B of the exact root, and count and ORDER of the crossings are the exact
   set's in the docstring's fold order (which also says which surface a distance belongs to), on every family of every shape; rays the reference itself cannot decide (through a rim, tangent, at EPS_ZERO) are set aside, at
   most 2 % of a family.  Observed on the committed seeds, worst |t - t_exact| / B per family over the five shapes and
   (ambiguous rays of 300, the largest over the shapes):
       outside 0.52 (0)   inside 0.58 (0)   rims 0.60 (1)   axis 0.24 (2, the full cone: its two rays ON the axis)
       plane 0.58 (0)     slant 0.62 (0)    apex 0.36 (0)
   (the largest ratios are cap crossings, two roundings against B = 3u|t|; a side root uses a small part of its bound).
   Of the slant family 113 .. 196 rays per shape take the cancellation-free branch and 144 .. 170 have a < 0.
2. Cylinder anchor: `Frustum(L, r, r)` gives the distances and normals of `Cylinder(L, r)`, `np.array_equal`.
3. Protocol: crossing points are on the surface, chord midpoints inside, normals unit, outward, orthogonal to the generator.
4. Plumbing: lowering and its rejections, the spec reader, the library's refusals (no GPU needed).
5. Laws, on `photon_tracer.follow(..., backend="host")`, 3000 fixed-seed rays each, within 4 standard errors:
   solid-angle partition of a point source on the axis, z = -0.05 (top cap), -1.80 (bottom cap), +1.49 (side), binomial
   sigma; mean chord 4V/S under uniform isotropic illumination, 787 chords, z = -1.15 with the sample's sigma.
"""
import math

import numpy as np
import pytest

from pvtrace_amd import Box, Cylinder, Frustum, Material, Node, Ray, Scene, Sphere
from pvtrace_amd import spec as spec_mod
from pvtrace_amd.algorithm import photon_tracer
from pvtrace_amd.engine import compile_scene, native
from pvtrace_amd.engine.compiler import GEOM_FRUSTUM, UnsupportedSceneError
from tests import frustum_cases as C

CASES = [(shape, family) for shape in C.SHAPES for family in C.families_of(shape)]


# -- 1. exact reference ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, family", CASES)
def test_crossing_distances_against_the_exact_reference(shape, family):
    params = C.SHAPES[shape]
    frustum = Frustum(*params)
    origins, directions = C.rays(shape, family)
    ambiguous, worst, hits = 0, 0.0, 0
    for o, d in zip(origins, directions):
        got = frustum._ray_distances(o, d)
        verdict, ratio = C.judge(params, o, d, got)
        if verdict == "ambiguous":
            ambiguous += 1
            continue
        assert verdict == "ok", (shape, family, o.tolist(), d.tolist(), verdict)
        worst, hits = max(worst, ratio), hits + bool(got)
    print(f"{shape} {family}: worst |t - t_exact| / B = {worst:.3f}, {ambiguous} ambiguous, {hits} rays cross")
    assert ambiguous <= C.MAX_AMBIGUOUS * len(origins), (shape, family, ambiguous)
    assert hits >= len(origins) // 3, (shape, family, hits)   # (the family does meet the shape)


def test_the_slant_family_takes_the_stable_branch_on_both_sides_of_the_generator():
    for shape, (L, r0, r1) in C.SHAPES.items():
        _, d = C.rays(shape, "slant")
        f = (r1 - r0) / L * d[:, 2]
        s = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
        a = s - f * f
        stable = np.abs(a) <= 2.0 ** -20 * (s + f * f)
        assert stable.sum() >= 100 and (~stable).sum() >= 50, shape
        assert (a[stable] < 0.0).sum() >= 30 and (a[stable] > 0.0).sum() >= 30, shape


# -- 2. cylinder anchor ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length, radius", [(2.0, 0.7), (10.0, 0.05), (0.1, 3.0)])
def test_equal_radii_are_the_cylinder_bit_for_bit(length, radius):
    frustum, cylinder = Frustum(length, radius, radius), Cylinder(length, radius)
    crossings = 0
    for family in C.GENERIC:
        origins, directions = C.rays((length, radius, radius), family)
        for o, d in zip(origins, directions):
            a, b = frustum._ray_distances(o, d), cylinder._ray_distances(o, d)
            assert np.array_equal(a, b), (family, o, d)
            for t in a:
                p = o + t * d
                assert np.array_equal(frustum.normal(p), cylinder.normal(p)), (family, o, d, t)
            crossings += len(a)
    assert crossings > 400


# -- 3. protocol -----------------------------------------------------------------------------------------------------------
def radial_residual_bound(params, o, d, t, p, exact):
    """How far from the side, measured along the radius, the point p = o + t d of a side root may lie: the bound B of the
    root (tests/frustum_cases.py) times the speed at which the ray closes on the wall, |(x dx + y dy)/rho - k dz|, plus the
    roundings of forming the point and r(z)."""
    L, r0, r1 = params
    k = (r1 - r0) / L
    rho = math.hypot(p[0], p[1])
    root = min((cr for cr in exact if cr.surface == "side"), key=lambda cr: abs(float(cr.t) - t))
    speed = abs((p[0] * d[0] + p[1] * d[1]) / rho - k * d[2])
    reach = math.sqrt(float(o @ o)) + abs(t)
    return 1.001 * float(root.bound) * speed + 8.0 * 2.0 ** -53 * (1.0 + abs(k)) * reach


@pytest.mark.parametrize("shape", sorted(C.SHAPES))
def test_protocol_properties(shape):
    """A crossing point lies on the surface in the sense of `is_on_surface` (the cylinder's convention: EPS_ZERO, absolute)
    wherever the point's own rounding allows -- always for rays that start inside the shape; a ray from three bounding
    radii away that grazes the needle leaves a radial residual of 2e-12, the cylinder's arithmetic does the same -- and
    within its derived residual everywhere."""
    params = L, r0, r1 = C.SHAPES[shape]
    frustum = Frustum(L, r0, r1)
    half, k = 0.5 * L, (r1 - r0) / L
    chords = sides = on_surface = 0
    for family in C.GENERIC + ("plane",):
        origins, directions = C.rays(shape, family)
        for o, d in zip(origins, directions):
            exact, ambiguous, _ = C.exact_crossings(params, o, d)
            if ambiguous:
                continue
            ts = sorted(frustum._ray_distances(o, d))
            points = [o + t * d for t in ts]
            listed = frustum.intersections(o, d)
            assert len(listed) == len(points) and all(np.array_equal(p, q) for p, q in zip(points, listed))
            for t, p in zip(ts, points):
                n = np.asarray(frustum.normal(p))
                assert abs(math.sqrt(float(n @ n)) - 1.0) <= 1e-15
                rho = math.hypot(p[0], p[1])
                if abs(abs(p[2]) - half) <= 1e-8 + 1e-5 * half:
                    assert n.tolist() == [0.0, 0.0, math.copysign(1.0, p[2])]
                    assert frustum.is_on_surface(p) and not frustum.contains(p), (shape, family, p)
                    continue
                rz = frustum.radius_at(p[2])
                bound = radial_residual_bound(params, o, d, t, p, exact)
                assert abs(rho - rz) <= bound, (shape, family, p, abs(rho - rz), bound)
                if bound < 0.5 * 2.220446049250313e-13 or family == "inside":
                    assert frustum.is_on_surface(p) and not frustum.contains(p), (shape, family, p)
                    on_surface += 1
                # the generator through p, g = (k x / rho, k y / rho, 1): n . g = k (rho - r(z)) / m, m the length the normal
                # was divided by -- zero ON the surface, so within the radial residual over m (small near the apex)
                g = np.array([k * p[0] / rho, k * p[1] / rho, 1.0])
                m = math.sqrt(rho * rho + (k * rz) ** 2)
                assert abs(float(n @ g)) / math.sqrt(float(g @ g)) <= abs(k) * bound / m + 1e-15, (shape, family, p)
                assert n[0] * p[0] + n[1] * p[1] > 0.0          # outward: away from the axis
                sides += 1
            if len(points) == 2:
                mid = 0.5 * (points[0] + points[1])
                assert frustum.contains(mid), (shape, family, mid)
                assert frustum.is_entering(points[0], d) and not frustum.is_entering(points[1], d)
                chords += 1
    assert chords > 100 and sides > 100 and on_surface > 100, (chords, sides, on_surface)
    assert not frustum.contains((0.0, 0.0, 1.01 * half)) and not frustum.contains((1.01 * max(r0, r1), 0.0, 0.0))


def test_bad_parameters_are_refused():
    # (the one point without a normal, the apex, lies on a cap plane and takes the cap's: GeometryError guards a zero vector)
    assert Frustum(2.0, 1.0, 0.0).normal((0.0, 0.0, 1.0)) == (0.0, 0.0, 1.0)
    for bad in ((0.0, 1.0, 1.0), (-1.0, 1.0, 1.0), (math.inf, 1.0, 1.0), (1.0, -0.1, 1.0), (1.0, 1.0, math.nan),
                (1.0, math.inf, 1.0), (1.0, 0.0, 0.0)):
        with pytest.raises(ValueError):
            Frustum(*bad)
    Frustum(1.0, 0.0, 1.0), Frustum(1.0, 1.0, 0.0)


# -- 4. plumbing -------------------------------------------------------------------------------------------------------------
def taper_scene(params=(2.0, 1.0, 0.4), world=None):
    world = Node(name="world", geometry=world or Box((50.0, 50.0, 50.0), material=Material(refractive_index=1.0)))
    Node(name="taper", parent=world, geometry=Frustum(*params, material=Material(refractive_index=1.5)))
    return Scene(world)


def taper_array():
    """3 x 3 tapers on a slab: eleven nodes, enough for a node grid -- which a truncated cone's scene does not get."""
    world = Node(name="world", geometry=Box((50.0, 50.0, 50.0), material=Material(refractive_index=1.0)))
    Node(name="slab", parent=world, geometry=Box((6.0, 6.0, 0.5), material=Material(refractive_index=1.5)))
    for i in range(3):
        for j in range(3):
            taper = Node(name=f"taper-{i}{j}", parent=world,
                         geometry=Frustum(1.0, 0.8, 0.3, material=Material(refractive_index=1.5)))
            taper.location = (2.0 * (i - 1), 2.0 * (j - 1), 0.75)
    return Scene(world)


def test_lowering():
    compiled = compile_scene(taper_scene())
    assert compiled.has_frustum and not compile_scene(Scene(Node(name="w", geometry=Sphere(1.0, material=Material(1.0))))).has_frustum
    assert compiled.geom_type.tolist() == [0, GEOM_FRUSTUM] and GEOM_FRUSTUM == 4
    assert compiled.geom_params[1].tolist() == [2.0, 1.0, 0.4, 0.0]


@pytest.mark.parametrize("attr, value", [("length", 0.0), ("radius_bottom", -1.0), ("radius_top", math.nan),
                                         ("radius_top", "wide")])
def test_lowering_refuses_parameters_changed_after_construction(attr, value):
    scene = taper_scene()
    setattr(scene.root.children[0].geometry, attr, value)
    with pytest.raises(UnsupportedSceneError):
        compile_scene(scene)


def test_spec_reader():
    material = {"refractive-index": 1.5}
    base = {"version": "1.0", "nodes": {
        "world": {"sphere": {"radius": 10.0, "material": {"refractive-index": 1.0}}},
        "guide": {"location": [0, 0, 1], "frustum": {"length": 2, "radius-bottom": 1, "radius-top": 0.25, "material": material}},
    }}
    scene = spec_mod.load(base)
    guide = [n for n in scene.root.children if n.name == "guide"][0]
    assert isinstance(guide.geometry, Frustum)
    assert (guide.geometry.length, guide.geometry.radius_bottom, guide.geometry.radius_top) == (2, 1, 0.25)
    assert compile_scene(scene).has_frustum
    bad = dict(base, nodes=dict(base["nodes"], guide={"frustum": {"length": 2, "radius-bottom": 0, "radius-top": 0,
                                                                  "material": material}}))
    with pytest.raises(spec_mod.SpecError, match="not both be 0"):
        spec_mod.load(bad)
    with pytest.raises(spec_mod.SpecError, match="frustum"):
        spec_mod.load(dict(base, nodes=dict(base["nodes"], guide={"location": [0, 0, 1]})))


def built():
    if not native.library_built():
        pytest.skip("library not built")


def test_the_library_never_proves_a_frustum_scene_lean_and_plans_no_grid_for_it():
    built()
    box_twin = Scene(Node(name="world", geometry=Box((50.0, 50.0, 50.0), material=Material(refractive_index=1.0))))
    Node(name="block", parent=box_twin.root, geometry=Box((1.0, 1.0, 2.0), material=Material(refractive_index=1.5)))
    assert native.lean_kind(compile_scene(box_twin)) != 0      # (the same scene with a box is lean ...)
    assert native.lean_kind(compile_scene(taper_scene())) == 0   # (... with a truncated cone it is not)
    assert native.lean_kind(compile_scene(taper_scene(world=Sphere(30.0, material=Material(refractive_index=1.0))))) == 0
    array = compile_scene(taper_array())
    assert array.geom_type.shape[0] >= 8 and native.node_grid_plan(array) is None
    boxes = taper_array()
    for node in boxes.root.children:
        if isinstance(node.geometry, Frustum):
            node.geometry = Cylinder(1.0, 0.8, material=node.geometry.material)
    assert native.node_grid_plan(compile_scene(boxes)) is not None   # (the same layout of cylinders does get one)


@pytest.mark.parametrize("params, message", [
    ((0.0, 1.0, 1.0), "frustum: length"), ((math.nan, 1.0, 1.0), "frustum: length"), ((math.inf, 1.0, 1.0), "frustum: length"),
    ((1.0, -1.0, 1.0), "frustum: radii must be finite"), ((1.0, 1.0, math.inf), "frustum: radii must be finite"),
    ((1.0, 0.0, 0.0), "frustum: radii must not both be 0"),
])
def test_the_packer_refuses_bad_parameters_with_a_message(params, message):
    built()
    compiled = compile_scene(taper_scene())
    compiled.geom_params[1, :3] = params
    with pytest.raises(ValueError, match=message):
        native.lean_kind(compiled)
    compiled.geom_type[1] = 5
    with pytest.raises(ValueError, match="unknown geometry type"):
        native.lean_kind(compiled)


# -- 5. closed-form laws on the host tracer ----------------------------------------------------------------------------
N_LAW = 3000


def host_histories(origins, directions):
    scene = C.law_scene()
    np.random.seed(7)   # (an n = 1 scene draws nothing; fixed all the same)
    return [photon_tracer.follow(scene, Ray(tuple(o), tuple(d), 555.0), backend="host") for o, d in zip(origins, directions)]


def test_solid_angle_partition_on_the_host_tracer():
    histories = host_histories(*C.point_source_rays(N_LAW))
    assert all([e.name for _, e in h] == ["GENERATE", "TRANSMIT", "EXIT"] for h in histories)
    where = C.which_surface(np.array([h[1][0].position for h in histories]))
    for j, (name, p) in enumerate(zip(("top", "bottom", "side"), C.partition_probabilities())):
        k = int(np.sum(where == j))
        z = (k - N_LAW * p) / math.sqrt(N_LAW * p * (1.0 - p))
        print(f"{name}: {k} of {N_LAW}, expected {N_LAW * p:.1f}, z = {z:+.2f}")
        assert abs(z) <= 4.0, (name, k, z)


def test_mean_chord_on_the_host_tracer():
    histories = host_histories(*C.chord_rays(N_LAW))
    chords = []
    for h in histories:
        names = [e.name for _, e in h]
        assert names in (["GENERATE", "EXIT"], ["GENERATE", "TRANSMIT", "TRANSMIT", "EXIT"]), names
        if len(h) == 4:
            chords.append(math.dist(h[1][0].position, h[2][0].position))
    chords = np.array(chords)
    z = (chords.mean() - C.mean_chord()) / (chords.std(ddof=1) / math.sqrt(len(chords)))
    print(f"{len(chords)} chords, mean {chords.mean():.4f}, 4V/S = {C.mean_chord():.4f}, z = {z:+.2f}")
    assert len(chords) > 500 and abs(z) <= 4.0, z
