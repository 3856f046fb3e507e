"""Scenes and helpers of the patterned-coating tests (tests/test_coating_patterns.py, tests/test_gpu_coating_patterns.py).
Four layouts that differ in which kernel serves them and in which arithmetic forms the local point -- (p1) an unrotated
box in a world, (p2) the same box rotated and shifted under a lattice smaller than its face, (p3) the 37-node tile array
with patterns of 5 x 3 x 1 and 7 x 1 x 1 cells on two tiles, (p4) a mesh beside the p1 box -- and a sphere whose coating
has `facet=None` and a mask bounded on all three axes.

Every builder takes `coating(pattern) -> Coating or None` so that one geometry serves "with this mask", "without a
pattern" and "without the coating"; `pattern` is what the layout would put on its coated face(s)."""
import numpy as np

from pvtrace_amd import (
    Absorber, Box, Coating, CoatedSurfaceDelegate, CoatingPattern, Light, Material, Mesh, Node, Scene, Sphere, Surface,
    isotropic,
)
from pvtrace_amd.engine import Recorder, compile_scene

TOP = (0.0, 0.0, 1.0)
SHIFT = (1.0, -2.0, 0.5)     # p2's location
TILES = ("tile-2-3", "tile-4-1")     # p3's two patterned tiles


def third_mask(shape, seed=5):
    """About a third of the cells set, at random from a fixed seed; at least one set and one clear cell."""
    n = int(np.prod(shape))
    flat = np.zeros(n, dtype=np.uint8)
    flat[np.random.default_rng(seed).permutation(n)[:max(1, int(round(n / 3.0)))]] = 1
    return flat.reshape(shape)


def detector(facet=TOP):
    """A perfect detector on `facet`, through the pattern it is given."""
    return lambda pattern: Coating(facet, reflectivity=0.0, absorptivity=1.0, transmission="matched", pattern=pattern)


def mirror(facet=TOP):
    return lambda pattern: Coating(facet, reflectivity=1.0, pattern=pattern)


def face_pattern(mask=None, half=5.0, shape=(8, 6, 1)):
    """A flat pattern over x, y in [-half, half), z unbounded; `mask`: an array, "ones", "zeros" or None (a random third)."""
    if isinstance(mask, str):
        mask = np.ones(shape, dtype=np.uint8) if mask == "ones" else np.zeros(shape, dtype=np.uint8)
    if mask is None:
        mask = third_mask(shape)
    return CoatingPattern(mask, (-half, -half, None), (half, half, None))


def _world(size=40.0):
    return Node(name="world", geometry=Box((size, size, size), material=Material(refractive_index=1.0)))


def _coated(coatings, roughness=0.0):
    coatings = [c for made in coatings if made is not None for c in (made if isinstance(made, list) else [made])]
    return Material(refractive_index=1.5, components=[Absorber(0.05, name="tint")],
                    surface=Surface(delegate=CoatedSurfaceDelegate(coatings, roughness=roughness)))


def _box(world, coatings, roughness=0.0):
    box = Node(name="box", parent=world, geometry=Box((10.0, 10.0, 2.0), material=_coated(coatings, roughness)))
    box.recorders = [Recorder("detected", event="detected"), Recorder("escaping", event="escaping"),
                     Recorder("lost", event="lost"), Recorder("killed-box", event="killed")]
    world.recorders = [Recorder("exit", event="exit"), Recorder("killed-world", event="killed")]
    return box


def _lamp(world, at):
    lamp = Node(name="lamp", parent=world, light=Light(direction=isotropic, name="lamp"))
    lamp.location = at
    return lamp


def p1(coating=None, pattern=None, roughness=0.0):
    """A 10 x 10 x 2 box, n = 1.5, unrotated at the origin of a 40 cm world, lit from inside."""
    coating = coating or detector()
    world = _world()
    _box(world, [coating(pattern)], roughness)
    _lamp(world, (0.5, 0.3, -0.2))
    return Scene(world)


def p2(coating=None, pattern=None):
    """The p1 box rotated 0.3 rad about y and shifted by SHIFT: the local point takes the rotation path."""
    coating = coating or detector()
    world = _world()
    box = _box(world, [coating(pattern)])
    box.rotate(0.3, (0.0, 1.0, 0.0))
    box.location = SHIFT
    _lamp(world, (SHIFT[0] + 0.4, SHIFT[1] + 0.3, SHIFT[2] - 0.1))
    return Scene(world)


def p3(coating=None, pattern=None):
    """The 37-node tile array of tests/absorbing_scenes.py; `pattern`: a pair, one per patterned tile (TILES)."""
    from benchmarks.configs import tiles_lsc

    coating = coating or detector()
    scene = tiles_lsc(6, recorders=None)
    patterns = pattern if isinstance(pattern, (tuple, list)) else (pattern, pattern)
    for name, pat in zip(TILES, patterns):
        tile = next(n for n in scene.root.preorder() if n.name == name)
        material = tile.geometry.material
        made = coating(pat)
        tile.geometry.material = Material(
            refractive_index=material.refractive_index, components=list(material.components),
            surface=Surface(delegate=CoatedSurfaceDelegate([] if made is None else [made])))
        tile.recorders = [Recorder(f"detected-{name}", event="detected"), Recorder(f"lost-{name}", event="lost")]
    scene.root.recorders = [Recorder("exit", event="exit"), Recorder("killed-world", event="killed")]
    return scene


def p4(coating=None, pattern=None):
    """A mesh beside the p1 box: the mesh kernels."""
    coating = coating or detector()
    world = _world()
    _box(world, [coating(pattern)])
    gem = Node(name="gem", parent=world, geometry=Mesh.box((2.0, 2.0, 2.0), material=Material(refractive_index=1.5)))
    gem.location = (8.0, 0.0, 0.0)
    gem.recorders = [Recorder("gem-in", event="entering")]
    _lamp(world, (0.5, 0.3, -0.2))
    return Scene(world)


def sphere(coating=None, pattern=None):
    """A sphere of radius 2, n = 1.5, whose coating has facet=None."""
    coating = coating or detector(None)
    world = _world()
    ball = Node(name="box", parent=world, geometry=Sphere(2.0, material=_coated([coating(pattern)])))
    ball.recorders = [Recorder("detected", event="detected"), Recorder("escaping", event="escaping"),
                      Recorder("lost", event="lost")]
    world.recorders = [Recorder("exit", event="exit")]
    _lamp(world, (0.3, 0.2, -0.1))
    return Scene(world)


def tile_patterns(masks=None):
    """p3's two patterns: 5 x 3 x 1 and 7 x 1 x 1 cells over a tile's 5 x 5 top face (cpat_start 0 and 15)."""
    shapes = ((5, 3, 1), (7, 1, 1))
    if masks is None:
        masks = [third_mask(s, seed=11 + i) for i, s in enumerate(shapes)]
    elif isinstance(masks, str):
        masks = [np.full(s, 1 if masks == "ones" else 0, dtype=np.uint8) for s in shapes]
    return tuple(CoatingPattern(m, (-2.5, -2.5, None), (2.5, 2.5, None)) for m in masks)


def volume_pattern(mask=None):
    """The sphere's 4 x 4 x 4 mask, bounded on all three axes (the lattice holds the whole sphere)."""
    if isinstance(mask, str):
        mask = np.full((4, 4, 4), 1 if mask == "ones" else 0, dtype=np.uint8)
    return CoatingPattern(third_mask((4, 4, 4), seed=9) if mask is None else mask, (-2.5, -2.5, -2.5), (2.5, 2.5, 2.5))


def small_pattern(mask=None, shape=(6, 6, 1)):
    """p2's lattice, deliberately smaller than the face: x, y in [-3, 3)."""
    return face_pattern(mask, half=3.0, shape=shape)


# layout -> (builder, pattern maker taking None / "ones" / "zeros", the name(s) of the patterned node(s), the coated facet)
LAYOUTS = {
    "p1": (p1, face_pattern, ("box",), TOP),
    "p2": (p2, small_pattern, ("box",), TOP),
    "p3": (p3, tile_patterns, TILES, TOP),
    "p4": (p4, face_pattern, ("box",), TOP),
}
SPHERE = (sphere, volume_pattern, ("box",), None)


def patterns_of(made):
    return made if isinstance(made, tuple) else (made,)


def local_points(scene, node_name, positions):
    """World positions -> the node's frame by rule 2 of the `Coating` docstring: pos + t on an unrotated node, the row
    products ((R0 x + R1 y) + R2 z) + t otherwise, one IEEE operation after the other (numpy fuses nothing)."""
    compiled = compile_scene(scene)
    m = np.asarray(compiled.world_to_local[compiled.node_names.index(node_name)], dtype=np.float64)
    p = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    if np.array_equal(m[:3, :3], np.eye(3)):
        return p + m[:3, 3]
    out = np.empty_like(p)
    for a in range(3):
        out[:, a] = ((m[a, 0] * p[:, 0] + m[a, 1] * p[:, 1]) + m[a, 2] * p[:, 2]) + m[a, 3]
    return out
