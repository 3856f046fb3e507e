"""Scenes and helpers of the absorbing-coating tests (tests/test_absorbing_coatings.py, tests/test_gpu_absorbing_coatings.py):
pencils onto one coated face whose outcome shares are known in closed form, and the three layouts the kernel serves
differently -- a coated box in a world (<= 16 nodes), a tile array on the node grid with absorbing inner faces, a mesh
beside a coated box."""
import math

import numpy as np

from pvtrace_amd import (
    AbsorptivityTable, Box, Coating, CoatedSurfaceDelegate, Material, Node, ReflectivityTable, Scene, Surface,
)
from pvtrace_amd.engine import Histogram, Recorder
from tests import scenes

TOP = (0.0, 0.0, 1.0)
EDGES = {"right": (1, 0, 0), "left": (-1, 0, 0), "far": (0, 1, 0), "near": (0, -1, 0)}


def five_sigma(count, n, p):
    """|count - n p| <= 5 sqrt(n p (1 - p)): the binomial bound of the law tests (a share of exactly 0 or 1 admits no
    deviation at all)."""
    return abs(count - n * p) <= 5.0 * math.sqrt(n * p * (1.0 - p))


def fresnel_r(theta, n1, n2):
    """Unpolarised Fresnel reflectivity at incidence angle `theta` (radians) going from n1 into n2 (Hecht)."""
    s = n1 / n2 * math.sin(theta)
    if s >= 1.0:
        return 1.0
    c1, c2 = math.cos(theta), math.sqrt(1.0 - s * s)
    rs = ((n1 * c1 - n2 * c2) / (n1 * c1 + n2 * c2)) ** 2
    rp = ((n1 * c2 - n2 * c1) / (n1 * c2 + n2 * c1)) ** 2
    return 0.5 * (rs + rp)


def coated_box(coatings, n_box=1.0, n_world=1.0, size=(10.0, 10.0, 2.0), recorders=True):
    """A box at the origin of a 40 cm world with `coatings` on its surface; recorders that hear each end of a photon once:
    `detected` per coated facet, `exit` on the world, `killed` on both."""
    world = Node(name="world", geometry=Box((40.0, 40.0, 40.0), material=Material(refractive_index=n_world)))
    box = Node(name="box", parent=world, geometry=Box(size, material=Material(
        refractive_index=n_box, surface=Surface(delegate=CoatedSurfaceDelegate(list(coatings))))))
    if recorders:
        box.recorders = [Recorder("detected", event="detected", histograms=[Histogram("angle", 0.0, math.pi / 2, 18)]),
                         Recorder("reflected", event="reflected"), Recorder("entering", event="entering"),
                         Recorder("escaping", event="escaping"), Recorder("killed-box", event="killed")]
        world.recorders = [Recorder("exit", event="exit"), Recorder("killed-world", event="killed")]
    return Scene(world)


def pencil_from_above(theta=0.0, at=(0.0, 0.0)):
    """(position, direction) of a ray that meets the top face (z = 1) of `coated_box` from outside at (at, 1) under the
    angle of incidence `theta`."""
    d = (math.sin(theta), 0.0, -math.cos(theta))
    return (at[0] - d[0], at[1], 1.0 - d[2]), d


def pencil_from_inside(theta, start=(0.0, 0.0, 0.0)):
    """(position, direction) of a ray inside `coated_box` that meets its top face from inside under `theta`."""
    return start, (math.sin(theta), 0.0, math.cos(theta))


def step_table():
    """A(wavelength, angle) with two wavelengths and two angles: clamped outside [500, 600] nm x [20, 60] degrees, so each
    of the four corners beyond them is a band with one value."""
    return AbsorptivityTable([500.0, 600.0], [[0.2, 0.6], [0.4, 0.8]], angle=[20.0, 60.0])


STEP_CELLS = {(450.0, 10.0): 0.2, (650.0, 10.0): 0.6, (450.0, 70.0): 0.4, (650.0, 70.0): 0.8}


def eqe_table(nw=16, na=8, peak=0.9):
    """A smooth EQE(wavelength, angle): high in the red, falling towards grazing incidence."""
    wl = np.linspace(400.0, 800.0, nw)
    ang = np.linspace(0.0, 90.0, na)
    spectral = peak * (0.35 + 0.65 / (1.0 + np.exp(-(wl - 560.0) / 30.0)))
    angular = np.cos(np.radians(ang)) ** 0.25
    return AbsorptivityTable(wl, np.clip(angular[:, None] * spectral[None, :], 0.0, 1.0), angle=ang)


def zero_table():
    """A table that absorbs nothing: the scene still lowers its absorptivity tables and runs the extension variants."""
    return AbsorptivityTable([400.0, 800.0], [[0.0, 0.0], [0.0, 0.0]], angle=[0.0, 90.0])


def _recorders_for(prefix, facets, capture=None):
    return [Recorder(f"{prefix}{label}", event="detected", facet=normal, capture=capture,
                     histograms=[Histogram("wavelength", 400.0, 800.0, 16)]) for label, normal in facets.items()]


# -- (S1) one coated box in the world: the Lumogen slab with cells on its four edges and a mirror underneath ---------------
def s1_slab(absorptivity="table", mirror=True, capture=None, recorders=True):
    """`absorptivity`: "table" (EQE table cells, a 95 % mirror that absorbs the rest), "zero" (tables of zeros), 0.0 (the
    scalar zero) or None (no absorptivity at all: the coatings of the same geometry, R alone)."""
    scene = scenes.lsc_equivalent(recorders=False)
    slab = next(n for n in scene.root.preorder() if n.name == "LSC")
    a_cell = {"table": eqe_table(), "zero": zero_table()}.get(absorptivity, absorptivity)
    a_mirror = {"table": 0.05, "zero": zero_table()}.get(absorptivity, absorptivity)
    coatings = [Coating(normal, reflectivity=0.0, absorptivity=a_cell, transmission="matched") for normal in EDGES.values()]
    if mirror:
        coatings.append(Coating((0, 0, -1), reflectivity=0.95, absorptivity=a_mirror))
    material = slab.geometry.material
    slab.geometry.material = Material(refractive_index=material.refractive_index, components=list(material.components),
                                      surface=Surface(delegate=CoatedSurfaceDelegate(coatings)))
    if recorders:
        slab.recorders = _recorders_for("cell-", EDGES, capture) + [
            Recorder("mirror", event="detected", facet=(0, 0, -1), capture=capture),
            Recorder("lost", event="lost"), Recorder("reacted", event="reacted"), Recorder("killed-slab", event="killed"),
            Recorder("top", event="escaping", facet=(0, 0, 1))]
        scene.root.recorders = [Recorder("exit", event="exit"), Recorder("killed-world", event="killed")]
    return scene


# -- (S2) a 37-node tile array: absorbing coatings on the inner faces between tiles --------------------------------------------
def s2_tiles(absorptivity="table", capture=None):
    from benchmarks.configs import tiles_lsc

    scene = tiles_lsc(6, recorders=None)
    a = {"table": eqe_table(8, 4, 0.8), "zero": zero_table()}.get(absorptivity, absorptivity)
    tiles = [n for n in scene.root.preorder() if n is not scene.root and n.geometry is not None]
    assert len(tiles) == 36
    xs = sorted({round(float(n.location[0]), 9) for n in tiles})
    ys = sorted({round(float(n.location[1]), 9) for n in tiles})
    for n in tiles:
        x, y = round(float(n.location[0]), 9), round(float(n.location[1]), 9)
        inner = {label: normal for label, normal in EDGES.items()
                 if not ((label == "right" and x == xs[-1]) or (label == "left" and x == xs[0])
                         or (label == "far" and y == ys[-1]) or (label == "near" and y == ys[0]))}
        material = n.geometry.material
        coatings = [Coating(normal, reflectivity=0.0, absorptivity=a, transmission="matched") for normal in inner.values()]
        n.geometry.material = Material(refractive_index=material.refractive_index, components=list(material.components),
                                       surface=Surface(delegate=CoatedSurfaceDelegate(coatings)))
        n.recorders = [Recorder(f"cells-{n.name}", event="detected", capture=capture),
                       Recorder(f"lost-{n.name}", event="lost"), Recorder(f"killed-{n.name}", event="killed")]
    scene.root.recorders = [Recorder("exit", event="exit"), Recorder("killed-world", event="killed")]
    return scene


# -- (S3) a mesh node with a coated box beside it ---------------------------------------------------------------------------------
def s3_mesh(absorptivity="table", capture=None):
    scene = scenes.mesh_lsc()
    world = scene.root
    slab = next(n for n in world.preorder() if n.name == "LSC")
    slab.recorders = [Recorder("lost", event="lost"), Recorder("killed-slab", event="killed")]
    a = {"table": eqe_table(8, 4, 0.55), "zero": zero_table()}.get(absorptivity, absorptivity)   # (R up to 0.4 beside it)
    coatings = [Coating((-1, 0, 0), reflectivity=0.1, absorptivity=a),
                Coating((0, 0, 1), reflectivity=ReflectivityTable([400.0, 800.0], [0.2, 0.4]), absorptivity=a)]
    panel = Node(name="panel", parent=world, geometry=Box((1.0, 6.0, 3.0), material=Material(
        refractive_index=1.5, surface=Surface(delegate=CoatedSurfaceDelegate(coatings)))))
    panel.location = (3.2, 0.0, 0.0)
    panel.recorders = [Recorder("panel-left", event="detected", facet=(-1, 0, 0), capture=capture),
                       Recorder("panel-any", event="detected", capture=capture), Recorder("killed-panel", event="killed")]
    world.recorders = [Recorder("exit", event="exit"), Recorder("killed-world", event="killed")]
    return scene


LAYOUTS = {"s1": s1_slab, "s2": s2_tiles, "s3": s3_mesh}
