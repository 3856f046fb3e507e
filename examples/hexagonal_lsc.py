"""A square and a hexagonal luminescent concentrator of equal area and thickness: which collects more at its edges?

Two Lumogen F Red plates, 1 cm thick, 25 cm^2 of top face: a 5 x 5 cm square and a regular hexagon.  Every edge face
carries a perfect cell bonded to the glass (`absorptivity=1.0`, `reflectivity=0.0`) and a `detected` recorder named by
`facet=facet_normal(k)`, exactly as the faces of a box are named by their axis normals.  The hexagon is a `Polyhedron`
(a table of eight planes traced analytically), and so is the square here (`Polyhedron.box`), so that both plates run the
same kernel; a `Box` gives the square the same collected fraction within the statistics.

    python examples/hexagonal_lsc.py [photons]     # on a machine with an MI355X
"""
import functools
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pvtrace_amd import (   # noqa: E402
    Absorber, Box, CoatedSurfaceDelegate, Coating, Light, Luminophore, Material, Node, Polyhedron, Scene, Surface, cone, engine,
)
from pvtrace_amd.data import lumogen_f_red_305   # noqa: E402
from pvtrace_amd.engine import Recorder   # noqa: E402

AREA, THICKNESS = 25.0, 1.0


def plates():
    side = math.sqrt(AREA)
    circumradius = math.sqrt(2.0 * AREA / (3.0 * math.sqrt(3.0)))   # a regular hexagon of area A: A = 3 sqrt(3) R^2 / 2
    return {"square": Polyhedron.box((side, side, THICKNESS)), "hexagon": Polyhedron.regular_prism(6, circumradius, THICKNESS)}


def build(plate):
    """The plate in air under a lamp; a cell and a `detected` recorder on every face whose normal lies in the xy plane."""
    x = np.arange(400, 800)
    world = Node(name="world", geometry=Box((50.0, 50.0, 50.0), material=Material(refractive_index=1.0)))
    edges = [k for k in range(len(plate.planes)) if plate.facet_normal(k)[2] == 0.0]
    coatings = [Coating(plate.facet_normal(k), reflectivity=0.0, absorptivity=1.0, transmission="matched") for k in edges]
    plate.material = Material(
        refractive_index=1.5,
        components=[Luminophore(coefficient=np.column_stack((x, lumogen_f_red_305.absorption(x) * 10.0)),
                                emission=np.column_stack((x, lumogen_f_red_305.emission(x))), quantum_yield=0.98,
                                name="Lumogen F Red 305"),
                    Absorber(0.02, name="host")],
        surface=Surface(delegate=CoatedSurfaceDelegate(coatings)))
    node = Node(name="plate", parent=world, geometry=plate)
    node.recorders = [Recorder(f"edge-{k}", event="detected", facet=plate.facet_normal(k)) for k in edges]
    node.recorders += [Recorder("entering", event="entering"), Recorder("lost", event="lost")]
    light = Node(name="sun", parent=world, light=Light(direction=functools.partial(cone, np.radians(10)), name="sun"))
    light.location = (0.0, 0.0, 5.0)
    light.rotate(np.radians(180), (1, 0, 0))
    return Scene(world), edges


def main(photons=200_000, seed=1):
    rows = {}
    for name, plate in plates().items():
        scene, edges = build(plate)
        rec = engine.simulate(scene, photons, seed=seed, record_every=0).recorders
        per_edge = [rec[f"edge-{k}"].rays for k in edges]
        rows[name] = {"edges": len(edges), "entered": rec["entering"].rays, "per_edge": per_edge,
                      "collected": sum(per_edge) / photons, "lost": rec["lost"].rays / photons,
                      "area": plate.volume / THICKNESS, "edge_area": plate.surface_area - 2.0 * plate.volume / THICKNESS}
        print(f"{name:8s} top face {rows[name]['area']:6.2f} cm^2, {len(edges)} edges of {rows[name]['edge_area']:5.2f} cm^2 in all: "
              f"collected {rows[name]['collected']:6.4f}, lost in the plate {rows[name]['lost']:6.4f}; per edge "
              + " ".join(f"{n / photons:.4f}" for n in per_edge))
    return rows


if __name__ == "__main__":
    main(int(float(sys.argv[1])) if len(sys.argv) > 1 else 200_000)
