"""Photobleaching loop: concentration field in -> absorbed-photon map out -> new field in, all on the GPU.

A 5 x 5 x 1 cm Lumogen slab whose dye carries a `ConcentrationGrid` is lit by a 20-degree cone from above.  The dye's
`absorbed` `VolumeMap`, made on the grid's own lattice with `VolumeMap.like`, says where photons were absorbed; the dye
is then bleached in proportion to that dose and the slab is traced again.  Prints the photons leaving through the four
edges before and after, and the absorption in the cells that were bleached most.

    python examples/photobleach.py [photons]
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pvtrace_amd import (   # noqa: E402
    Absorber, Box, ConcentrationGrid, Light, Luminophore, Material, Node, Scene, VolumeMap, cone, engine,
    lumogen_f_red_305,
)
from pvtrace_amd.engine import Recorder   # noqa: E402

SHAPE, LOWER, UPPER = (16, 16, 4), (-2.5, -2.5, -0.5), (2.5, 2.5, 0.5)
EDGES = {"left": (-1, 0, 0), "right": (1, 0, 0), "near": (0, -1, 0), "far": (0, 1, 0)}


def slab(concentration):
    """The scene with the dye at relative concentration `concentration` (an array on the lattice)."""
    grid = ConcentrationGrid(concentration, LOWER, UPPER)
    x = np.arange(400, 800)
    world = Node(name="world", geometry=Box((100.0, 100.0, 100.0), material=Material(refractive_index=1.0)))
    body = Node(name="slab", parent=world, geometry=Box((5.0, 5.0, 1.0), material=Material(
        refractive_index=1.5, components=[
            Luminophore(coefficient=np.column_stack((x, lumogen_f_red_305.absorption(x) * 10.0)),
                        emission=np.column_stack((x, lumogen_f_red_305.emission(x))), quantum_yield=0.98,
                        name="dye", concentration=grid),
            Absorber(0.02, name="host"),
        ])))
    body.recorders = [Recorder(f"edge-{name}", event="escaping", facet=facet) for name, facet in EDGES.items()]
    body.volume_maps = [VolumeMap.like(grid, "dose", event="absorbed", component="dye")]
    lamp = Node(name="lamp", parent=world, light=Light(direction=functools.partial(cone, np.radians(20)), name="lamp"))
    lamp.location = (0.0, 0.0, 5.0)
    lamp.rotate(np.radians(180), (1, 0, 0))
    return Scene(world)


def trace(concentration, photons, seed):
    result = engine.simulate(slab(concentration), photons, seed=seed, record_every=0, emit_seed=seed + 1)
    edge = sum(result.recorders[f"edge-{name}"].rays for name in EDGES)
    return edge, result.volume_maps["dose"]


def main(photons=200_000, seed=5, depth=0.8):
    fresh = np.ones(SHAPE)
    edge_before, dose = trace(fresh, photons, seed)
    # bleach in proportion to the absorbed dose: the most exposed cell loses `depth` of its dye
    bleached = fresh * (1.0 - depth * dose.counts / dose.counts.max())
    edge_after, dose_after = trace(bleached, photons, seed)
    worst = dose.counts >= 0.5 * dose.counts.max()
    print(f"photons {photons}: absorbed by the dye {dose.total} -> {dose_after.total}")
    print(f"in the {int(worst.sum())} most exposed cells: {int(dose.counts[worst].sum())} -> {int(dose_after.counts[worst].sum())}")
    print(f"edge output: {edge_before} -> {edge_after}")
    return {"edge_before": int(edge_before), "edge_after": int(edge_after), "dose_before": dose, "dose_after": dose_after,
            "worst": worst}


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:2]))
