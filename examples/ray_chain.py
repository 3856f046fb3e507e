"""Two scenes chained by captured rays: the light leaving one edge of an LSC is traced on through a coupling optic.

Stage one lights a 5 x 5 x 1 cm Lumogen slab from above; the recorder on its +x edge is made with `capture=...`, so the
result holds the rays behind its count -- position, direction and wavelength of every photon that left through that
edge.  Stage two is another scene in the same coordinates: a glass prism butted against that edge and a cell behind it.
The captured rays are its input bundle, traced with the table-level entry `_kernel.trace_bundle`.  Prints how many of the
edge's photons reach the cell.

    python examples/ray_chain.py [photons]
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pvtrace_amd import (   # noqa: E402
    Absorber, Box, Light, Luminophore, Material, Node, Scene, cone, engine, lumogen_f_red_305,
)
from pvtrace_amd.engine import Recorder, _kernel, compile_scene   # noqa: E402


def concentrator(capacity):
    x = np.arange(400, 800)
    world = Node(name="world", geometry=Box((100.0, 100.0, 100.0), material=Material(refractive_index=1.0)))
    body = Node(name="slab", parent=world, geometry=Box((5.0, 5.0, 1.0), material=Material(
        refractive_index=1.5, components=[
            Luminophore(coefficient=np.column_stack((x, lumogen_f_red_305.absorption(x) * 10.0)),
                        emission=np.column_stack((x, lumogen_f_red_305.emission(x))), quantum_yield=0.98, name="dye"),
            Absorber(0.02, name="host"),
        ])))
    body.recorders = [Recorder("edge", event="escaping", facet=(1, 0, 0), capture=capacity)]
    lamp = Node(name="lamp", parent=world, light=Light(direction=functools.partial(cone, np.radians(20)), name="lamp"))
    lamp.location = (0.0, 0.0, 5.0)
    lamp.rotate(np.radians(180), (1, 0, 0))
    return Scene(world)


def coupler():
    """A 1 cm glass block from x = 2.5 (the slab's edge) to 3.5 and a cell, a thin absorbing plate, behind it."""
    world = Node(name="world", geometry=Box((100.0, 100.0, 100.0), material=Material(refractive_index=1.0)))
    optic = Node(name="optic", parent=world, geometry=Box((1.0, 5.0, 1.0), material=Material(refractive_index=1.5)))
    optic.location = (3.0 + 1e-6, 0.0, 0.0)
    cell = Node(name="cell", parent=world, geometry=Box((0.05, 5.0, 1.0), material=Material(
        refractive_index=1.5, components=[Absorber(1e3, name="silicon")])))
    cell.location = (3.525 + 2e-6, 0.0, 0.0)
    cell.recorders = [Recorder("cell", event="lost")]
    world.recorders = [Recorder("missed", event="exit")]
    return Scene(world)


def main(photons=200_000, seed=5):
    first = engine.simulate(concentrator(photons), photons, seed=seed, record_every=0, emit_seed=seed + 1)
    edge = first.captures["edge"]
    compiled = compile_scene(coupler())
    rays = (edge.position, edge.direction, edge.wavelength)
    second = _kernel.trace_bundle(compiled, *rays, seed + 2, 1000, 16, 0, 1, 0)
    tallies = dict(zip(compiled.recorder_names, (int(v) for v in second["rec_distinct"])))
    print(f"photons {photons}: {first.recorders['edge'].rays} leave the +x edge ({len(edge)} rows captured, {edge.dropped} dropped)")
    print(f"second stage: {tallies['cell']} absorbed in the cell, {tallies['missed']} leave the scene")
    return {"captured": edge, "second_stage_input": rays, "cell": tallies["cell"], "missed": tallies["missed"]}


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:2]))
