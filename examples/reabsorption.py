"""How often is collected light re-emitted, and which share of the escape-cone loss is first-generation light?

A 5 x 5 x 1 cm Lumogen slab is lit from above.  Each of its four edges carries a recorder of the luminescence that
leaves through it, with two histograms of the photon's event counters: `emissions` (how many times the photon was
re-emitted before it reached the edge) and `emissions` x `reflections` (and how many internal reflections it survived).
The top face carries one more: the luminescence lost through the escape cone, by generation.  The counters describe the
photon as it arrives; they cost no memory that grows with the photon count and no event log.

    python examples/reabsorption.py [photons]
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pvtrace_amd import (   # noqa: E402
    Absorber, Box, Light, Luminophore, Material, Node, Scene, cone, engine, lumogen_f_red_305,
)
from pvtrace_amd.engine import Heatmap, Histogram, Recorder   # noqa: E402

EDGES = {"right": (1, 0, 0), "left": (-1, 0, 0), "far": (0, 1, 0), "near": (0, -1, 0)}
GENERATIONS = 16
BOUNCES = 64


def concentrator():
    x = np.arange(400, 800)
    world = Node(name="world", geometry=Box((100.0, 100.0, 100.0), material=Material(refractive_index=1.0)))
    body = Node(name="slab", parent=world, geometry=Box((5.0, 5.0, 1.0), material=Material(
        refractive_index=1.5, components=[
            Luminophore(coefficient=np.column_stack((x, lumogen_f_red_305.absorption(x) * 10.0)),
                        emission=np.column_stack((x, lumogen_f_red_305.emission(x))), quantum_yield=0.98, name="dye"),
            Absorber(0.02, name="host"),
        ])))
    body.recorders = [Recorder(f"edge-{label}", event="escaping", facet=normal, source="components", histograms=[
        Histogram("emissions", 0, GENERATIONS, GENERATIONS),
        Heatmap("emissions", "reflections", (0, GENERATIONS, GENERATIONS), (0, BOUNCES, BOUNCES))])
        for label, normal in EDGES.items()]
    body.recorders.append(Recorder("top-loss", event="escaping", facet=(0, 0, 1), source="components",
                                   histograms=[Histogram("emissions", 0, GENERATIONS, GENERATIONS)]))
    lamp = Node(name="lamp", parent=world, light=Light(direction=functools.partial(cone, np.radians(20)), name="lamp"))
    lamp.location = (0.0, 0.0, 5.0)
    lamp.rotate(np.radians(180), (1, 0, 0))
    return Scene(world)


def main(photons=200_000, seed=5):
    result = engine.simulate(concentrator(), photons, seed=seed, record_every=0, emit_seed=seed + 1)
    edges = [result.recorders[f"edge-{label}"] for label in EDGES]
    generations = sum(rec.histogram(0)[1] for rec in edges)                 # collected photons by number of emissions
    joint = sum(rec.histogram(1)[2] for rec in edges)                       # ... and by reflections
    collected = int(generations.sum())
    mean_emissions = float(np.dot(np.arange(GENERATIONS), generations)) / collected
    mean_reflections = float(np.dot(np.arange(BOUNCES), joint.sum(axis=0))) / int(joint.sum())
    top = result.recorders["top-loss"].histogram(0)[1]
    first_generation = float(top[1]) / int(top.sum())                       # luminescence arrives with one emission at least
    print(f"photons {photons}: {collected} collected at the edges")
    print(f"mean re-emissions of a collected photon: {mean_emissions - 1.0:.4f} (emissions {mean_emissions:.4f}, "
          f"reflections {mean_reflections:.3f})")
    print(f"top-face loss: {int(top.sum())} photons, first generation {100.0 * first_generation:.2f} %")
    return {"result": result, "collected": collected, "mean_emissions": mean_emissions, "mean_reflections": mean_reflections,
            "first_generation_share": first_generation}


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:2]))
