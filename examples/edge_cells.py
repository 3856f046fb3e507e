"""Solar cells on two edges of a luminescent slab and a real mirror underneath: where do the photons end?

A hand-built 5 x 5 x 1 cm Lumogen F Red slab.  The cells on the +x and -x edges are absorbing coatings with a tabulated
EQE(wavelength, angle) -- the probability that a photon ARRIVING at the cell is collected -- bonded to the glass
(`reflectivity=0.0, transmission="matched"`); what a cell does not collect passes on into the world.  The mirror under
the slab reflects 95 % and absorbs the other 5 %, as evaporated aluminium does, instead of leaking it through the metal.
`detected` recorders count what each coating absorbed; the rest of the photons are lost in the slab or escape.

    python examples/edge_cells.py [photons]     # on a machine with an MI355X
"""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pvtrace_amd import (   # noqa: E402
    Absorber, AbsorptivityTable, Box, CoatedSurfaceDelegate, Coating, Light, Luminophore, Material, Node, Scene, Surface,
    cone, engine,
)
from pvtrace_amd.data import lumogen_f_red_305   # noqa: E402
from pvtrace_amd.engine import Histogram, Recorder   # noqa: E402

CELLS = {"right": (1, 0, 0), "left": (-1, 0, 0)}


def eqe_table():
    """A silicon-like EQE: high in the red, falling towards grazing incidence."""
    wl, ang = np.linspace(400.0, 800.0, 41), np.linspace(0.0, 90.0, 10)
    spectral = 0.92 * (0.4 + 0.6 / (1.0 + np.exp(-(wl - 560.0) / 30.0)))
    return AbsorptivityTable(wl, np.cos(np.radians(ang))[:, None] ** 0.25 * spectral[None, :], angle=ang)


def build():
    x = np.arange(400, 800)
    world = Node(name="world", geometry=Box((50.0, 50.0, 50.0), material=Material(refractive_index=1.0)))
    eqe = eqe_table()
    coatings = [Coating(normal, reflectivity=0.0, absorptivity=eqe, transmission="matched") for normal in CELLS.values()]
    coatings.append(Coating((0, 0, -1), reflectivity=0.95, absorptivity=0.05))
    slab = Node(name="slab", parent=world, geometry=Box((5.0, 5.0, 1.0), material=Material(
        refractive_index=1.5,
        components=[Luminophore(coefficient=np.column_stack((x, lumogen_f_red_305.absorption(x) * 10.0)),
                                emission=np.column_stack((x, lumogen_f_red_305.emission(x))), quantum_yield=0.98,
                                name="Lumogen F Red 305"),
                    Absorber(0.02, name="host")],
        surface=Surface(delegate=CoatedSurfaceDelegate(coatings)))))
    slab.recorders = [Recorder(f"cell-{label}", event="detected", facet=normal,
                               histograms=[Histogram("wavelength", 400.0, 800.0, 40)]) for label, normal in CELLS.items()]
    slab.recorders += [Recorder("mirror", event="detected", facet=(0, 0, -1)), Recorder("lost", event="lost"),
                       Recorder("killed-slab", event="killed")]
    world.recorders = [Recorder("escaped", event="exit"), Recorder("killed-world", event="killed")]
    light = Node(name="sun", parent=world, light=Light(direction=functools.partial(cone, np.radians(20)), name="sun"))
    light.location = (0.0, 0.0, 5.0)
    light.rotate(np.radians(180), (1, 0, 0))
    return Scene(world)


def main(photons=1_000_000):
    result = engine.simulate(build(), photons, seed=1, record_every=0)
    rec = result.recorders
    counts = {"detected": sum(rec[f"cell-{label}"].rays for label in CELLS), "mirror": rec["mirror"].rays,
              "lost": rec["lost"].rays, "escaped": rec["escaped"].rays,
              "killed": rec["killed-slab"].rays + rec["killed-world"].rays}
    shares = {name: count / photons for name, count in counts.items()}
    print(f"{photons} photons")
    for name, share in shares.items():
        print(f"  {name:9s} {share:8.4f}")
    for label in CELLS:
        print(f"  cell-{label}: {rec[f'cell-{label}'].rays} photons, mean wavelength {rec[f'cell-{label}'].mean('wavelength'):.1f} nm")
    return {"photons": photons, "shares": shares, "recorders": rec}


if __name__ == "__main__":
    main(int(float(sys.argv[1])) if len(sys.argv) > 1 else 1_000_000)
