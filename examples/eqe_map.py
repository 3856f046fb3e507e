"""EQE(lambda) and the collection-efficiency map eta(x, y) of a concentrator, from ONE launch.

A 5 x 5 x 1 cm Lumogen slab is lit from above by an area light that covers its face, with a broad spectrum.  Each of its
four edges carries a recorder of the light that leaves through it, with two histograms of the photon AS IT WAS LAUNCHED:
`origin_wavelength` (the wavelength the lamp gave it, not the re-emitted one the edge sees) and `origin_x` x `origin_y`
(where on the face it started).  The same two histograms on the terminal recorders -- `exit` on the world, `lost` and
`killed` in the slab and the world: every photon ends in exactly one of them -- count the photons launched per bin, the
denominators:

    EQE(lambda) = collected at the edges / launched, per launch-wavelength bin
    eta(x, y)   = the same per cell of the face

The histograms cost no memory that grows with the photon count, no event log and no capture.

    python examples/eqe_map.py [photons]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pvtrace_amd import (   # noqa: E402
    Absorber, Box, Distribution, Light, Luminophore, Material, Node, Scene, engine, lumogen_f_red_305,
)
from pvtrace_amd.engine import Heatmap, Histogram, Recorder   # noqa: E402
from pvtrace_amd.light import RectangularMask, SpectrumWavelengthMask   # noqa: E402

EDGES = {"right": (1, 0, 0), "left": (-1, 0, 0), "far": (0, 1, 0), "near": (0, -1, 0)}
TERMINAL = ("exit", "lost-slab", "killed-slab", "lost-world", "killed-world")
BAND = (400.0, 700.0, 30)     # launch wavelengths, 10 nm bins
HALF = 2.5                    # the face is 2 HALF x 2 HALF
MAP = 8


def origin_histograms():
    return [Histogram("origin_wavelength", *BAND),
            Heatmap("origin_x", "origin_y", (-HALF, HALF, MAP), (-HALF, HALF, MAP))]


def concentrator():
    x = np.arange(400, 800)
    world = Node(name="world", geometry=Box((100.0, 100.0, 100.0), material=Material(refractive_index=1.0)))
    body = Node(name="slab", parent=world, geometry=Box((2 * HALF, 2 * HALF, 1.0), material=Material(
        refractive_index=1.5, components=[
            Luminophore(coefficient=np.column_stack((x, lumogen_f_red_305.absorption(x) * 10.0)),
                        emission=np.column_stack((x, lumogen_f_red_305.emission(x))), quantum_yield=0.98, name="dye"),
            Absorber(0.02, name="host"),
        ])))
    body.recorders = [Recorder(f"edge-{label}", event="escaping", facet=normal, histograms=origin_histograms())
                      for label, normal in EDGES.items()]
    body.recorders += [Recorder("lost-slab", event="lost", histograms=origin_histograms()),
                       Recorder("killed-slab", event="killed", histograms=origin_histograms())]
    world.recorders = [Recorder("exit", event="exit", histograms=origin_histograms()),
                       Recorder("lost-world", event="lost", histograms=origin_histograms()),
                       Recorder("killed-world", event="killed", histograms=origin_histograms())]
    lam = np.linspace(BAND[0], BAND[1], 31)
    lamp = Node(name="lamp", parent=world, light=Light(
        wavelength=SpectrumWavelengthMask(Distribution(lam, np.exp(-((lam - 550.0) / 150.0) ** 2))),
        position=RectangularMask(HALF, HALF), name="lamp"))
    lamp.location = (0.0, 0.0, 5.0)
    lamp.rotate(np.radians(180), (1, 0, 0))
    return Scene(world)


def main(photons=400_000, seed=5):
    result = engine.simulate(concentrator(), photons, seed=seed, record_every=0, emit_seed=seed + 1)
    recs = result.recorders
    collected = sum(np.asarray(recs[f"edge-{label}"].histogram(0)[1]) for label in EDGES)
    launched = sum(np.asarray(recs[name].histogram(0)[1]) for name in TERMINAL)
    wavelengths = BAND[0] + (np.arange(BAND[2]) + 0.5) * (BAND[1] - BAND[0]) / BAND[2]
    eqe = np.full(BAND[2], np.nan)
    eqe[launched > 0] = collected[launched > 0] / launched[launched > 0]
    print(f"photons {photons}: {int(launched.sum())} binned by launch wavelength, {int(collected.sum())} collected at the edges")
    for k in np.flatnonzero(launched > 0):
        print(f"{wavelengths[k]:6.1f} nm  EQE {eqe[k]:.4f}  ({int(collected[k])} of {int(launched[k])})")
    eta_collected = sum(np.asarray(recs[f"edge-{label}"].histogram(1)[2]) for label in EDGES).reshape(MAP, MAP)
    eta_launched = sum(np.asarray(recs[name].histogram(1)[2]) for name in TERMINAL).reshape(MAP, MAP)
    eta = eta_collected / eta_launched
    print(f"collection efficiency eta(x, y), {MAP} x {MAP} cells of the face (rows: x, columns: y):")
    for row in eta:
        print(" ".join(f"{v:.3f}" for v in row))
    total = float(collected.sum()) / photons
    print(f"overall: {total:.4f} of the launched photons reach an edge")
    return {"result": result, "wavelengths": wavelengths, "eqe": eqe, "eta": eta, "total": total}


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:2]))
