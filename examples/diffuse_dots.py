"""Diffusely transmitting dots on a light-guide plate: the other half of examples/dot_pattern.py.

A 10 x 4 x 0.3 cm acrylic plate is lit through its -x edge, every ray guided by total internal reflection.  Dots are
printed on the TOP face.  A dot that transmits diffusely -- `Coating((0, 0, 1), reflectivity=0.2,
transmission=ScatterLobe.lambertian(), pattern=...)`, a cosine lobe about the outgoing normal -- lets guided light out
beyond the critical angle: under the rule of a scattering coating a transmission lobe about "normal" behaves as
"matched" there, so the coating's own R applies and the transmitted photon leaves into the lobe.  Its twin, the same
dots with `transmission="fresnel"`, has no refracted ray to offer beyond the critical angle: R stays 1 and nothing at
all leaves through the top.  The extracted share -- photons leaving the top face over photons launched -- is printed
against the dots' coverage, as a table with a bar per row.

    python examples/diffuse_dots.py [photons]     # on a machine with an MI355X
"""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pvtrace_amd import (   # noqa: E402
    Box, CoatedSurfaceDelegate, Coating, CoatingPattern, Light, Material, Node, ScatterLobe, Scene, Surface, cone, engine,
    rectangular_mask,
)
from pvtrace_amd.engine import Recorder   # noqa: E402

LENGTH, WIDTH, THICKNESS = 10.0, 4.0, 0.3
CELLS = (200, 80, 1)


def dots(coverage, seed=4):
    mask = np.random.default_rng(seed).random(CELLS) < coverage
    return CoatingPattern(mask, (-LENGTH / 2, -WIDTH / 2, None), (LENGTH / 2, WIDTH / 2, None))


def build(coverage, diffuse=True):
    world = Node(name="world", geometry=Box((40.0, 40.0, 40.0), material=Material(refractive_index=1.0)))
    transmission = ScatterLobe.lambertian() if diffuse else "fresnel"
    coatings = [Coating((0, 0, 1), reflectivity=0.2, transmission=transmission, pattern=dots(coverage)),
                Coating((1, 0, 0), reflectivity=1.0), Coating((0, 1, 0), reflectivity=1.0), Coating((0, -1, 0), reflectivity=1.0)]
    plate = Node(name="plate", parent=world, geometry=Box((LENGTH, WIDTH, THICKNESS), material=Material(
        refractive_index=1.49, surface=Surface(delegate=CoatedSurfaceDelegate(coatings)))))
    plate.recorders = [Recorder("top", event="escaping", facet=(0, 0, 1))]
    world.recorders = [Recorder("exit", event="exit")]
    # the lamp: a strip just inside the -x edge, shining along +x within 40 degrees of the axis -- all of it guided
    lamp = Node(name="lamp", parent=world, light=Light(
        position=functools.partial(rectangular_mask, 0.4 * THICKNESS, 0.45 * WIDTH),
        direction=functools.partial(cone, np.radians(40.0)), name="lamp"))
    lamp.rotate(np.radians(90.0), (0, 1, 0))
    lamp.location = (-LENGTH / 2 + 0.01, 0.0, 0.0)
    return Scene(world)


def main(photons=200_000, coverages=(0.05, 0.1, 0.2, 0.4, 0.8)):
    out = {"coverage": list(coverages), "diffuse": [], "specular": []}
    for coverage in coverages:
        shares = []
        for diffuse in (True, False):
            result = engine.simulate(build(coverage, diffuse), photons, seed=1, record_every=0)
            shares.append(result.recorders["top"].rays / photons)
        out["diffuse"].append(shares[0])
        out["specular"].append(shares[1])
        print(f"coverage {coverage:4.2f}: diffuse dots extract {shares[0]:6.4f} {'#' * int(round(60 * shares[0])):60s} "
              f"specular twin {shares[1]:6.4f}")
    return out


if __name__ == "__main__":
    main(int(float(sys.argv[1])) if len(sys.argv) > 1 else 200_000)
