"""Printed outcoupling dots under a light-guide plate: why the dot density grows away from the lamp.

A 10 x 4 x 0.3 cm acrylic plate is lit through its -x edge.  The light is guided by total internal reflection until it
meets a white dot printed on the bottom face -- a Lambertian reflector, `Coating((0, 0, -1), reflectivity=1.0,
reflection="lambertian", pattern=...)` -- which scatters part of it into the escape cone of the top face.  The dots are
binary geometry: a `CoatingPattern` mask of 200 x 80 cells (0.5 mm) whose cells are set at random with the local dot
density.  With a uniform density the plate is bright near the lamp and dim at the far end; a density that grows as the
guided flux falls evens the top face out.  The outcoupled light is a `Heatmap("x", "y")` on the top face; the uniformity
printed is min / max of its column sums along x.

    python examples/dot_pattern.py [photons]     # on a machine with an MI355X
"""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pvtrace_amd import (   # noqa: E402
    Box, CoatedSurfaceDelegate, Coating, CoatingPattern, Light, Material, Node, Scene, Surface, cone, engine,
    rectangular_mask,
)
from pvtrace_amd.engine import Heatmap, Recorder   # noqa: E402

LENGTH, WIDTH, THICKNESS = 10.0, 4.0, 0.3
CELLS = (200, 80, 1)
COLUMNS = 10
LOSS_PER_CM = 0.06     # share of the guided flux the graded pattern takes out per centimetre of a fully printed face


def density(kind):
    """Dot density (the share of printed cells) along x, one value per mask column."""
    s = (np.arange(CELLS[0]) + 0.5) * LENGTH / CELLS[0]     # distance from the lamp's edge
    if kind == "uniform":
        return np.full(CELLS[0], 0.4)
    # flux F falls as F' = -k p F; p F is constant for p = p0 / (1 - k p0 s)
    return 0.25 / (1.0 - LOSS_PER_CM * s)


def dots(kind, seed=4):
    rng = np.random.default_rng(seed)
    mask = rng.random(CELLS) < density(kind)[:, None, None]
    return CoatingPattern(mask, (-LENGTH / 2, -WIDTH / 2, None), (LENGTH / 2, WIDTH / 2, None))


def build(kind):
    world = Node(name="world", geometry=Box((40.0, 40.0, 40.0), material=Material(refractive_index=1.0)))
    coatings = [Coating((0, 0, -1), reflectivity=1.0, reflection="lambertian", pattern=dots(kind)),
                Coating((1, 0, 0), reflectivity=1.0), Coating((0, 1, 0), reflectivity=1.0), Coating((0, -1, 0), reflectivity=1.0)]
    plate = Node(name="plate", parent=world, geometry=Box((LENGTH, WIDTH, THICKNESS), material=Material(
        refractive_index=1.49, surface=Surface(delegate=CoatedSurfaceDelegate(coatings)))))
    plate.recorders = [Recorder("top", event="escaping", facet=(0, 0, 1), histograms=[
        Heatmap("x", "y", (-LENGTH / 2, LENGTH / 2, COLUMNS), (-WIDTH / 2, WIDTH / 2, 4))])]
    world.recorders = [Recorder("exit", event="exit")]
    # the lamp: a strip just inside the -x edge, shining along +x within 40 degrees of the axis -- all of it guided
    lamp = Node(name="lamp", parent=world, light=Light(
        position=functools.partial(rectangular_mask, 0.4 * THICKNESS, 0.45 * WIDTH),
        direction=functools.partial(cone, np.radians(40.0)), name="lamp"))
    lamp.rotate(np.radians(90.0), (0, 1, 0))
    lamp.location = (-LENGTH / 2 + 0.01, 0.0, 0.0)
    return Scene(world)


def main(photons=500_000):
    out = {}
    for kind in ("uniform", "graded"):
        pattern_coverage = dots(kind).coverage
        result = engine.simulate(build(kind), photons, seed=1, record_every=0)
        top = result.recorders["top"]
        _, _, bins = top.histogram(0)
        columns = np.asarray(bins).reshape(COLUMNS, -1).sum(axis=1)
        uniformity = float(columns.min()) / float(columns.max())
        out[kind] = {"uniformity": uniformity, "outcoupled": int(top.rays), "columns": columns.tolist(),
                     "coverage": pattern_coverage}
        print(f"{kind:8s} dots cover {pattern_coverage:5.3f} of the face; {top.rays} of {photons} photons leave the top; "
              f"columns {columns.tolist()}; uniformity min/max = {uniformity:.3f}")
    return out


if __name__ == "__main__":
    main(int(float(sys.argv[1])) if len(sys.argv) > 1 else 500_000)
