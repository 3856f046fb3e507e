"""An LSC under structured illumination, emitted on the GPU: a half-shaded image source with an LED-like direction table.

A 5 x 5 x 1 cm Lumogen slab is lit from above by a lamp whose position delegate is a `PositionGrid` -- an image over the
face, one half of it shaded -- and whose direction delegate is a `DirectionTable`, a 15-degree Gaussian lobe about
the lamp's axis.  Both are tables the device emitter samples, so the session keeps `emission == "device"`.

  1. eta(x, y): the `origin_x` x `origin_y` heatmap of the edge recorders over that of the terminal recorders, the
     collection efficiency per cell of the face, where the image puts light.
  2. a two-stage chain: the `absorbed` `VolumeMap` of the slab becomes, through `PositionGrid.like`, the emitter of a
     second scene -- an isotropic glow inside the same slab where the first scene absorbed -- and the share of that
     glow that reaches the edges is printed.

    python examples/shaded_lsc.py [photons]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pvtrace_amd import (   # noqa: E402
    Absorber, Box, DirectionTable, Light, Luminophore, Material, Node, PositionGrid, ScatterLobe, Scene, VolumeMap, isotropic,
    lumogen_f_red_305,
)
from pvtrace_amd.engine import Heatmap, Recorder, Session   # noqa: E402
from pvtrace_amd.light import ConstantWavelengthMask   # noqa: E402

EDGES = {"right": (1, 0, 0), "left": (-1, 0, 0), "far": (0, 1, 0), "near": (0, -1, 0)}
TERMINAL = ("exit", "lost-slab", "killed-slab", "lost-world", "killed-world")
HALF, MAP = 2.5, 8
SHAPE, LOWER, UPPER = (10, 10, 4), (-HALF, -HALF, -0.5), (HALF, HALF, 0.5)


def origin_map():
    return [Heatmap("origin_x", "origin_y", (-HALF, HALF, MAP), (-HALF, HALF, MAP))]


def slab_world(maps=False):
    x = np.arange(400, 800)
    world = Node(name="world", geometry=Box((100.0, 100.0, 100.0), material=Material(refractive_index=1.0)))
    body = Node(name="slab", parent=world, geometry=Box((2 * HALF, 2 * HALF, 1.0), material=Material(
        refractive_index=1.5, components=[
            Luminophore(coefficient=np.column_stack((x, lumogen_f_red_305.absorption(x) * 10.0)),
                        emission=np.column_stack((x, lumogen_f_red_305.emission(x))), quantum_yield=0.98, name="dye"),
            Absorber(0.02, name="host"),
        ])))
    body.recorders = [Recorder(f"edge-{label}", event="escaping", facet=normal, histograms=origin_map())
                      for label, normal in EDGES.items()]
    body.recorders += [Recorder("lost-slab", event="lost", histograms=origin_map()),
                       Recorder("killed-slab", event="killed", histograms=origin_map())]
    world.recorders = [Recorder("exit", event="exit", histograms=origin_map()),
                       Recorder("lost-world", event="lost", histograms=origin_map()),
                       Recorder("killed-world", event="killed", histograms=origin_map())]
    if maps:
        body.volume_maps = [VolumeMap("absorbed", SHAPE, LOWER, UPPER, event="absorbed")]
    return world, body


def shaded_scene():
    """Stage one: the image lamp above the face."""
    world, _ = slab_world(maps=True)
    cells = 64
    u = (np.arange(cells) + 0.5) / cells - 0.5
    image = np.exp(-0.5 * (u[:, None] ** 2 + u[None, :] ** 2) / 0.35 ** 2)      # a broad beam profile ...
    image[: cells // 2, :] = 0.0                                                # ... one half of the aperture shaded
    lamp = Node(name="lamp", parent=world, light=Light(
        position=PositionGrid(image, (-HALF, -HALF, None), (HALF, HALF, None)),
        direction=DirectionTable(ScatterLobe.gaussian(15.0, "normal").table), name="lamp"))
    lamp.location = (0.0, 0.0, 5.0)
    lamp.rotate(np.radians(180), (1, 0, 0))
    return Scene(world)


def glow_scene(absorbed):
    """Stage two: an isotropic 620 nm glow inside the slab, distributed as stage one's absorbed map."""
    world, _ = slab_world()        # (the slab sits at the origin unrotated: its frame, the map's, is the world's)
    Node(name="glow", parent=world, light=Light(wavelength=ConstantWavelengthMask(620.0), position=PositionGrid.like(absorbed),
                                                direction=isotropic, name="glow"))
    return Scene(world)


def run(scene, photons, seed):
    with Session(scene) as session:
        assert session.emission == "device"          # both stages are sampled on the GPU
        return session.collect(session.submit(photons, seed, record_every=0, emit_seed=seed + 1))


def edge_share(result):
    return sum(result.recorders[f"edge-{label}"].rays for label in EDGES) / sum(result.recorders[n].rays for n in TERMINAL)


def main(photons=400_000, seed=5):
    first = run(shaded_scene(), photons, seed)
    recs = first.recorders
    collected = sum(np.asarray(recs[f"edge-{label}"].histogram(0)[2]) for label in EDGES).reshape(MAP, MAP)
    launched = sum(np.asarray(recs[name].histogram(0)[2]) for name in TERMINAL).reshape(MAP, MAP)
    eta = np.full((MAP, MAP), np.nan)
    eta[launched > 0] = collected[launched > 0] / launched[launched > 0]
    print(f"photons {photons}: {int(launched.sum())} launched from {int((launched > 0).sum())} of {MAP * MAP} cells of the face")
    print(f"collection efficiency eta(x, y), {MAP} x {MAP} cells (rows: x, columns: y; -- = shaded):")
    for row in eta:
        print(" ".join("  -- " if np.isnan(v) else f"{v:.3f}" for v in row))
    absorbed = first.volume_maps["absorbed"]
    print(f"stage one: {edge_share(first):.4f} of the photons reach an edge, {absorbed.total} absorptions mapped")
    second = run(glow_scene(absorbed), photons, seed + 2)
    print(f"stage two: {edge_share(second):.4f} of a 620 nm glow distributed as that map reach an edge")
    return {"eta": eta, "launched": launched, "absorbed": absorbed, "first": first, "second": second}


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:2]))
