"""How much diffuse light does a tapered light guide deliver to its small face?

A PMMA taper -- a truncated cone, `Frustum(length, radius_bottom, radius_top)`, traced analytically -- is lit on its large
face by a Lambertian disc of the face's size.  `escaping` recorders on the two caps (`facet=(0, 0, +-1)`) count what
leaves through the small exit face and what comes back out of the entrance; an un-faceted one counts every escape, so the
slanted wall's share is the rest.  Conservation of etendue bounds the delivered fraction of light that is inside the
guide by (r_exit / r_entrance)^2 n^2 for an exit into air; steeper tapers turn more of it around.

    python examples/tapered_guide.py [photons]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pvtrace_amd import Absorber, Box, Frustum, Light, Material, Node, Scene, engine, lambertian   # noqa: E402
from pvtrace_amd.engine import Recorder   # noqa: E402
from pvtrace_amd.light import CircularMask   # noqa: E402

LENGTH, ENTRANCE = 10.0, 1.0
RATIOS = (1.0, 1.5, 2.0, 3.0, 4.0)


def guide(ratio):
    world = Node(name="world", geometry=Box((100.0, 100.0, 100.0), material=Material(refractive_index=1.0)))
    taper = Node(name="taper", parent=world, geometry=Frustum(LENGTH, ENTRANCE, ENTRANCE / ratio, material=Material(
        refractive_index=1.49, components=[Absorber(0.002, name="PMMA")])))
    taper.recorders = [Recorder("exit-face", event="escaping", facet=(0, 0, 1)),
                       Recorder("entrance-face", event="escaping", facet=(0, 0, -1)),
                       Recorder("escaping", event="escaping"), Recorder("entering", event="entering"),
                       Recorder("lost", event="lost")]
    lamp = Node(name="lamp", parent=world, light=Light(position=CircularMask(ENTRANCE), direction=lambertian, name="lamp"))
    lamp.location = (0.0, 0.0, -0.5 * LENGTH - 0.01)
    return Scene(world)


def main(photons=200_000, seed=3):
    rows = []
    for ratio in RATIOS:
        rec = engine.simulate(guide(ratio), photons, seed=seed, record_every=0, emit_seed=seed + 1).recorders
        entered = rec["entering"].rays
        exit_face, entrance, every = rec["exit-face"].rays, rec["entrance-face"].rays, rec["escaping"].rays
        rows.append({"ratio": ratio, "entered": entered, "collected": exit_face / photons, "returned": entrance / photons,
                     "wall": (every - exit_face - entrance) / photons, "lost": rec["lost"].rays / photons})
        print(f"taper {ratio:3.1f}:1  entered {entered / photons:6.3f}  exit face {rows[-1]['collected']:6.3f}  "
              f"back out of the entrance {rows[-1]['returned']:6.3f}  through the wall {rows[-1]['wall']:6.3f}  "
              f"absorbed {rows[-1]['lost']:6.3f}")
    return rows


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:2]))
