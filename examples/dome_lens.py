"""How much of an isotropic emitter's light does a dome over it let out?

An emitter sits at the centre of the base of a clear encapsulant of index 1.5 and base radius 1, just inside it.  Light
that meets a flat face of the encapsulant beyond the critical angle is totally reflected: only the critical cone,
(1 - cos(theta_c))/2 = 12.7 % of all the light, gets through such a face, less its Fresnel loss.  Under a FLAT cover (a
cylinder) that is all the top face lets out; the base below the emitter lets out as much, and the rest wanders to the
side wall or is absorbed.  A spherical cap -- `Conicoid.spherical_cap(radius, height)`, traced analytically, with the true
local normal at every point -- of the same base bends its surface towards the emitter.  A HEMISPHERE centred on the
emitter is met at normal incidence by every ray, the ones the base has totally reflected included (their mirror image
sits at the centre too), and loses only the 4 % Fresnel reflection: at least 0.96 (1 - 0.127) = 84 % of all the light
leaves through the dome, and what is reflected gets further chances.  The rows give the fraction of the photons that
leave through the top (flat cover: its top face; domes: the curved side), against the dome's height.

    python examples/dome_lens.py [photons]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pvtrace_amd import Absorber, Box, Conicoid, Cylinder, Light, Material, Node, Scene, engine, isotropic   # noqa: E402
from pvtrace_amd.engine import Recorder   # noqa: E402

BASE_RADIUS, INDEX = 1.0, 1.5
HEIGHTS = (0.1, 0.25, 0.5, 0.75, 1.0)     # of the dome over its base; 1.0 = the base radius: the hemisphere
FLAT_THICKNESS = 0.25


def cover(height=None):
    """The encapsulant over the emitter: a dome of `height`, or (None) the flat cover."""
    material = Material(refractive_index=INDEX, components=[Absorber(0.01, name="encapsulant")])
    if height is None:
        return Cylinder(FLAT_THICKNESS, BASE_RADIUS, material=material), FLAT_THICKNESS
    radius = (BASE_RADIUS * BASE_RADIUS + height * height) / (2.0 * height)   # the sphere through the base's rim
    return Conicoid.spherical_cap(radius, height, material=material), height


def lamp_scene(height=None):
    world = Node(name="world", geometry=Box((50.0, 50.0, 50.0), material=Material(refractive_index=1.0)))
    shape, thickness = cover(height)
    part = Node(name="cover", parent=world, geometry=shape)
    part.recorders = [Recorder("top-face", event="escaping", facet=(0, 0, 1)), Recorder("base", event="escaping", facet=(0, 0, -1)),
                      Recorder("escaping", event="escaping"), Recorder("lost", event="lost")]
    emitter = Node(name="emitter", parent=world, light=Light(direction=isotropic, name="emitter"))
    emitter.location = (0.0, 0.0, -0.5 * thickness + 1e-6)     # just inside the base
    return Scene(world)


def main(photons=200_000, seed=3):
    rows = {}
    for label, height in [("flat", None)] + [(f"dome {h:4.2f}", h) for h in HEIGHTS]:
        rec = engine.simulate(lamp_scene(height), photons, seed=seed, record_every=0, emit_seed=seed + 1).recorders
        top = rec["top-face"].rays if height is None else rec["escaping"].rays - rec["base"].rays
        rows[label] = {"height": height, "escaping": top / photons, "base": rec["base"].rays / photons, "lost": rec["lost"].rays / photons}
        print(f"{label:10s} out of the top {rows[label]['escaping']:6.3f}  out of the base {rows[label]['base']:6.3f}  "
              f"absorbed {rows[label]['lost']:6.3f}")
    return rows


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:2]))
