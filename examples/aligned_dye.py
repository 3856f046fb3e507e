"""Aligned dyes in a luminescent slab: how dye alignment moves light out of the escape cone.

A 5 x 5 x 0.5 cm slab of index 1.5 holds a dye of quantum yield 1.  A photon emitted within the critical angle of the slab's
normal leaves through a large face; the rest is guided.  For an isotropic emitter the escape-cone share of the first
emission is 1 - mu_c = 0.2546 (mu_c = sqrt(1 - 1 / n^2)).  With the emission dipoles along the slab's normal
(homeotropic alignment, `Alignment((0, 0, 1), emission_order=1.0)`) the emission falls as sin^2 about the normal and the
share drops to 0.0890; dipoles lying in the slab's plane (planar, order -0.5 about the normal) raise it.  The closed form
beside each measured share is the integral of f(mu; S) = 1 - S (1.5 mu^2 - 0.5) from mu_c to 1 (both cones).

    python examples/aligned_dye.py [photons]     # on a machine with an MI355X
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pvtrace_amd import Alignment, Box, Event, Light, Luminophore, Material, Node, Scene, engine   # noqa: E402

INDEX = 1.5
NORMAL = (0.0, 0.0, 1.0)
CASES = {"isotropic": 0.0, "homeotropic": 1.0, "planar": -0.5}     # the emission order about the slab's normal
MAX_EVENTS = 24


def escape_cone_share(order, index=INDEX):
    """Integral of f(mu; S) over mu_c .. 1: the share of an emission inside the two escape cones."""
    mu_c = math.sqrt(1.0 - 1.0 / (index * index))
    return (1.0 + 0.5 * order) * (1.0 - mu_c) - 0.5 * order * (1.0 - mu_c ** 3)


def build(order):
    world = Node(name="world", geometry=Box((40.0, 40.0, 40.0), material=Material(refractive_index=1.0)))
    alignment = None if order == 0.0 else Alignment(NORMAL, emission_order=order)
    dye = Luminophore(8.0, x=np.arange(400.0, 801.0), quantum_yield=1.0, name="dye", alignment=alignment)
    Node(name="slab", parent=world, geometry=Box((5.0, 5.0, 0.5), material=Material(refractive_index=INDEX, components=[dye])))
    lamp = Node(name="lamp", parent=world, light=Light(name="lamp"))
    lamp.location = (0.0, 0.0, 3.0)
    lamp.rotate(math.pi, (1.0, 0.0, 0.0))
    return Scene(world)


def main(photons=100_000):
    mu_c = math.sqrt(1.0 - 1.0 / (INDEX * INDEX))
    out = {}
    for name, order in CASES.items():
        result = engine.simulate(build(order), photons, seed=1, record_every=1, max_events=MAX_EVENTS, maxsteps=MAX_EVENTS // 3)
        counts = np.asarray(result.data["counts"])
        kinds = np.asarray(result.data["kind"]).reshape(len(counts), MAX_EVENTS)
        live = np.arange(MAX_EVENTS)[None, :] < counts[:, None]
        emits = (kinds == Event.EMIT.value) & live
        rays = np.flatnonzero(emits.any(axis=1))
        first = np.argmax(emits[rays], axis=1)     # the first emission of every photon that has one
        mu = np.asarray(result.data["direction"]).reshape(len(counts), MAX_EVENTS, 3)[rays, first, 2]
        in_cone = int(np.sum(np.abs(mu) > mu_c))
        closed = escape_cone_share(order)
        out[name] = {"emitted": int(len(rays)), "in_cone": in_cone, "share": in_cone / len(rays), "closed_form": closed}
        print(f"{name:12s} S_e = {order:4.1f}: {in_cone} of {len(rays)} first emissions inside the escape cones, "
              f"share {in_cone / len(rays):.4f}; closed form {closed:.4f}")
    return out


if __name__ == "__main__":
    main(int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000)
