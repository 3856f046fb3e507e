"""Fluence inside a slab: a path-length `VolumeMap` against Beer-Lambert, and against the `absorbed` map.

A 2 x 2 x 1 cm index-matched slab is lit evenly and normally from above, once clear and once with a uniform absorber of
alpha = 1 / cm.  The `pathlength` map sums the path photons travel in each voxel (exact fixed-point integers, one count
= 2^-30 cm); divided by the voxel's volume it is the fluence.  Over depth the fluence per unit of incident fluence
falls as exp(-alpha z) averaged over each layer -- and stays 1 in the clear slab, where an `absorbed` map shows nothing
at all.  In the absorbing slab alpha x `pathlength` estimates what the `absorbed` map counts, cell by cell.

    python examples/fluence_map.py [photons]
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pvtrace_amd import (   # noqa: E402
    Absorber, Box, Light, Material, Node, Scene, Surface, VolumeMap, engine, rectangular_mask,
)
from pvtrace_amd.material import NullSurfaceDelegate   # noqa: E402

SHAPE, LOWER, UPPER = (4, 4, 8), (-1.0, -1.0, -0.5), (1.0, 1.0, 0.5)
AREA, DEPTH = 4.0, 1.0


def slab(alpha):
    world = Node(name="world", geometry=Box((40.0, 40.0, 40.0), material=Material(refractive_index=1.0)))
    components = [Absorber(alpha, name="ink")] if alpha > 0.0 else []
    body = Node(name="slab", parent=world, geometry=Box((2.0, 2.0, 1.0), material=Material(
        refractive_index=1.0, surface=Surface(NullSurfaceDelegate()), components=components)))
    body.volume_maps = [VolumeMap("path", SHAPE, LOWER, UPPER, event="pathlength"),
                        VolumeMap("absorbed", SHAPE, LOWER, UPPER, event="absorbed")]
    lamp = Node(name="lamp", parent=world, light=Light(position=functools.partial(rectangular_mask, 1.0, 1.0), name="lamp"))
    lamp.location = (0.0, 0.0, 5.0)
    lamp.rotate(np.radians(180), (1, 0, 0))
    return Scene(world)


def profile(alpha, photons, seed):
    """Fluence per layer over the incident fluence, what Beer-Lambert expects of it, and how far apart they are."""
    result = engine.simulate(slab(alpha), photons, seed=seed, record_every=0, emit_seed=seed + 1)
    path, absorbed = result.volume_maps["path"], result.volume_maps["absorbed"]
    layers = SHAPE[2]
    h = DEPTH / layers
    # layer k of the lattice runs upwards in z; the light comes from above: depth 0 is the top layer
    length = path.pathlength.sum(axis=(0, 1))[::-1]
    measured = length / (AREA * h) / (photons / AREA)          # mean fluence of the layer / incident fluence
    z = np.arange(layers + 1) * h
    expected = (np.exp(-alpha * z[:-1]) - np.exp(-alpha * z[1:])) / (alpha * h) if alpha > 0.0 else np.ones(layers)
    # a photon's path in a layer is h with the probability that it crosses it, and less where it stops: the variance of
    # the layer's sum is at most photons x p h^2, p = exp(-alpha z_top) the probability of reaching the layer
    # (so that of `measured` at most p / photons)
    sigma = np.sqrt(np.exp(-alpha * z[:-1]) / photons)
    worst = float((np.abs(measured - expected) / sigma).max())
    out = {"profile": measured, "expected": expected, "worst_sigma": worst, "path": path, "absorbed": absorbed}
    if alpha > 0.0:
        # collision against track-length estimator, cell by cell: A - alpha L has variance E[alpha L]
        rate = alpha * path.pathlength
        out["absorbed_vs_path_worst_sigma"] = float(np.abs((absorbed.counts - rate) / np.sqrt(rate)).max())
    return out


def main(photons=200_000, seed=11):
    clear, absorbing = profile(0.0, photons, seed), profile(1.0, photons, seed)
    print(f"photons {photons}; fluence per layer / incident fluence, top to bottom")
    print("  clear slab     ", " ".join(f"{v:.4f}" for v in clear["profile"]), f"(absorbed: {clear['absorbed'].total})")
    print("  alpha = 1 / cm ", " ".join(f"{v:.4f}" for v in absorbing["profile"]))
    print("  Beer-Lambert   ", " ".join(f"{v:.4f}" for v in absorbing["expected"]),
          f"(worst deviation {absorbing['worst_sigma']:.2f} sigma)")
    print(f"  absorbed map against alpha x pathlength, worst cell: {absorbing['absorbed_vs_path_worst_sigma']:.2f} sigma")
    return {"clear": clear, "absorbing": absorbing}


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:2]))
