"""Cost of patterned coatings (`Coating(..., pattern=CoatingPattern(...))`): photons/s of the headline's 5 x 5 x 1 cm slab
(benchmarks/configs.py cfg2_lsc) at 10^7 photons, tallies only, "fenced" (one `engine.simulate` call, timed to its return):

  (a) no coating, on the plain kernel variants;
  (b) none, on the extension variants the patterned scenes run on (a `reacted` volume map of 1 x 1 x 1: the slab has no
      Reactor, so the map counts nothing);
  (c) the bottom face a Lambertian mirror through a 64 x 64 x 1 checker mask;
  (d) the same through a 2048 x 2048 x 1 checker mask (4 MiB of cells: beyond what the caches hold beside the tables);
  (e) the same coverage (half the face) written as 32 `region` strips, every other one of 64 along x -- the linear scan
      over the node's coating rows that a pattern replaces.

    python benchmarks/coating_pattern.py [--photons N] [--repeats R]     # on a machine with an MI355X

Prints one JSON line: per case the median, minimum and maximum photons/s over the windows (the cases alternate, one warm
launch each first), and the ratios (c)/(b), (d)/(c) and (c)/(e) of the medians with the min-max range each could take
(min of one over max of the other, and the reverse).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pvtrace_amd import (   # noqa: E402
    CoatedSurfaceDelegate, Coating, CoatingPattern, Material, Surface, VolumeMap, engine,
)
from benchmarks import configs   # noqa: E402

LOWER, UPPER = (-2.5, -2.5, -0.5), (2.5, 2.5, 0.5)
BOTTOM = (0, 0, -1)
CASES = ("a_plain", "b_extension", "c_checker_64", "d_checker_2048", "e_regions_32")


def checker(n):
    ix, iy = np.indices((n, n))
    return ((ix + iy) % 2 == 0).astype(np.uint8).reshape(n, n, 1)


def mirror(**where):
    return Coating(BOTTOM, reflectivity=1.0, reflection="lambertian", **where)


def slab(name):
    scene = configs.cfg2_lsc()
    body = next(n for n in scene.root.children if n.name == "LSC")
    if name == "b_extension":
        body.volume_maps = [VolumeMap("reacted", (1, 1, 1), LOWER, UPPER, event="reacted")]
    coatings = None
    if name in ("c_checker_64", "d_checker_2048"):
        n = 64 if name == "c_checker_64" else 2048
        coatings = [mirror(pattern=CoatingPattern(checker(n), (LOWER[0], LOWER[1], None), (UPPER[0], UPPER[1], None)))]
    if name == "e_regions_32":
        h = (UPPER[0] - LOWER[0]) / 64
        coatings = [mirror(region=((LOWER[0] + 2 * k * h, LOWER[0] + (2 * k + 1) * h), None, None)) for k in range(32)]
    if coatings is not None:
        material = body.geometry.material
        body.geometry.material = Material(refractive_index=material.refractive_index, components=list(material.components),
                                          surface=Surface(delegate=CoatedSurfaceDelegate(coatings)))
    return scene


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--photons", type=int, default=10 ** 7)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cases", default=",".join(CASES), help="comma-separated subset of the cases")
    args = ap.parse_args()
    cases = tuple(name for name in CASES if name in args.cases.split(","))
    if not engine.is_available():
        print("HIP engine not built or no GPU visible; run: python -c 'import __graft_entry__ as g; g.build()'")
        return 1
    scenes = {name: slab(name) for name in cases}
    for scene in scenes.values():
        engine.simulate(scene, args.photons, seed=1, record_every=0)   # load, upload, warm the clocks
    windows = {name: [] for name in scenes}
    for r in range(args.repeats):   # alternate the cases
        for name, scene in scenes.items():
            tic = time.perf_counter()
            engine.simulate(scene, args.photons, seed=7 + r, record_every=0)
            windows[name].append(args.photons / (time.perf_counter() - tic))
    out = {"photons": args.photons, "windows": args.repeats}
    for name in scenes:
        out[f"{name}_photons_per_s"] = {"median": statistics.median(windows[name]), "min": min(windows[name]), "max": max(windows[name])}
    for top, bottom in (("c_checker_64", "b_extension"), ("d_checker_2048", "c_checker_64"), ("c_checker_64", "e_regions_32")):
        if top in scenes and bottom in scenes:
            t, b = out[f"{top}_photons_per_s"], out[f"{bottom}_photons_per_s"]
            out[f"{top}_over_{bottom}"] = {"median": t["median"] / b["median"], "min": t["min"] / b["max"], "max": t["max"] / b["min"]}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
