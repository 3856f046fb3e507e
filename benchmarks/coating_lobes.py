"""Cost of scattering coatings (`Coating(reflection=ScatterLobe(...))`): photons/s of the headline's 5 x 5 x 1 cm slab
(benchmarks/configs.py cfg2_lsc) at 10^7 photons, tallies only, one `Session` per case, by the GPU's own time of each
launch (`kernel_ms`):

  (a) the bottom face the built-in Lambertian mirror, on the extension variants the lobe scenes run on (a `reacted` volume
      map of 1 x 1 x 1: the slab has no Reactor, so the map counts nothing);
  (b) the same face with `ScatterLobe.lambertian()`: the same law, sampled from the 257-node table;
  (c) the same face with a Gaussian gloss lobe of 10 degrees about "specular";
  (d) case (b) through a 64 x 64 x 1 checker `CoatingPattern`.

    python benchmarks/coating_lobes.py [--photons N] [--repeats R]     # on a machine with an MI355X

Prints one JSON line: per case the median, minimum and maximum photons/s over the windows (the cases alternate, one warm
launch each first) and the ratios (b)/(a), (c)/(a), (d)/(b) of the medians.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pvtrace_amd import (   # noqa: E402
    CoatedSurfaceDelegate, Coating, CoatingPattern, Material, ScatterLobe, Surface, VolumeMap, engine,
)
from pvtrace_amd.engine import Session   # noqa: E402
from benchmarks import configs   # noqa: E402

LOWER, UPPER = (-2.5, -2.5, -0.5), (2.5, 2.5, 0.5)
BOTTOM = (0, 0, -1)
CASES = ("a_lambertian", "b_lobe_cosine", "c_lobe_gloss", "d_lobe_cosine_checker_64")


def checker(n):
    ix, iy = np.indices((n, n))
    return ((ix + iy) % 2 == 0).astype(np.uint8).reshape(n, n, 1)


def slab(name):
    scene = configs.cfg2_lsc()
    body = next(n for n in scene.root.children if n.name == "LSC")
    where = {}
    if name == "a_lambertian":
        body.volume_maps = [VolumeMap("reacted", (1, 1, 1), LOWER, UPPER, event="reacted")]
        reflection = "lambertian"
    elif name == "c_lobe_gloss":
        reflection = ScatterLobe.gaussian(10.0, "specular")
    else:
        reflection = ScatterLobe.lambertian()
    if name == "d_lobe_cosine_checker_64":
        where["pattern"] = CoatingPattern(checker(64), (LOWER[0], LOWER[1], None), (UPPER[0], UPPER[1], None))
    material = body.geometry.material
    coatings = [Coating(BOTTOM, reflectivity=1.0, reflection=reflection, **where)]
    body.geometry.material = Material(refractive_index=material.refractive_index, components=list(material.components),
                                      surface=Surface(delegate=CoatedSurfaceDelegate(coatings)))
    return scene


def stats(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


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
    out = {"photons": args.photons, "windows": args.repeats}
    sessions = {name: Session(slab(name)) for name in cases}
    try:
        def launch(name, seed):
            s = sessions[name]
            result = s.collect(s.submit(args.photons, seed, record_every=0, emit_seed=seed + 1))
            return 1e-3 * result.kernel_ms

        for name in sessions:
            launch(name, 1)   # load, upload, warm the clocks
        kernel = {name: [] for name in sessions}
        for r in range(args.repeats):   # alternate the cases
            for name in sessions:
                kernel[name].append(args.photons / launch(name, 7 + r))
        for name, s in sessions.items():
            out[f"{name}_photons_per_s"] = dict(stats(kernel[name]), variant=s.dscene.launch_info()["variant"])
    finally:
        for s in sessions.values():
            s.close()
    for top, bottom in (("b_lobe_cosine", "a_lambertian"), ("c_lobe_gloss", "a_lambertian"), ("d_lobe_cosine_checker_64", "b_lobe_cosine")):
        if top in sessions and bottom in sessions:
            t, b = out[f"{top}_photons_per_s"], out[f"{bottom}_photons_per_s"]
            out[f"{top}_over_{bottom}"] = {"median": t["median"] / b["median"], "min": t["min"] / b["max"], "max": t["max"] / b["min"]}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
