"""Cost of aligned components (`Alignment`): photons/s of the headline's 5 x 5 x 1 cm slab (benchmarks/configs.py cfg2_lsc)
at 10^7 photons, tallies only, "fenced" (one `engine.simulate` call, timed to its return):

  (a) no alignment, on the plain kernel variants;
  (b) none, on the extension variants the aligned scenes run on (a `reacted` volume map of 1 x 1 x 1: the slab has no
      Reactor, so the map counts nothing);
  (c) the dye and the background aligned along the slab's normal with absorption order 0.6;
  (d) the same with the dye's emission order 0.6 as well.

    python benchmarks/aligned_luminophore.py [--photons N] [--repeats R]     # on a machine with an MI355X

Prints one JSON line: per case the median, minimum and maximum photons/s over the windows (the cases alternate, one warm
launch each first), and the ratios (c)/(b) and (d)/(b) of the medians with the min-max range each could take (min of one
over max of the other, and the reverse).  (The aligned cases trace other physics: more light is guided.)
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pvtrace_amd import Alignment, VolumeMap, engine   # noqa: E402
from benchmarks import configs   # noqa: E402

LOWER, UPPER = (-2.5, -2.5, -0.5), (2.5, 2.5, 0.5)
CASES = ("a_plain", "b_extension", "c_absorption", "d_absorption_emission")


def slab(name):
    scene = configs.cfg2_lsc()
    body = next(n for n in scene.root.children if n.name == "LSC")
    if name == "b_extension":
        body.volume_maps = [VolumeMap("reacted", (1, 1, 1), LOWER, UPPER, event="reacted")]
    if name in ("c_absorption", "d_absorption_emission"):
        emission = 0.6 if name == "d_absorption_emission" else 0.0
        for component in body.geometry.material.components:
            emits = emission if type(component).__name__ == "Luminophore" else 0.0
            component.alignment = Alignment((0.0, 0.0, 1.0), absorption_order=0.6, emission_order=emits)
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
    for top, bottom in (("c_absorption", "b_extension"), ("d_absorption_emission", "b_extension"), ("b_extension", "a_plain")):
        if top in scenes and bottom in scenes:
            t, b = out[f"{top}_photons_per_s"], out[f"{bottom}_photons_per_s"]
            out[f"{top}_over_{bottom}"] = {"median": t["median"] / b["median"], "min": t["min"] / b["max"], "max": t["max"] / b["min"]}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
