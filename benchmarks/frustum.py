"""Cost of the truncated cone (`pvtrace_amd.Frustum`, traced analytically by the extension kernel variants): photons/s of
the headline's dyed PMMA body (benchmarks/configs.py cfg2_lsc: its world, lamp, material and face recorders) at 10^7
photons, tallies only, "fenced" (one `engine.simulate` call, timed to its return), with the body as

  (a) the 5 x 5 x 1 cm box, on the extension variants (a `reacted` volume map of 1 x 1 x 1: the slab has no Reactor, so
      the map counts nothing -- the way benchmarks/history_counters.py case (b) forces them);
  (b) a cylinder of the same height and volume (radius 2.82 cm), on the plain variants;
  (b2) the same cylinder on the extension variants, forced as in (a);
  (c) the frustum with both radii equal to (b)'s: the same solid, the new code path (it runs the extension variants, so
      (c)/(b2) is the price of the shape and (b2)/(b) that of the family);
  (d) a 2:1 taper of the same height and volume (radii 3.69 and 1.85 cm).

    python benchmarks/frustum.py [--photons N] [--repeats R]     # on a machine with an MI355X

Prints one JSON line: per case the median, minimum and maximum photons/s over the windows (the cases alternate, one warm
launch each first), the kernel variant each ran, and the ratios (c)/(b), (c)/(b2) and (d)/(c) of the medians.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pvtrace_amd import Cylinder, Frustum, VolumeMap, engine   # noqa: E402
from pvtrace_amd.engine import Session   # noqa: E402
from benchmarks import configs   # noqa: E402

LOWER, UPPER = (-2.5, -2.5, -0.5), (2.5, 2.5, 0.5)
HEIGHT, VOLUME = 1.0, 25.0
RADIUS = math.sqrt(VOLUME / (math.pi * HEIGHT))
R_TOP = math.sqrt(3.0 * VOLUME / (7.0 * math.pi * HEIGHT))   # V = pi L (r0^2 + r0 r1 + r1^2) / 3 with r0 = 2 r1
CASES = ("a_box_extension", "b_cylinder", "b2_cylinder_extension", "c_frustum_equal_radii", "d_taper_2_to_1")


def body_scene(name):
    scene = configs.cfg2_lsc()
    body = next(n for n in scene.root.children if n.name == "LSC")
    material = body.geometry.material
    if name in ("a_box_extension", "b2_cylinder_extension"):
        body.volume_maps = [VolumeMap("reacted", (1, 1, 1), LOWER, UPPER, event="reacted")]
    if name in ("b_cylinder", "b2_cylinder_extension"):
        body.geometry = Cylinder(HEIGHT, RADIUS, material=material)
    elif name == "c_frustum_equal_radii":
        body.geometry = Frustum(HEIGHT, RADIUS, RADIUS, material=material)
    elif name == "d_taper_2_to_1":
        body.geometry = Frustum(HEIGHT, 2.0 * R_TOP, R_TOP, material=material)
    return scene


def variant_of(scene):
    with Session(scene) as s:
        s.collect(s.submit(1024, 1, record_every=0, emit_seed=1))
        return s.dscene.launch_info()["variant"]


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
    scenes = {name: body_scene(name) for name in cases}
    for scene in scenes.values():
        engine.simulate(scene, args.photons, seed=1, record_every=0)   # load, upload, warm the clocks
    windows = {name: [] for name in scenes}
    for r in range(args.repeats):   # alternate the cases
        for name, scene in scenes.items():
            tic = time.perf_counter()
            engine.simulate(scene, args.photons, seed=7 + r, record_every=0)
            windows[name].append(args.photons / (time.perf_counter() - tic))
    out = {"photons": args.photons, "windows": args.repeats}
    for name, scene in scenes.items():
        out[f"{name}_photons_per_s"] = {"median": statistics.median(windows[name]), "min": min(windows[name]),
                                        "max": max(windows[name]), "variant": variant_of(scene)}
    for top, bottom in (("c_frustum_equal_radii", "b_cylinder"), ("c_frustum_equal_radii", "b2_cylinder_extension"),
                        ("d_taper_2_to_1", "c_frustum_equal_radii")):
        if top in scenes and bottom in scenes:
            out[f"{top}_over_{bottom}"] = out[f"{top}_photons_per_s"]["median"] / out[f"{bottom}_photons_per_s"]["median"]
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
