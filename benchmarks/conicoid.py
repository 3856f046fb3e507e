"""Cost of the solids of revolution of a conic (`pvtrace_amd.Conicoid`, traced analytically by the extension kernel
variants): photons/s of the headline's dyed PMMA body (benchmarks/configs.py cfg2_lsc: its world, lamp, material and
face recorders) at 10^7 photons, tallies only, with the body as

  (a) a cylinder of the slab's height and volume (radius 2.82 cm), on the extension variants (a `reacted` volume map of
      1 x 1 x 1: the body has no Reactor, so the map counts nothing -- the way benchmarks/history_counters.py case (b)
      forces them);
  (b) the same solid as `Conicoid(L, (r*r, 0, 0))`: (b)/(a) is the price of the general quadric, its cancellation-free
      roots and the out-of-line call against the cylinder's inlined test;
  (c) a sphere of the slab's volume (radius 1.81 cm), on the extension variants, forced as in (a);
  (d) the same solid as `Conicoid.ellipsoid(R, R)`: (d)/(c) likewise against the sphere's inlined test;
  (e) a dome, `Conicoid.spherical_cap(R, h)` with a base of the cylinder's radius and the cylinder's height.

Every case keeps ONE `Session` open -- the scene is lowered, packed and uploaded once -- and is timed launch for launch:
`launch` is the wall time of submit + collect of one launch, `kernel` the GPU's own time of that launch (`kernel_ms`).

    python benchmarks/conicoid.py [--photons N] [--repeats R]     # on a machine with an MI355X

Prints one JSON line: per case the median, minimum and maximum photons/s over the windows, by `launch` and by `kernel` (the
cases alternate, one warm launch each first), the kernel variant each ran, and from the KERNEL medians the ratios (b)/(a)
and (d)/(c).
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

from pvtrace_amd import Conicoid, Cylinder, Sphere, VolumeMap, engine   # noqa: E402
from pvtrace_amd.engine import Session   # noqa: E402
from benchmarks import configs   # noqa: E402

HEIGHT, VOLUME = 1.0, 25.0
RADIUS = math.sqrt(VOLUME / (math.pi * HEIGHT))
BALL = (3.0 * VOLUME / (4.0 * math.pi)) ** (1.0 / 3.0)
DOME_RADIUS = (RADIUS * RADIUS + HEIGHT * HEIGHT) / (2.0 * HEIGHT)   # the sphere through the base's rim
CASES = ("a_cylinder_extension", "b_conicoid_cylinder", "c_sphere_extension", "d_conicoid_sphere", "e_dome")


def body_scene(name):
    scene = configs.cfg2_lsc()
    body = next(n for n in scene.root.children if n.name == "LSC")
    material = body.geometry.material
    if name in ("a_cylinder_extension", "c_sphere_extension"):
        reach = max(RADIUS, BALL) + 0.5
        body.volume_maps = [VolumeMap("reacted", (1, 1, 1), (-reach,) * 3, (reach,) * 3, event="reacted")]
    body.geometry = {
        "a_cylinder_extension": lambda: Cylinder(HEIGHT, RADIUS, material=material),
        "b_conicoid_cylinder": lambda: Conicoid(HEIGHT, (RADIUS * RADIUS, 0.0, 0.0), material=material),
        "c_sphere_extension": lambda: Sphere(BALL, material=material),
        "d_conicoid_sphere": lambda: Conicoid.ellipsoid(BALL, BALL, material=material),
        "e_dome": lambda: Conicoid.spherical_cap(DOME_RADIUS, HEIGHT, material=material),
    }[name]()
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
    sessions = {name: Session(body_scene(name)) for name in cases}
    try:
        def launch(name, seed):
            s = sessions[name]
            tic = time.perf_counter()
            result = s.collect(s.submit(args.photons, seed, record_every=0, emit_seed=seed + 1))
            return time.perf_counter() - tic, 1e-3 * result.kernel_ms

        for name in sessions:
            launch(name, 1)   # load, upload, warm the clocks
        wall, kernel = {name: [] for name in sessions}, {name: [] for name in sessions}
        for r in range(args.repeats):   # alternate the cases
            for name in sessions:
                w, k = launch(name, 7 + r)
                wall[name].append(args.photons / w)
                kernel[name].append(args.photons / k)
        for name, s in sessions.items():
            out[f"{name}_photons_per_s"] = {"launch": stats(wall[name]), "kernel": stats(kernel[name]),
                                            "variant": s.dscene.launch_info()["variant"]}
    finally:
        for s in sessions.values():
            s.close()
    median = {name: out[f"{name}_photons_per_s"]["kernel"]["median"] for name in sessions}
    for top, bottom in (("b_conicoid_cylinder", "a_cylinder_extension"), ("d_conicoid_sphere", "c_sphere_extension")):
        if top in median and bottom in median:
            out[f"{top}_over_{bottom}"] = median[top] / median[bottom]
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
