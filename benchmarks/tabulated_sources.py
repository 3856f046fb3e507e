"""Cost of tabulated sources (`pvtrace_amd.PositionGrid`, `pvtrace_amd.DirectionTable`) sampled by the
device emitter: photons/s of the headline's dyed PMMA slab (benchmarks/configs.py cfg2_lsc: its world, material and face
recorders) at 10^7 photons, tallies only, under a lamp 5 cm above the face that is

  (a) a rectangle of the face's size with Lambertian directions, from the built-ins, on the device;
  (b) the same source as a 1 x 1 x 1 `PositionGrid` and `ScatterLobe.lambertian().table`: (b)/(a) is the price of the
      table code for a source the closed forms can express;
  (c) a 256 x 256 image over the face (a smooth profile, one quadrant shaded) and a 10-degree Gaussian table;
  (d) a 2048 x 2048 image of the same profile: (d)/(c) is the price of a 22-step bisection through a 32 MiB table;
  (e) case (c) with `emission="host"`: (c)/(e) is what keeping such a light on the device is worth.

Every case keeps ONE `Session` open -- the scene is lowered, packed and uploaded once -- and is timed launch for launch:
`launch` is the wall time of submit + collect of one launch, `kernel` the GPU's own time of that launch (`kernel_ms`).

    python benchmarks/tabulated_sources.py [--photons N] [--repeats R]     # on a machine with an MI355X

Prints one JSON line: per case the median, minimum and maximum photons/s over the windows, by `launch` and by `kernel` (the
cases alternate, one warm launch each first), the kernel variant and the emission each ran, and the ratios (b)/(a),
(c)/(a), (d)/(c) from the KERNEL medians and (c)/(e) from the LAUNCH medians (the host's emission is outside the kernel).
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

from pvtrace_amd import DirectionTable, Light, PositionGrid, ScatterLobe, engine, lambertian   # noqa: E402
from pvtrace_amd.engine import Session   # noqa: E402
from pvtrace_amd.light import RectangularMask   # noqa: E402
from benchmarks import configs   # noqa: E402

HALF = 2.5
CASES = ("a_builtin_rect_lambertian", "b_grid_1x1x1_lambertian_table", "c_image_256_gaussian", "d_image_2048_gaussian",
         "e_image_256_gaussian_host")


def image(n):
    """A smooth beam profile on n x n cells, one quadrant shaded."""
    x = (np.arange(n) + 0.5) / n - 0.5
    profile = np.exp(-0.5 * (x[:, None] ** 2 + x[None, :] ** 2) / 0.3 ** 2) * (1.0 + 0.3 * np.sin(40.0 * x[:, None]))
    profile[: n // 2, : n // 2] = 0.0
    return profile


def lamp_scene(name):
    scene = configs.cfg2_lsc()
    lamp = next(n for n in scene.root.preorder() if getattr(n, "light", None) is not None)
    flat = lambda weights: PositionGrid(weights, (-HALF, -HALF, None), (HALF, HALF, None))
    gaussian = lambda: DirectionTable(ScatterLobe.gaussian(10.0, "normal").table)
    lamp.light = {
        "a_builtin_rect_lambertian": lambda: Light(position=RectangularMask(HALF, HALF), direction=lambertian),
        "b_grid_1x1x1_lambertian_table": lambda: Light(position=flat(np.ones((1, 1))), direction=DirectionTable(ScatterLobe.lambertian().table)),
        "c_image_256_gaussian": lambda: Light(position=flat(image(256)), direction=gaussian()),
        "d_image_2048_gaussian": lambda: Light(position=flat(image(2048)), direction=gaussian()),
        "e_image_256_gaussian_host": lambda: Light(position=flat(image(256)), direction=gaussian()),
    }[name]()
    lamp.light.name = "lamp"
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
    sessions = {name: Session(lamp_scene(name), emission="host" if name.endswith("_host") else "device") for name in cases}
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
                                            "variant": s.dscene.launch_info()["variant"], "emission": s.emission}
    finally:
        for s in sessions.values():
            s.close()
    for top, bottom, clock in (("b_grid_1x1x1_lambertian_table", "a_builtin_rect_lambertian", "kernel"),
                               ("c_image_256_gaussian", "a_builtin_rect_lambertian", "kernel"),
                               ("d_image_2048_gaussian", "c_image_256_gaussian", "kernel"),
                               ("c_image_256_gaussian", "e_image_256_gaussian_host", "launch")):
        if top in sessions and bottom in sessions:
            out[f"{top}_over_{bottom}"] = (out[f"{top}_photons_per_s"][clock]["median"] /
                                           out[f"{bottom}_photons_per_s"][clock]["median"])
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
