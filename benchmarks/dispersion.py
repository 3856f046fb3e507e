"""Cost of a refractive-index table n(wavelength): photons/s of the headline slab (benchmarks/configs.py cfg2_lsc:
LSC((5, 5, 1)) with the face recorders) three ways -- the scalar index 1.5, a one-point table holding 1.5 (the same
photon paths, bit for bit: the ratio is the cost of the lookups alone) and a 400-point Sellmeier table (Schott N-BK7
over 400-799 nm: other paths, and a deeper bracket) -- at 10^7 photons, tallies only, "fenced" (one `engine.simulate`
call, timed to its return).  The table is looked up at every step in the slab (the clock) and at every surface hit on
either side of it (Fresnel, the critical angle, Snell).

    python benchmarks/dispersion.py [--photons N] [--repeats R]     # on a machine with an MI355X

Prints one JSON line: photons/s per scene and the ratios to the scalar scene (> 1: faster than the scalar index).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pvtrace_amd import RefractiveIndexTable   # noqa: E402
from pvtrace_amd import engine   # noqa: E402
from benchmarks import configs   # noqa: E402

BK7_B = (1.03961212, 0.231792344, 1.01046945)
BK7_C = (0.00600069867, 0.0200179144, 103.560653)


def headline(index):
    scene = configs.cfg2_lsc()
    slab = next(n for n in scene.root.children if n.name == "LSC")
    slab.geometry.material.refractive_index = index
    return scene


def fenced(scene, n, seed):
    tic = time.perf_counter()
    engine.simulate(scene, n, seed=seed, record_every=0)
    return time.perf_counter() - tic


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--photons", type=int, default=10 ** 7)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    if not engine.is_available():
        print("HIP engine not built or no GPU visible; run: python -c 'import __graft_entry__ as g; g.build()'")
        return 1
    sellmeier = RefractiveIndexTable.from_sellmeier(BK7_B, BK7_C, np.arange(400.0, 800.0))
    scenes = {"scalar": headline(1.5), "one_point_table": headline(RefractiveIndexTable([555.0], [1.5])),
              "sellmeier_400": headline(sellmeier)}
    for scene in scenes.values():
        engine.simulate(scene, 100000, seed=1, record_every=0)   # load, upload, warm
    best = {name: float("inf") for name in scenes}
    for r in range(args.repeats):   # alternate the scenes, keep each one's best
        for name, scene in scenes.items():
            best[name] = min(best[name], fenced(scene, args.photons, 7 + r))
    out = {"photons": args.photons}
    for name in scenes:
        out[f"fenced_{name}_photons_per_s"] = args.photons / best[name]
    out["ratio_one_point_table_over_scalar"] = best["scalar"] / best["one_point_table"]
    out["ratio_sellmeier_400_over_scalar"] = best["scalar"] / best["sellmeier_400"]
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
