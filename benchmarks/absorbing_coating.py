"""Cost of absorbing coatings (`Coating(..., absorptivity=...)` and `detected` recorders): photons/s of the headline's
5 x 5 x 1 cm slab (benchmarks/configs.py cfg2_lsc) at 10^7 photons, tallies only, "fenced" (one `engine.simulate` call,
timed to its return):

  (a) no absorbing coating, on the plain kernel variants;
  (b) none, on the extension variants the absorbing scenes run on (a `reacted` volume map of 1 x 1 x 1: the slab has no
      Reactor, so the map counts nothing);
  (c) four edge cells with the scalar EQE 0.9 (`reflectivity=0.0, transmission="matched"`) and a `detected` recorder each;
  (d) the same with a 64 x 16 EQE(wavelength, angle) table.

    python benchmarks/absorbing_coating.py [--photons N] [--repeats R]     # on a machine with an MI355X

Prints one JSON line: per case the median, minimum and maximum photons/s over the windows (the cases alternate, one warm
launch each first) and the share of photons detected.  Cases (a) and (b) need no absorbing coating and run on a commit
without them; `--cases a_plain,b_extension` runs them alone, as such a commit does.
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

from pvtrace_amd import CoatedSurfaceDelegate, Coating, Material, Surface, VolumeMap, engine   # noqa: E402
from pvtrace_amd.engine import Recorder   # noqa: E402
from benchmarks import configs   # noqa: E402

LOWER, UPPER = (-2.5, -2.5, -0.5), (2.5, 2.5, 0.5)
EDGES = {"left": (-1, 0, 0), "right": (1, 0, 0), "near": (0, -1, 0), "far": (0, 1, 0)}
HAS_ABSORB = "absorptivity" in Coating.__init__.__code__.co_varnames
CASES = ("a_plain", "b_extension") + (("c_scalar_cells", "d_table_cells") if HAS_ABSORB else ())


def eqe_table():
    from pvtrace_amd import AbsorptivityTable

    wl, ang = np.linspace(400.0, 800.0, 64), np.linspace(0.0, 90.0, 16)
    spectral = 0.9 * (0.35 + 0.65 / (1.0 + np.exp(-(wl - 560.0) / 30.0)))
    return AbsorptivityTable(wl, np.cos(np.radians(ang))[:, None] ** 0.25 * spectral[None, :], angle=ang)


def slab(name):
    scene = configs.cfg2_lsc()
    body = next(n for n in scene.root.children if n.name == "LSC")
    if name == "b_extension":
        body.volume_maps = [VolumeMap("reacted", (1, 1, 1), LOWER, UPPER, event="reacted")]
    if name in ("c_scalar_cells", "d_table_cells"):
        eqe = 0.9 if name == "c_scalar_cells" else eqe_table()
        cells = [Coating(normal, reflectivity=0.0, absorptivity=eqe, transmission="matched") for normal in EDGES.values()]
        material = body.geometry.material
        body.geometry.material = Material(refractive_index=material.refractive_index, components=list(material.components),
                                          surface=Surface(delegate=CoatedSurfaceDelegate(cells)))
        body.recorders = list(body.recorders) + [Recorder(f"cell-{label}", event="detected", facet=normal)
                                                 for label, normal in EDGES.items()]
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
    detected = {name: 0.0 for name in scenes}
    for r in range(args.repeats):   # alternate the cases
        for name, scene in scenes.items():
            tic = time.perf_counter()
            result = engine.simulate(scene, args.photons, seed=7 + r, record_every=0)
            windows[name].append(args.photons / (time.perf_counter() - tic))
            detected[name] = sum(rec.rays for rec in result.recorders.values() if rec.spec.event == "detected") / args.photons
    out = {"photons": args.photons, "windows": args.repeats}
    for name in scenes:
        out[f"{name}_photons_per_s"] = {"median": statistics.median(windows[name]), "min": min(windows[name]), "max": max(windows[name])}
        out[f"{name}_detected_share"] = detected[name]
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
