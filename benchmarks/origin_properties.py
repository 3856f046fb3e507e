"""Cost of the launch-origin histogram properties (`Histogram("origin_wavelength" | "origin_x" | "origin_y" | "origin_z", ...)`):
photons/s of the headline's 5 x 5 x 1 cm slab (benchmarks/configs.py cfg2_lsc) at 10^7 photons, tallies only, "fenced" (one
`engine.simulate` call, timed to its return):

  (a) no origin, on the plain kernel variants;
  (b) none, on the extension variants the scenes that read an origin run on (a `reacted` volume map of 1 x 1 x 1: the slab
      has no Reactor, so the map counts nothing);
  (c) four edge recorders with an `origin_wavelength` histogram;
  (d) the same plus an `origin_x` x `origin_y` heatmap on each.

    python benchmarks/origin_properties.py [--photons N] [--repeats R]     # on a machine with an MI355X

Prints one JSON line: per case the median, minimum and maximum photons/s over the windows (the cases alternate, one warm
launch each first), and the ratios (c)/(b) and (d)/(b) of the medians.  Cases (a) and (b) read no origin and run on a
commit without them; `--cases a_plain,b_extension` runs them alone, as such a commit does.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pvtrace_amd import VolumeMap, engine   # noqa: E402
from pvtrace_amd.engine import Heatmap, Histogram, Recorder   # noqa: E402
from pvtrace_amd.engine import recorder as recorder_module   # noqa: E402
from benchmarks import configs   # noqa: E402

LOWER, UPPER = (-2.5, -2.5, -0.5), (2.5, 2.5, 0.5)
EDGES = {"left": (-1, 0, 0), "right": (1, 0, 0), "near": (0, -1, 0), "far": (0, 1, 0)}
HAS_ORIGINS = hasattr(recorder_module, "ORIGIN_PROPERTIES")
CASES = ("a_plain", "b_extension") + (("c_origin_wavelength", "d_origin_heatmap") if HAS_ORIGINS else ())


def slab(name):
    scene = configs.cfg2_lsc()
    body = next(n for n in scene.root.children if n.name == "LSC")
    if name == "b_extension":
        body.volume_maps = [VolumeMap("reacted", (1, 1, 1), LOWER, UPPER, event="reacted")]
    if name in ("c_origin_wavelength", "d_origin_heatmap"):
        for label, normal in EDGES.items():
            hists = [Histogram("origin_wavelength", 400, 800, 40)]
            if name == "d_origin_heatmap":
                hists.append(Heatmap("origin_x", "origin_y", (-2.5, 2.5, 8), (-2.5, 2.5, 8)))
            body.recorders = list(body.recorders) + [Recorder(f"edge-{label}", event="escaping", facet=normal, histograms=hists)]
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
    base = out.get("b_extension_photons_per_s")
    for name in ("c_origin_wavelength", "d_origin_heatmap"):
        if base and name in scenes:
            out[f"{name}_over_b"] = out[f"{name}_photons_per_s"]["median"] / base["median"]
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
