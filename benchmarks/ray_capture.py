"""Cost of ray capture (`Recorder(..., capture=rows)`: the rays behind a recorder's count as 96-byte rows): photons/s of
the headline's 5 x 5 x 1 cm slab (benchmarks/configs.py cfg2_lsc) at 10^7 photons, tallies only, "fenced" (one
`engine.simulate` call, timed to its return, the download of the rows included):

  (a) no capture, on the smooth kernel variants;
  (b) no capture, on the extension variants the capture launches run on (a 1 x 1 x 1 concentration field of value 1
      traces bit for bit like none);
  (c) the four edge recorders captured;
  (d) one recorder that every photon fires (`exit` on the root) captured: the worst case for the cursor.

    python benchmarks/ray_capture.py [--photons N] [--repeats R]     # on a machine with an MI355X

Prints one JSON line: photons/s per case (fenced, and of the trace launch alone as the GPU timed it), rows captured, and
ns per captured row (time difference to (b) over the rows, both ways).  Cases (a) and (b) need no capture and run on a
commit without it; `--cases a_smooth,b_extension` runs them alone, as such a commit does.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pvtrace_amd import engine   # noqa: E402
from pvtrace_amd.engine import Recorder   # noqa: E402
from pvtrace_amd.material import ConcentrationGrid   # noqa: E402
from benchmarks import configs   # noqa: E402

LOWER, UPPER = (-2.5, -2.5, -0.5), (2.5, 2.5, 0.5)
EDGES = ("left", "right", "near", "far")
HAS_CAPTURE = "capture" in Recorder.__init__.__code__.co_varnames
CASES = ("a_smooth", "b_extension") + (("c_edges", "d_every_photon") if HAS_CAPTURE else ())


def slab(name, photons):
    scene = configs.cfg2_lsc()
    body = next(n for n in scene.root.children if n.name == "LSC")
    if name == "b_extension":
        grid = ConcentrationGrid(np.ones((1, 1, 1)), LOWER, UPPER)
        for component in body.geometry.material.components:
            component.concentration = grid
    if name == "c_edges":
        for rec in body.recorders:
            if rec.name in EDGES:
                rec.capture = photons // 4
    if name == "d_every_photon":
        scene.root.recorders = [Recorder("exit-all", event="exit", capture=photons)]
    return scene


def fenced(scene, n, seed):
    tic = time.perf_counter()
    result = engine.simulate(scene, n, seed=seed, record_every=0)
    return time.perf_counter() - tic, result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--photons", type=int, default=10 ** 7)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cases", default=",".join(CASES), help="comma-separated subset of the cases")
    args = ap.parse_args()
    cases = tuple(name for name in CASES if name in args.cases.split(","))
    if not engine.is_available():
        print("HIP engine not built or no GPU visible; run: python -c 'import __graft_entry__ as g; g.build()'")
        return 1
    scenes = {name: slab(name, args.photons) for name in cases}
    for scene in scenes.values():
        engine.simulate(scene, 100000, seed=1, record_every=0)   # load, upload, warm
    best = {name: float("inf") for name in scenes}
    kernel = {name: float("inf") for name in scenes}   # the trace launch alone, as the GPU timed it
    rows = {name: 0 for name in scenes}
    for r in range(args.repeats):   # alternate the cases, keep each one's best
        for name, scene in scenes.items():
            seconds, result = fenced(scene, args.photons, 7 + r)
            best[name] = min(best[name], seconds)
            kernel[name] = min(kernel[name], result.kernel_ms * 1e-3)
            rows[name] = sum(len(c) for c in getattr(result, "captures", {}).values())
            if HAS_CAPTURE:
                assert all(c.dropped == 0 for c in result.captures.values())
    out = {"photons": args.photons}
    for name in scenes:
        out[f"fenced_{name}_photons_per_s"] = args.photons / best[name]
        out[f"kernel_{name}_photons_per_s"] = args.photons / kernel[name]
    for name in cases:
        if name not in CASES[2:] or "b_extension" not in cases:
            continue
        out[f"{name}_rows"] = rows[name]
        out[f"ratio_{name}_over_b_extension"] = best["b_extension"] / best[name]
        out[f"{name}_ns_per_captured_row"] = (best[name] - best["b_extension"]) / max(rows[name], 1) * 1e9
        out[f"{name}_kernel_ns_per_captured_row"] = (kernel[name] - kernel["b_extension"]) / max(rows[name], 1) * 1e9
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
