"""Cost of rough interfaces (`FresnelSurfaceDelegate(roughness=alpha)`, GGX microfacet normals): photons/s of the
headline's 5 x 5 x 1 cm slab (benchmarks/configs.py cfg2_lsc) with its surface smooth (alpha = 0: the scene of the
headline, traced by the smooth kernel variants) and at alpha = 0.05 and 0.3 (the rough variants), at 10^7 photons,
tallies only, "fenced" (one `engine.simulate` call, timed to its return).  A short history run counts the surface
events (REFLECT / TRANSMIT) per photon of each scene, which turns the difference in time into a cost per surface event.

    python benchmarks/rough_surface.py [--photons N] [--repeats R]     # on a machine with an MI355X

Prints one JSON line: photons/s per scene, surface events per photon, and the extra device time per surface event
against the smooth slab (ps of the whole GPU's throughput: 1 / rate difference / surface events).  A rough slab lets
more trapped light out, so its photons take fewer steps: the per-event figure compares time per surface event.
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
from pvtrace_amd.material import FresnelSurfaceDelegate   # noqa: E402
from benchmarks import configs   # noqa: E402

REFLECT, TRANSMIT = 1, 2
ALPHAS = (0.0, 0.05, 0.3)


def slab(alpha):
    scene = configs.cfg2_lsc()
    body = next(n for n in scene.root.children if n.name == "LSC")
    delegate = body.geometry.material.surface.delegate
    assert isinstance(delegate, FresnelSurfaceDelegate)
    if alpha > 0.0:   # (the LSC builder's delegate keeps its coatings: only the uncovered points are rough)
        delegate._roughness = float(alpha)
    return scene


def fenced(scene, n, seed):
    tic = time.perf_counter()
    engine.simulate(scene, n, seed=seed, record_every=0)
    return time.perf_counter() - tic


def surface_events_per_photon(scene, n=20000):
    r = engine.simulate(scene, n, seed=3, record_every=1, max_events=512)
    kind = np.asarray(r.data["kind"])
    return float(np.count_nonzero((kind == REFLECT) | (kind == TRANSMIT))) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--photons", type=int, default=10 ** 7)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    if not engine.is_available():
        print("HIP engine not built or no GPU visible; run: python -c 'import __graft_entry__ as g; g.build()'")
        return 1
    scenes = {f"alpha_{a:g}": slab(a) for a in ALPHAS}
    for scene in scenes.values():
        engine.simulate(scene, 100000, seed=1, record_every=0)   # load, upload, warm
    best = {name: float("inf") for name in scenes}
    for r in range(args.repeats):   # alternate the scenes, keep each one's best
        for name, scene in scenes.items():
            best[name] = min(best[name], fenced(scene, args.photons, 7 + r))
    out = {"photons": args.photons}
    for name in scenes:
        out[f"fenced_{name}_photons_per_s"] = args.photons / best[name]
    events = {name: surface_events_per_photon(scene) for name, scene in scenes.items()}
    for name in scenes:
        out[f"{name}_surface_events_per_photon"] = events[name]
    base = best["alpha_0"] / args.photons / events["alpha_0"]   # device time per surface event, smooth
    for name in scenes:
        if name != "alpha_0":
            out[f"ratio_{name}_over_smooth"] = best["alpha_0"] / best[name]
            out[f"{name}_extra_ps_per_surface_event"] = (best[name] / args.photons / events[name] - base) * 1e12
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
