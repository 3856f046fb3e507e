"""Cost of volume maps (`VolumeMap`: per-voxel integer tallies of a node's volume events): photons/s of the headline's
5 x 5 x 1 cm slab (benchmarks/configs.py cfg2_lsc) without a map (the smooth kernel variants), with a 1 x 1 x 1
concentration field of value 1 and no map (the extension variants the maps' launches run on, paying the field's march
instead), with a `reacted` map of 1 x 1 x 1 (the slab has no Reactor: the maps' code runs at every absorption and counts
nothing), and with one `absorbed` map of 1 x 1 x 1 (every event on ONE slot: the worst contention), of 32 x 32 x 4,
of 128 x 128 x 32, and with an `absorbed` and an `emitted` map of 32 x 32 x 4 x 16 wavelength bins, at 10^7 photons,
tallies only, "fenced" (one `engine.simulate` call, timed to its return).  The maps change no photon's history, so the
scenes trace the same photons; the maps' own totals give the events counted, which turns the difference in time against
the map that counts nothing into a device time per counted event.

    python benchmarks/volume_map.py [--photons N] [--repeats R]     # on a machine with an MI355X

Prints one JSON line: photons/s per case, events counted per photon, and ps of device time per counted event (ps of the
whole GPU's throughput: time difference / events counted).
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
from pvtrace_amd.engine import VolumeMap   # noqa: E402
from pvtrace_amd.material import ConcentrationGrid   # noqa: E402
from benchmarks import configs   # noqa: E402

LOWER, UPPER = (-2.5, -2.5, -0.5), (2.5, 2.5, 0.5)
WAVELENGTH = (300.0, 900.0, 16)


def maps(name):
    if name == "absorbed_1x1x1":
        return [VolumeMap("absorbed", (1, 1, 1), LOWER, UPPER)]
    if name == "absorbed_32x32x4":
        return [VolumeMap("absorbed", (32, 32, 4), LOWER, UPPER)]
    if name == "absorbed_128x128x32":
        return [VolumeMap("absorbed", (128, 128, 32), LOWER, UPPER)]
    if name == "absorbed_emitted_32x32x4x16":
        return [VolumeMap("absorbed", (32, 32, 4), LOWER, UPPER, wavelength=WAVELENGTH),
                VolumeMap("emitted", (32, 32, 4), LOWER, UPPER, event="emitted", wavelength=WAVELENGTH)]
    if name == "reacted_counts_nothing":
        return [VolumeMap("reacted", (1, 1, 1), LOWER, UPPER, event="reacted")]
    return []   # "none", "extension_no_map"


CASES = ("none", "extension_no_map", "reacted_counts_nothing", "absorbed_1x1x1", "absorbed_32x32x4", "absorbed_128x128x32",
         "absorbed_emitted_32x32x4x16")


def slab(name):
    scene = configs.cfg2_lsc()
    body = next(n for n in scene.root.children if n.name == "LSC")
    if name == "extension_no_map":   # (a unit field traces bit for bit like no field, on the extension variants)
        grid = ConcentrationGrid(np.ones((1, 1, 1)), LOWER, UPPER)
        for component in body.geometry.material.components:
            component.concentration = grid
    body.volume_maps = maps(name)
    return scene


def fenced(scene, n, seed):
    tic = time.perf_counter()
    result = engine.simulate(scene, n, seed=seed, record_every=0)
    return time.perf_counter() - tic, result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--photons", type=int, default=10 ** 7)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    if not engine.is_available():
        print("HIP engine not built or no GPU visible; run: python -c 'import __graft_entry__ as g; g.build()'")
        return 1
    scenes = {name: slab(name) for name in CASES}
    for scene in scenes.values():
        engine.simulate(scene, 100000, seed=1, record_every=0)   # load, upload, warm
    best = {name: float("inf") for name in scenes}
    counted = {name: 0 for name in scenes}
    for r in range(args.repeats):   # alternate the cases, keep each one's best
        for name, scene in scenes.items():
            seconds, result = fenced(scene, args.photons, 7 + r)
            best[name] = min(best[name], seconds)
            counted[name] = sum(m.total for m in result.volume_maps.values())
    out = {"photons": args.photons}
    for name in scenes:
        out[f"fenced_{name}_photons_per_s"] = args.photons / best[name]
    out["ratio_extension_no_map_over_none"] = best["none"] / best["extension_no_map"]
    out["ratio_reacted_counts_nothing_over_none"] = best["none"] / best["reacted_counts_nothing"]
    for name in CASES[3:]:
        out[f"{name}_events_counted_per_photon"] = counted[name] / args.photons
        out[f"ratio_{name}_over_none"] = best["none"] / best[name]
        out[f"{name}_ps_per_counted_event"] = (best[name] - best["reacted_counts_nothing"]) / counted[name] * 1e12
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
