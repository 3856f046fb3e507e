"""Cost of path-length maps (`VolumeMap(event="pathlength")`: the path photons travel per voxel, in fixed-point
integers): photons/s of the headline's 5 x 5 x 1 cm slab (benchmarks/configs.py cfg2_lsc) on the extension variants
with (a) an `absorbed` map of 32 x 32 x 4 alone, (b) a `pathlength` map of 32 x 32 x 4 added -- the launches now run
the kernels compiled with the walk --, (c) that map at 128 x 128 x 32 and (d) at 1 x 1 x 1 (one piece per segment, all on
ONE slot), at 10^7 photons, tallies only, "fenced" (one `engine.simulate` call, timed to its return), five windows, the
cases alternating.  The maps change no photon's history, so the cases trace the same photons.

    python benchmarks/pathlength_map.py [--photons N] [--repeats R]     # on a machine with an MI355X

Prints one JSON line: per case the median, least and greatest photons/s of its windows, the ratios (b) / (a) and
(c) / (b) of the median times, and for (d) the nanoseconds per piece: (median time of (d) - that of (a)) / segments,
the segments counted as the pieces of the 1 x 1 x 1 map's walk (`pieces_per_photon` x photons; a segment inside one cell
is one piece).  The piece count comes from a history launch of 20 000 photons walked on the host.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pvtrace_amd import engine   # noqa: E402
from pvtrace_amd.engine import VolumeMap   # noqa: E402
from pvtrace_amd.engine.tally import path_map_slots   # noqa: E402
from benchmarks import configs   # noqa: E402

LOWER, UPPER = (-2.5, -2.5, -0.5), (2.5, 2.5, 0.5)
CASES = {"a_absorbed_32x32x4": None, "b_pathlength_32x32x4": (32, 32, 4), "c_pathlength_128x128x32": (128, 128, 32),
         "d_pathlength_1x1x1": (1, 1, 1)}


def slab(shape):
    scene = configs.cfg2_lsc()
    body = next(n for n in scene.root.children if n.name == "LSC")
    body.volume_maps = [VolumeMap("absorbed", (32, 32, 4), LOWER, UPPER)]
    if shape is not None:
        body.volume_maps.append(VolumeMap("path", shape, LOWER, UPPER, event="pathlength"))
    return scene


def fenced(scene, n, seed):
    tic = time.perf_counter()
    result = engine.simulate(scene, n, seed=seed, record_every=0)
    return time.perf_counter() - tic, result


def pieces_per_photon(scene, n=20_000):
    """Pieces the 1 x 1 x 1 map's walk adds per photon, counted on the host from the histories of a small launch."""
    result = engine.simulate(scene, n, seed=7, record_every=1, max_events=512)
    _, pieces = path_map_slots(result.compiled, result.histories())
    return float(pieces.sum()) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--photons", type=int, default=10 ** 7)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not engine.is_available():
        print("HIP engine not built or no GPU visible; run: python -c 'import __graft_entry__ as g; g.build()'")
        return 1
    scenes = {name: slab(shape) for name, shape in CASES.items()}
    for scene in scenes.values():
        engine.simulate(scene, 100000, seed=1, record_every=0)   # load, upload, warm
    times = {name: [] for name in scenes}
    units = {}
    for r in range(args.repeats):   # alternate the cases
        for name, scene in scenes.items():
            seconds, result = fenced(scene, args.photons, 7 + r)
            times[name].append(seconds)
            if "path" in result.volume_maps:
                units[name] = result.volume_maps["path"].total
    out = {"photons": args.photons, "windows": args.repeats}
    median = {name: statistics.median(t) for name, t in times.items()}
    for name, t in times.items():
        out[f"fenced_{name}_photons_per_s"] = {"median": args.photons / median[name], "min": args.photons / max(t),
                                               "max": args.photons / min(t)}
    out["time_ratio_b_over_a"] = median["b_pathlength_32x32x4"] / median["a_absorbed_32x32x4"]
    out["time_ratio_c_over_b"] = median["c_pathlength_128x128x32"] / median["b_pathlength_32x32x4"]
    per_photon = pieces_per_photon(scenes["d_pathlength_1x1x1"])
    out["d_pieces_per_photon"] = per_photon
    out["d_ns_per_piece"] = (median["d_pathlength_1x1x1"] - median["a_absorbed_32x32x4"]) / (per_photon * args.photons) * 1e9
    out["path_cm_per_photon"] = {name: u * 2.0 ** -30 / args.photons for name, u in units.items()}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
