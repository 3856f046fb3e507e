"""Cost of a coating reflectivity table: photons/s of the selective-mirror slab (tests/coating_table_scene.py: a Lumogen F
Red slab whose top face carries R(wavelength, angle of incidence)) against the same slab with a scalar coating of the
same placement and modes, at 10^7 photons, tallies only; a table that holds the scalar's value everywhere isolates the
cost of the lookup (same photon paths).  Two ways of running: "fenced" (one `engine.simulate` call,
timed to its return) and "streamed" (`engine.simulate_stream` in bundles of 10^6, timed over the whole stream).  The
table is looked up only when a photon meets the coated face (a bracket on each axis and an arc cosine).

    python benchmarks/coating_table.py [--photons N] [--repeats R]     # on a machine with an MI355X

Prints one JSON line: photons/s per scene and way, and the ratios (> 1: faster than the scalar coating).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pvtrace_amd import (   # noqa: E402
    Box, CoatedSurfaceDelegate, Coating, Light, Luminophore, Material, Node, ReflectivityTable, Scene, Surface,
    rectangular_mask,
)
from pvtrace_amd import engine   # noqa: E402
from pvtrace_amd.data import lumogen_f_red_305   # noqa: E402
from pvtrace_amd.engine import Recorder   # noqa: E402
from pvtrace_amd.light import ConstantWavelengthMask   # noqa: E402
from tests import coating_table_scene as S   # noqa: E402


def slab(reflectivity):
    delegate = CoatedSurfaceDelegate([Coating((0, 0, 1), reflectivity=reflectivity)])
    scene, node = S.build(Node, Scene, Box, Material, Surface, Light, rectangular_mask, ConstantWavelengthMask(S.PUMP_NM),
                          S.components(Luminophore, lumogen_f_red_305), delegate=delegate)
    node.recorders = [Recorder(f"{k}", event="escaping", facet=f)
                      for k, f in (("top", (0, 0, 1)), ("bottom", (0, 0, -1)))] + [Recorder("lost", event="lost")]
    return scene


def fenced(scene, n, seed):
    tic = time.perf_counter()
    engine.simulate(scene, n, seed=seed, record_every=0)
    return time.perf_counter() - tic


def streamed(scene, n, seed, bundle=1000000):
    tic = time.perf_counter()
    for _ in engine.simulate_stream(scene, n, bundle=bundle, seed=seed, record_every=0):
        pass
    return time.perf_counter() - tic


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--photons", type=int, default=10 ** 7)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    if not engine.is_available():
        print("HIP engine not built or no GPU visible; run: python -c 'import __graft_entry__ as g; g.build()'")
        return 1
    table = ReflectivityTable(S.MIRROR_WAVELENGTH, S.MIRROR_VALUE, angle=S.MIRROR_ANGLE)
    # "constant_table" holds 0.5 everywhere: the same photon paths as "scalar", bit for bit -- their ratio is the cost of
    # the lookup alone; "table" (the selective mirror) also changes the paths
    constant = ReflectivityTable(S.MIRROR_WAVELENGTH, 0.5 + 0.0 * S.MIRROR_VALUE, angle=S.MIRROR_ANGLE)
    scenes = {"table": slab(table), "constant_table": slab(constant), "scalar": slab(0.5)}
    for scene in scenes.values():
        engine.simulate(scene, 100000, seed=1, record_every=0)   # load, upload, warm
    out = {"photons": args.photons}
    for way, fn in (("fenced", fenced), ("streamed", streamed)):
        best = {name: float("inf") for name in scenes}
        for r in range(args.repeats):   # alternate the two scenes, keep each one's best
            for name, scene in scenes.items():
                best[name] = min(best[name], fn(scene, args.photons, 7 + r))
        for name in scenes:
            out[f"{way}_{name}_photons_per_s"] = args.photons / best[name]
        out[f"{way}_ratio_table_over_scalar"] = best["scalar"] / best["table"]
        out[f"{way}_ratio_constant_table_over_scalar"] = best["scalar"] / best["constant_table"]
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
