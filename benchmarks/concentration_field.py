"""Cost of concentration fields (`ConcentrationGrid` on the volume components): photons/s of the headline's 5 x 5 x 1 cm
slab (benchmarks/configs.py cfg2_lsc) without a field (the smooth kernel variants), with a 1 x 1 x 1 field of value 1
(the field variants, no plane to cross), with a 1 x 1 x 16 through-thickness gradient and with a 32 x 32 x 4 printed
pattern (dye squares with clear gaps), at 10^7 photons, tallies only, "fenced" (one `engine.simulate` call, timed to
its return).  Every component of the slab carries the same field.  A short history run counts the lattice planes the
photons' free paths cross (per step inside the slab, from the cells of its two ends), which turns the difference in
time into a cost per cell crossing.

    python benchmarks/concentration_field.py [--photons N] [--repeats R]     # on a machine with an MI355X

Prints one JSON line: photons/s per scene, cells crossed per photon, and ps of device time per cell crossing against
the 1 x 1 x 1 field (ps of the whole GPU's throughput: time difference / photons / crossings).  The fields change the
absorption, so the photons of different scenes take different numbers of steps: the figures are per photon and per
crossing, not a like-for-like slowdown.
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
from pvtrace_amd.engine.compiler import compile_scene   # noqa: E402
from pvtrace_amd.material import ConcentrationGrid   # noqa: E402
from benchmarks import configs   # noqa: E402

LOWER, UPPER = (-2.5, -2.5, -0.5), (2.5, 2.5, 0.5)


def field(name):
    if name == "none":
        return None
    if name == "unit_1x1x1":
        return ConcentrationGrid(np.ones((1, 1, 1)), LOWER, UPPER)
    if name == "gradient_1x1x16":
        return ConcentrationGrid(np.linspace(0.1, 1.9, 16).reshape(1, 1, 16), LOWER, UPPER)
    ix, iy, _ = np.indices((32, 32, 4))
    return ConcentrationGrid(np.where((ix % 4 < 2) & (iy % 4 < 2), 2.0, 0.0), LOWER, UPPER)   # "pattern_32x32x4"


SCENES = ("none", "unit_1x1x1", "gradient_1x1x16", "pattern_32x32x4")


def slab(name):
    scene = configs.cfg2_lsc()
    body = next(n for n in scene.root.children if n.name == "LSC")
    grid = field(name)
    for component in body.geometry.material.components:
        component.concentration = grid
    return scene


def fenced(scene, n, seed):
    tic = time.perf_counter()
    engine.simulate(scene, n, seed=seed, record_every=0)
    return time.perf_counter() - tic


def crossings_per_photon(scene, grid, n=20000):
    """Lattice planes crossed per photon: per step that starts and ends inside the slab, the cells of its two ends."""
    if grid is None:
        return 0.0
    compiled = compile_scene(scene)
    w2l = compiled.world_to_local[compiled.node_names.index("LSC")]
    r = engine.simulate(scene, n, seed=3, record_every=1, max_events=512)
    counts = np.asarray(r.data["counts"])
    pos = np.asarray(r.data["position"]).reshape(counts.size, 512, 3)
    shape, h = np.array(grid.shape), grid.h
    total = 0
    for i, k in enumerate(counts):
        p = pos[i, :k] @ w2l[:3, :3].T + w2l[:3, 3]
        inside = np.all((p >= np.array(LOWER) - 1e-9) & (p <= np.array(UPPER) + 1e-9), axis=1)
        cell = np.clip(np.floor((p - grid.lower) / h), 0, shape - 1)
        both = inside[:-1] & inside[1:]
        total += int(np.abs(np.diff(cell, axis=0))[both].sum())
    return total / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--photons", type=int, default=10 ** 7)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    if not engine.is_available():
        print("HIP engine not built or no GPU visible; run: python -c 'import __graft_entry__ as g; g.build()'")
        return 1
    scenes = {name: slab(name) for name in SCENES}
    for scene in scenes.values():
        engine.simulate(scene, 100000, seed=1, record_every=0)   # load, upload, warm
    best = {name: float("inf") for name in scenes}
    for r in range(args.repeats):   # alternate the scenes, keep each one's best
        for name, scene in scenes.items():
            best[name] = min(best[name], fenced(scene, args.photons, 7 + r))
    out = {"photons": args.photons}
    for name in scenes:
        out[f"fenced_{name}_photons_per_s"] = args.photons / best[name]
    cross = {name: crossings_per_photon(scenes[name], field(name)) for name in scenes}
    for name in scenes:
        out[f"{name}_cells_crossed_per_photon"] = cross[name]
    out["ratio_unit_1x1x1_over_none"] = best["none"] / best["unit_1x1x1"]
    for name in ("gradient_1x1x16", "pattern_32x32x4"):
        out[f"ratio_{name}_over_none"] = best["none"] / best[name]
        if cross[name] > 0.0:
            out[f"{name}_ps_per_cell_crossing"] = (best[name] - best["unit_1x1x1"]) / args.photons / cross[name] * 1e12
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
